// pp2_masked.h -- admission of a coded model to the masked-support form of the
// tile-resident loop (pp2_resident.hip).  Host code with no
// HIP call in it (tests/masked_admit_check.cpp runs it stand-alone).
//
// On a generated model every off-centre transition weight is either the base
// kernel's constant or +0, and it is +0 exactly when the cell it points to, or
// the cell itself, is blocked (occupied, or off the grid).  Where that holds
// the resident loop keeps b and J of blocked cells as +0 in its LDS planes and
// takes the weight as a wave-uniform scalar: fmaf(w, +0, acc) == acc ==
// fmaf(+0, v, acc) for the finite w, v and the never -0 acc of the sparse rows.
// masked_admit decides it, comparing bit patterns:
//   * an entry is blocked (F = 1) when every off-centre support weight of every
//     action is +0 and the pair (fl(gamma * T centre), C) is the same for all
//     nine actions;
//   * w_main (the weight action a gives the cell it points to, T index a) and
//     w_side (its other off-centre support cells) are the same for all eight
//     move actions;
//   * for every cell x of rows [-1, rows] (pads included), every move action a
//     and every off-centre support index i,
//       T[x][a][i] == (F(x) || F(x + off_i)) ? +0 : w(a, i),
//     cells off those rows or columns counting as F = 1.
// The relation is checked per cell through its entry: an entry that is not
// blocked fixes, weight by weight, which of its 8 neighbours must be blocked
// (+0) and which must not (w); entries whose actions disagree about a
// neighbour, or hold any other weight, reject the model.
#pragma once
#include <stdint.h>

#include <cstring>
#include <vector>

namespace pp2 {

struct MaskedModel {
  bool ok = false;
  float w_main = 0.0f, w_side = 0.0f;  // raw weights (+0 when no entry holds one)
  std::vector<uint8_t> blocked;        // F per entry
};

namespace masked_detail {
// (the base kernels' supports: pp2_internal.h kSup / kSupN)
constexpr int kN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
constexpr int kS[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5}, {0, 3, 4, 6}, {4, 0, 0, 0},
                          {2, 4, 5, 8}, {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};
inline uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}
}  // namespace masked_detail

namespace masked_detail {
// The per-entry half of the admission: F per entry, else the neighbours
// (bit i, T index i) that must be blocked, and the two weights.
struct MaskedEntries {
  bool ok = false;
  std::vector<uint8_t> blocked;
  std::vector<uint16_t> need;
  uint32_t wm = 0u, ws = 0u;
};

inline MaskedEntries masked_entries(const float* dict, int E, int dict_row, float gamma) {
  MaskedEntries m;
  m.blocked.assign((size_t)E, 0);
  m.need.assign((size_t)E, 0);
  bool have_main = false, have_side = false;
  uint32_t& wm = m.wm;
  uint32_t& ws = m.ws;
  for (int e = 0; e < E; ++e) {
    const float* d = dict + (size_t)e * dict_row;
    bool all_zero = true, same = true;
    const uint32_t g0 = bits(gamma * d[4]), c0 = bits(d[9]);
    for (int a = 0; a < 9; ++a) {
      for (int j = 0; j < kN[a]; ++j)
        if (kS[a][j] != 4 && bits(d[a * 10 + kS[a][j]]) != 0u) all_zero = false;
      if (bits(gamma * d[a * 10 + 4]) != g0 || bits(d[a * 10 + 9]) != c0) same = false;
    }
    if (all_zero && same) {
      m.blocked[e] = 1;
      continue;
    }
    // 0: not seen, 1: +0 (neighbour blocked), 2: the constant (neighbour free)
    int state[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < 9; ++a) {
      if (a == 4) continue;
      for (int j = 0; j < kN[a]; ++j) {
        const int i = kS[a][j];
        if (i == 4) continue;
        const uint32_t t = bits(d[a * 10 + i]);
        int st;
        if (t == 0u) {
          st = 1;
        } else {
          st = 2;
          bool& have = i == a ? have_main : have_side;
          uint32_t& w = i == a ? wm : ws;
          if (!have) {
            have = true;
            w = t;
          } else if (w != t) {
            return m;
          }
        }
        if (state[i] != 0 && state[i] != st) return m;
        state[i] = st;
      }
    }
    uint16_t nb = 0;
    for (int i = 0; i < 9; ++i)
      if (i != 4 && state[i] == 1) nb |= (uint16_t)(1u << i);
    m.need[e] = nb;
  }
  m.ok = true;
  return m;
}

// The relation, cell by cell, over rows [r_lo, r_hi) of a plane of R rows of
// wp codes: F of the 8 neighbours against the entry's need, in two passes
// without a data-dependent branch -- h = F(x - 1) | F(x) << 1 | F(x + 1) << 2
// per cell of rows [r_lo - 1, r_hi] (the plane's own rows where it has them, a
// row of 7s above and below the plane), then the three rows' triples against
// the need (a blocked cell compares nothing).
inline bool masked_cells(const uint16_t* code, int wp, int R, int E, const uint8_t* bl,
                         const uint16_t* nd, int r_lo, int r_hi) {
  if (r_lo < 0) r_lo = 0;
  if (r_hi > R) r_hi = R;
  if (r_lo >= r_hi) return true;
  const int nr = r_hi - r_lo;
  std::vector<uint8_t> h((size_t)(nr + 2) * wp, 7);  // h row j: plane row r_lo - 1 + j
  unsigned bad = 0;
  for (int r = r_lo > 0 ? r_lo - 1 : 0; r < (r_hi < R ? r_hi + 1 : R); ++r) {
    const uint16_t* cr = code + (size_t)r * wp;
    uint8_t* __restrict hr = &h[(size_t)(r - r_lo + 1) * wp];
    unsigned prev = 1, cur = cr[0] < E ? bl[cr[0]] : 1;
    bad |= cr[0] >= E;
    for (int x = 0; x < wp; ++x) {
      unsigned next = 1;
      if (x + 1 < wp) {
        const unsigned c = cr[x + 1];
        bad |= c >= (unsigned)E;
        next = bl[c < (unsigned)E ? c : 0];
      }
      hr[x] = (uint8_t)(prev | cur << 1 | next << 2);
      prev = cur;
      cur = next;
    }
  }
  if (bad) return false;
  for (int r = r_lo; r < r_hi; ++r) {
    const uint16_t* cr = code + (size_t)r * wp;
    const uint8_t* h0 = &h[(size_t)(r - r_lo) * wp];
    const uint8_t* h1 = h0 + wp;
    const uint8_t* h2 = h1 + wp;
    for (int x = 0; x < wp; ++x) {
      const unsigned own = (h1[x] >> 1) & 1u;
      const unsigned nb = h0[x] | (h1[x] & 1u) << 3 | (h1[x] & 4u) << 3 | (unsigned)h2[x] << 6;
      bad |= (nb ^ nd[cr[x]]) & (own - 1u);
    }
  }
  return !bad;
}
}  // namespace masked_detail

// code: the code plane at (row -1, x 0), rows + 2 rows of wp codes (< E);
// dict: E rows of dict_row floats, [a][T_a0 .. T_a8, C_a] at 10 * a.
inline MaskedModel masked_admit(const uint16_t* code, int wp, int rows, const float* dict, int E,
                                int dict_row, float gamma) {
  using namespace masked_detail;
  MaskedModel m;
  if (E <= 0 || wp <= 0 || rows <= 0) return m;
  MaskedEntries en = masked_entries(dict, E, dict_row, gamma);
  m.blocked.swap(en.blocked);
  if (!en.ok) return m;
  if (!masked_cells(code, wp, rows + 2, E, m.blocked.data(), en.need.data(), 0, rows + 2))
    return m;
  std::memcpy(&m.w_main, &en.wm, 4);
  std::memcpy(&m.w_side, &en.ws, 4);
  m.ok = true;
  return m;
}

// The windowed form, for a plane that masked_admit admitted before codes of
// its rows [r_lo + 1, r_hi - 1) changed (r_lo, r_hi: rows of the plane, row 0
// being the grid's row -1; clipped to it): the entries' half as above, the
// cells' relation over rows [r_lo, r_hi) alone, read against their true
// neighbour rows r_lo - 1 and r_hi.  True iff masked_admit would still admit
// the plane, given that every row outside the window still satisfies it.
inline bool masked_admit_window(const uint16_t* code, int wp, int rows, const float* dict, int E,
                                int dict_row, float gamma, int r_lo, int r_hi) {
  using namespace masked_detail;
  if (E <= 0 || wp <= 0 || rows <= 0) return false;
  const MaskedEntries en = masked_entries(dict, E, dict_row, gamma);
  if (!en.ok) return false;
  return masked_cells(code, wp, rows + 2, E, en.blocked.data(), en.need.data(), r_lo, r_hi);
}

}  // namespace pp2
