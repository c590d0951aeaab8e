// Stand-alone host check of pp2::masked_admit_window (path_planning_2d_amd/
// csrc/pp2_masked.h), the windowed re-check a map update runs instead of the
// whole-plane masked_admit.  Built by tests/test_masked_window_cpu.py with the
// host compiler and -fsanitize=address,undefined as its own executable; no
// GPU, no HIP.
//
// Planes are 12 x 16 codes (10 grid rows and the two halo rows; 13 columns and
// 3 pads, or 16 columns and no pad) over dictionaries of generated models (the
// generator restated per cell as in masked_admit_check.cpp).  The oracle is
// the admission rule's own statement, evaluated cell by cell from the
// dictionary rows -- T[x][a][i] == (F(x) || F(x + off_i)) ? +0 : w(a, i),
// cells off the plane counting as F = 1 -- which gives, per plane row, whether
// some cell of that row breaks it.  A window [lo, hi) must be admitted exactly
// when none of its rows does:
//   * admitted planes: every window position, the clipped ones included, is
//     admitted -- free cells on both sides of every window edge, so "off the
//     window = blocked" would reject;
//   * a map change re-coded with the same dictionary: the window the runtime
//     derives from the changed rows agrees with masked_admit on the new plane;
//   * one deliberately wrong cell (a free cell coded as a blocked entry, with
//     free cells above and below it) in plane row r: rows r - 1, r and r + 1
//     break; every window is held to the oracle, and the three named ones --
//     the cell inside the window, just below it, and in the row above it --
//     must reject, while windows clear of the three rows must admit.
// Exit status 0 when every case holds.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "pp2_masked.h"

namespace {

constexpr int kRow = 108;
constexpr float kGamma = 0.95f;

void base_kernel(int u, float* tp) {
  for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
  static const int sup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5}, {0, 3, 4, 6}, {4, 4, 4, 4},
                                {2, 4, 5, 8}, {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};
  if (u == 4) {
    tp[4] = 1.0f;
    return;
  }
  for (int j = 0; j < 4; ++j) tp[sup[u][j]] = 0.1f;
  tp[u] = 0.7f;
}

// (H + 2) x wp tuples of 90 floats, row -1 first; halo rows and pads zero
std::vector<float> generate(const std::vector<uint8_t>& map, int H, int W, int wp, int gx, int gy) {
  std::vector<float> cell((size_t)(H + 2) * wp * 90, 0.0f);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t lm[9];
      for (int i = 0; i < 9; ++i) {
        const int nx = x + i % 3 - 1, ny = y + i / 3 - 1;
        lm[i] = (nx < 0 || nx >= W || ny < 0 || ny >= H) ? 1 : map[(size_t)ny * W + nx];
      }
      float* d = &cell[((size_t)(y + 1) * wp + x) * 90];
      for (int u = 0; u < 9; ++u) {
        float tp[9], nm[9];
        base_kernel(u, tp);
        for (int i = 0; i < 9; ++i) nm[i] = lm[4] == 1 ? (i == 4 ? 1.0f : 0.0f) : tp[i];
        for (int i = 0; i < 9; ++i)
          if (lm[i] == 1 && i != 4) {
            tp[4] += tp[i];
            tp[i] = 0.0f;
          }
        if (lm[4] == 1) {
          for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
          tp[4] = 1.0f;
        }
        float c = 0.0f;
        for (int i = 0; i < 9; ++i) c = __builtin_fmaf(lm[i] == 1 ? 2.0f : 1.0f, nm[i], c);
        if (u == 4) c = (x == gx && y == gy) ? 0.0f : 2.0f;
        for (int i = 0; i < 9; ++i) d[u * 10 + i] = tp[i];
        d[u * 10 + 9] = c;
      }
    }
  return cell;
}

// one dictionary shared by successive planes, as after a map update
struct Dict {
  std::map<std::vector<uint32_t>, int> ids;
  std::vector<float> rows;
  int E = 0;
  std::vector<uint16_t> encode(const std::vector<float>& cell) {
    std::vector<uint16_t> code(cell.size() / 90);
    for (size_t i = 0; i < code.size(); ++i) {
      std::vector<uint32_t> key(90);
      std::memcpy(key.data(), &cell[i * 90], 360);
      auto it = ids.find(key);
      if (it == ids.end()) {
        it = ids.emplace(key, E++).first;
        rows.resize((size_t)E * kRow, 0.0f);
        std::memcpy(&rows[(size_t)(E - 1) * kRow], &cell[i * 90], 360);
      }
      code[i] = (uint16_t)it->second;
    }
    return code;
  }
};

std::vector<uint8_t> scatter_map(int H, int W, unsigned seed, int percent) {
  std::vector<uint8_t> map((size_t)H * W, 0);
  unsigned s = seed;
  for (auto& v : map) {
    s = s * 1664525u + 1013904223u;
    v = (s >> 16) % 100 < (unsigned)percent;
  }
  return map;
}

uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

// The rule as stated, per plane row: does some cell of the row break it?
// F and the weights come from the whole-plane admission of a plane over the
// same dictionary.
std::vector<bool> rows_broken(const std::vector<uint16_t>& code, int wp, int R, const Dict& d,
                              const pp2::MaskedModel& mm) {
  static const int kN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
  static const int kS[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5}, {0, 3, 4, 6}, {4, 0, 0, 0},
                               {2, 4, 5, 8}, {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};
  auto F = [&](int r, int x) {
    if (r < 0 || r >= R || x < 0 || x >= wp) return true;
    return mm.blocked[code[(size_t)r * wp + x]] != 0;
  };
  std::vector<bool> broken((size_t)R, false);
  for (int r = 0; r < R; ++r)
    for (int x = 0; x < wp; ++x) {
      if (F(r, x)) continue;  // (a blocked cell holds no off-centre weight: the entry's own test)
      const float* row = &d.rows[(size_t)code[(size_t)r * wp + x] * kRow];
      for (int a = 0; a < 9; ++a) {
        if (a == 4) continue;
        for (int j = 0; j < kN[a]; ++j) {
          const int i = kS[a][j];
          if (i == 4) continue;
          const bool blocked = F(r + i / 3 - 1, x + i % 3 - 1);
          const uint32_t want = blocked ? 0u : bits(i == a ? mm.w_main : mm.w_side);
          if (bits(row[a * 10 + i]) != want) broken[(size_t)r] = true;
        }
      }
    }
  return broken;
}

int fails = 0;
void expect(bool ok, const char* what, int a = -1, int b = -1) {
  if (!ok) {
    std::printf("FAIL: %s (%d, %d)\n", what, a, b);
    ++fails;
  }
}

bool window(const std::vector<uint16_t>& code, int wp, int H, const Dict& d, int lo, int hi) {
  return pp2::masked_admit_window(code.data(), wp, H, d.rows.data(), d.E, kRow, kGamma, lo, hi);
}

// every window position against the per-row oracle; returns the windows checked
int all_windows(const std::vector<uint16_t>& code, int wp, int H, const Dict& d,
                const std::vector<bool>& broken, const char* what) {
  const int R = H + 2;
  int n = 0;
  for (int lo = -2; lo <= R + 1; ++lo)
    for (int hi = lo + 1; hi <= R + 3; ++hi) {
      bool want = true;
      for (int r = lo < 0 ? 0 : lo; r < (hi > R ? R : hi); ++r) want = want && !broken[(size_t)r];
      expect(window(code, wp, H, d, lo, hi) == want, what, lo, hi);
      ++n;
    }
  return n;
}

void geometry(int H, int W, int wp, unsigned seed0) {
  const int R = H + 2;
  for (unsigned seed = seed0; seed < seed0 + 6; ++seed) {
    std::vector<uint8_t> map = scatter_map(H, W, seed, 25);
    // a free 5 x 5 block for the wrong-cell cases, centre (cy, cx)
    const int cy = 5, cx = 6;
    for (int y = cy - 2; y <= cy + 2; ++y)
      for (int x = cx - 2; x <= cx + 2; ++x) map[(size_t)y * W + x] = 0;
    map[0] = 1;  // (an occupied cell: a blocked entry that is not the halo's)
    const int gx = 2, gy = 8;
    map[(size_t)gy * W + gx] = 0;
    Dict d;
    std::vector<uint16_t> code = d.encode(generate(map, H, W, wp, gx, gy));
    const pp2::MaskedModel mm =
        pp2::masked_admit(code.data(), wp, H, d.rows.data(), d.E, kRow, kGamma);
    expect(mm.ok, "generated plane admitted", (int)seed);
    if (!mm.ok) continue;
    std::vector<bool> none = rows_broken(code, wp, R, d, mm);
    for (int r = 0; r < R; ++r) expect(!none[(size_t)r], "oracle: an admitted plane breaks no row", r);
    all_windows(code, wp, H, d, none, "admitted plane: every window admitted");

    // a map change in grid rows [ya, yb), re-coded over the same (growing)
    // dictionary: the runtime's window is plane rows [ya, yb + 2)
    for (int ya = 0; ya < H; ya += 3) {
      const int yb = ya + 2 < H ? ya + 2 : H;
      std::vector<uint8_t> m2 = map;
      for (int y = ya; y < yb; ++y)
        for (int x = 1; x < W; x += 2) m2[(size_t)y * W + x] ^= 1;
      m2[(size_t)gy * W + gx] = 0;
      std::vector<uint16_t> c2 = d.encode(generate(m2, H, W, wp, gx, gy));
      const bool whole = pp2::masked_admit(c2.data(), wp, H, d.rows.data(), d.E, kRow, kGamma).ok;
      expect(whole, "changed plane admitted by masked_admit", ya);
      // (model cells change in rows [ya - 1, yb]: the dilated rectangle)
      const int lo = (ya > 0 ? ya - 1 : 0), hi = (yb < H ? yb + 1 : H) + 2;
      expect(window(c2, wp, H, d, lo, hi) == whole, "changed plane: window == whole", ya);
    }

    // one wrong cell: the free centre cell coded as the occupied cell's entry
    const pp2::MaskedModel m1 =
        pp2::masked_admit(code.data(), wp, H, d.rows.data(), d.E, kRow, kGamma);
    const int r = cy + 1;  // its plane row
    std::vector<uint16_t> bad = code;
    const uint16_t blocked_code = code[(size_t)1 * wp + 0];  // grid cell (0, 0), occupied
    expect(m1.ok && m1.blocked[blocked_code] == 1 && m1.blocked[code[(size_t)r * wp + cx]] == 0,
           "(the wrong cell turns a free cell into a blocked one)");
    bad[(size_t)r * wp + cx] = blocked_code;
    expect(!pp2::masked_admit(bad.data(), wp, H, d.rows.data(), d.E, kRow, kGamma).ok,
           "one wrong cell: rejected by masked_admit");
    const std::vector<bool> br = rows_broken(bad, wp, R, d, m1);
    expect(br[(size_t)r - 1] && br[(size_t)r + 1], "oracle: the rows above and below break");
    for (int q = 0; q < R; ++q)
      if (q < r - 1 || q > r + 1) expect(!br[(size_t)q], "oracle: no other row breaks", q);
    all_windows(bad, wp, H, d, br, "one wrong cell: every window against the oracle");
    expect(!window(bad, wp, H, d, r, r + 1) || !br[(size_t)r], "wrong cell inside the window");
    expect(!window(bad, wp, H, d, r - 2, r + 3), "wrong cell inside a wider window: rejected");
    expect(!window(bad, wp, H, d, r - 1, r), "wrong cell just below the window: rejected");
    expect(!window(bad, wp, H, d, r + 1, r + 2), "wrong cell in the row above the window: rejected");
    expect(window(bad, wp, H, d, 0, r - 1), "window clear above: admitted");
    expect(window(bad, wp, H, d, r + 2, R), "window clear below: admitted");
  }
}

}  // namespace

int main() {
  geometry(10, 13, 16, 3u);   // pad columns
  geometry(10, 16, 16, 40u);  // a grid as wide as its row stride
  if (fails == 0) std::printf("masked_admit_window: all cases hold\n");
  return fails == 0 ? 0 : 1;
}
