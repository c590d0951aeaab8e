// Stand-alone host check of the path gates in path_planning_2d_amd/csrc/
// pp2_dict_props.h: which dictionaries and states may use the sparse rows, the
// tile-resident loop and the tile-resident sweeps.  Built by tests/
// test_resident_gates_cpu.py with the host compiler and
// -fsanitize=address,undefined as its own executable; no GPU, no HIP.
//
// It feeds the scan made-up dictionaries -- a generated-like one and one
// violation at a time -- and asserts the truth table row by row.  The
// predicates as they stood before the header existed are transcribed below
// (namespace before); the program prints which rows they get wrong
// ("before: ..." lines, pinned by the Python test) without failing on them.
// Exit status 0 when every row holds for the header.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pp2_dict_props.h"

namespace {

constexpr int kRow = 108;  // floats per dictionary row ([a][T0..T8, C] at 10 a, L at 90)
constexpr int kL = 90;
const int kSupN[9] = {4, 4, 4, 4, 1, 4, 4, 4, 4};
const int kSup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5}, {0, 3, 4, 6}, {4, 0, 0, 0},
                        {2, 4, 5, 8}, {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};

using Dict = std::vector<float>;

// a free cell with free neighbours, a blocked cell, the goal
void add_entry(Dict& d, int kind, float l0 = 0.05f) {
  const size_t o = d.size();
  d.resize(o + kRow, 0.0f);
  float* e = &d[o];
  for (int a = 0; a < 9; ++a) {
    if (kind == 1 || a == 4) {
      e[a * 10 + 4] = 1.0f;
    } else {
      for (int j = 0; j < 4; ++j) e[a * 10 + kSup[a][j]] = 0.1f;
      e[a * 10 + a] = 0.7f;
    }
    e[a * 10 + 9] = kind == 1 ? 2.0f : a == 4 ? (kind == 2 ? 0.0f : 2.0f) : 1.0f;
  }
  for (int z = 0; z < 16; ++z) e[kL + z] = z == 0 ? l0 : 0.0625f;
}

Dict clean() {
  Dict d;
  add_entry(d, 0);
  add_entry(d, 1);
  add_entry(d, 2);
  add_entry(d, 0, 0.25f);
  return d;
}

// The gates as pp2_runtime.cpp had them before pp2_dict_props.h
// (build_model_dict's scan, coded_active, resident_model_ok, solve_plan_ok
// without its plan lookup), transcribed once.
namespace before {
struct Props {
  bool t_finite, tl_nonneg, sparse, rfact;
};
bool fnn(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b < 0x7f800000u;
}
Props scan(const Dict& dh, float gam) {
  const int E = (int)(dh.size() / kRow);
  Props p{true, true, false, false};
  for (int e = 0; e < E; ++e)
    for (int a = 0; a < 9; ++a)
      for (int i = 0; i < 9; ++i)
        if (!std::isfinite(dh[(size_t)e * kRow + a * 10 + i])) p.t_finite = false;
  for (int e = 0; e < E; ++e) {
    for (int a = 0; a < 9; ++a)
      for (int i = 0; i < 9; ++i)
        if (!fnn(dh[(size_t)e * kRow + a * 10 + i])) p.tl_nonneg = false;
    for (int z = 0; z < 16; ++z)
      if (!fnn(dh[(size_t)e * kRow + kL + z])) p.tl_nonneg = false;
  }
  bool sparse = gam >= 0.0f && gam < 1.0f;
  double cmax = 0.0;
  for (int e = 0; e < E && sparse; ++e)
    for (int a = 0; a < 9; ++a) {
      const float cv = dh[(size_t)e * kRow + a * 10 + 9];
      if (!fnn(cv)) {
        sparse = false;
        break;
      }
      cmax = cv > cmax ? cv : cmax;
    }
  if (sparse && cmax / (1.0 - (double)gam) >= 0.5 * (double)std::numeric_limits<float>::max())
    sparse = false;
  for (int e = 0; e < E && sparse; ++e)
    for (int a = 0; a < 9 && sparse; ++a)
      for (int i = 0; i < 9; ++i) {
        bool in = false;
        for (int j = 0; j < kSupN[a]; ++j) in |= kSup[a][j] == i;
        uint32_t bits;
        std::memcpy(&bits, &dh[(size_t)e * kRow + a * 10 + i], 4);
        if (!in && bits != 0) {
          sparse = false;
          break;
        }
      }
  for (int a = 0; a < 9 && sparse; ++a) {
    std::vector<std::vector<uint32_t>> pairs;
    for (int e = 0; e < E && sparse; ++e) {
      const float* src = &dh[(size_t)e * kRow];
      float q[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
      for (int j = 0; j < kSupN[a]; ++j) {
        r[j] = src[a * 10 + kSup[a][j]];
        q[j] = gam * r[j];
      }
      std::vector<uint32_t> key(9);
      std::memcpy(key.data(), q, 16);
      std::memcpy(&key[4], &src[a * 10 + 9], 4);
      std::memcpy(&key[5], r, 16);
      size_t k = 0;
      while (k < pairs.size() && pairs[k] != key) ++k;
      if (k == pairs.size()) {
        if ((int)k >= 16) {
          sparse = false;
          break;
        }
        pairs.push_back(key);
      }
    }
  }
  bool rfact = sparse;
  std::vector<std::vector<uint32_t>> lcls;
  for (int e = 0; e < E && rfact; ++e) {
    std::vector<uint32_t> key(16);
    std::memcpy(key.data(), &dh[(size_t)e * kRow + kL], 64);
    size_t k = 0;
    while (k < lcls.size() && lcls[k] != key) ++k;
    if (k == lcls.size()) {
      if ((int)k >= 32) {
        rfact = false;
        break;
      }
      lcls.push_back(key);
    }
  }
  p.sparse = sparse;
  p.rfact = rfact;
  return p;
}
// (the state: belief_sparse_ok alone; there was no flag for the values)
bool coded_active(const Props& p, const pp2::GateCtx& x) {
  return x.use_coded && x.entries > 0 && x.cpt == 4 && (!p.sparse || x.belief_ok);
}
bool loop_resident(const Props& p, const pp2::GateCtx& x) {
  return !x.sharded && x.resident && coded_active(p, x) && p.sparse && p.t_finite && p.tl_nonneg &&
         p.rfact && x.norm_block <= 32 - 2 && x.ncus > 0;
}
bool sweep_resident(const Props& p, const pp2::GateCtx& x) {
  return !(!x.resident || x.sharded || !coded_active(p, x) || !p.sparse || x.ncus <= 0);
}
bool sparse_rows(const Props& p, const pp2::GateCtx& x) { return coded_active(p, x) && p.sparse; }
}  // namespace before

int failures = 0, rows = 0;

// want_*: 1 yes, 0 no
void row(const char* name, const Dict& d, float gamma, pp2::GateCtx x, int want_loop,
         int want_sweep, int want_sparse) {
  ++rows;
  x.entries = (int)(d.size() / kRow);
  const pp2::DictProps p = pp2::dict_props(d.data(), x.entries, kRow, gamma);
  const int got[3] = {pp2::gate_loop_resident(p, x), pp2::gate_sweep_resident(p, x),
                      pp2::gate_sparse_rows(p, x)};
  const int want[3] = {want_loop, want_sweep, want_sparse};
  const before::Props q = before::scan(d, gamma);
  const int was[3] = {before::loop_resident(q, x), before::sweep_resident(q, x),
                      before::sparse_rows(q, x)};
  static const char* col[3] = {"loop", "sweep", "sparse"};
  for (int i = 0; i < 3; ++i) {
    if (got[i] != want[i]) {
      ++failures;
      std::printf("FAIL %s: %s resident/rows = %d, want %d\n", name, col[i], got[i], want[i]);
    }
    if (was[i] != want[i]) std::printf("before: %s / %s was %d, want %d\n", name, col[i], was[i], want[i]);
  }
  // a resident path never without the sparse rows, nor a masked pre-check
  // without the loop's model conditions
  if ((got[0] || got[1]) && !got[2]) {
    ++failures;
    std::printf("FAIL %s: resident without sparse rows\n", name);
  }
  if (pp2::gate_masked_precheck(p, true) && !(p.rfact() && p.tl_nonneg())) {
    ++failures;
    std::printf("FAIL %s: masked pre-check\n", name);
  }
}

float at_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

}  // namespace

int main() {
  const float g = 0.95f;
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const pp2::GateCtx x0;
  // on-support cells of the free entry: action 1's main weight, action 5's side
  const int t_main = 1 * 10 + 1, t_side = 5 * 10 + 2;

  row("generated-like", clean(), g, x0, 1, 1, 1);
  {
    pp2::GateCtx x = x0;
    x.norm_block = 1;
    row("generated-like, norm block 1", clean(), g, x, 1, 1, 1);
  }
  // T on the support: one condition for all three paths (the header's choice:
  // finite and >= +0, -0 refused)
  struct {
    const char* name;
    float v;
  } tcases[] = {{"T negative", -0.7f}, {"T -0", -0.0f}, {"T +inf", inf}, {"T NaN", nan},
                {"T -inf", -inf}, {"T negative NaN", at_bits(0xffc00000u)}};
  for (auto& t : tcases)
    for (int idx : {t_main, t_side}) {
      Dict d = clean();
      d[idx] = t.v;
      row((std::string("on-support ") + t.name + (idx == t_main ? " (main)" : " (side)")).c_str(),
          d, g, x0, 0, 0, 0);
    }
  // L concerns the belief alone: no resident loop; the sweeps and the sparse
  // rows stay (the state flag takes the belief off them once a step has run)
  for (float v : {-0.25f, -0.0f, inf, nan}) {
    Dict d = clean();
    d[3 * kRow + kL + 3] = v;
    char name[64];
    std::snprintf(name, sizeof name, "one L entry %g%s", (double)v, std::signbit(v) ? " (signed)" : "");
    row(name, d, g, x0, 0, 1, 1);
  }
  for (float v : {-0.0f, -2.5f, inf, nan, 3.0e38f}) {
    Dict d = clean();
    d[2 * kRow + 4 * 10 + 9] = v;
    char name[64];
    std::snprintf(name, sizeof name, "one C %g%s", (double)v, std::signbit(v) ? " (signed)" : "");
    row(name, d, g, x0, 0, 0, 0);
  }
  row("gamma 1.0", clean(), 1.0f, x0, 0, 0, 0);
  row("gamma < 0", clean(), -0.5f, x0, 0, 0, 0);
  row("gamma NaN", clean(), nan, x0, 0, 0, 0);
  {
    Dict d = clean();
    d[4 * 10 + 0] = 0.25f;  // the stay action's support is {4}
    row("off-support T 0.25", d, g, x0, 0, 0, 0);
    d[4 * 10 + 0] = -0.0f;
    row("off-support T -0 bits", d, g, x0, 0, 0, 0);
  }
  {
    Dict d16, d17;
    for (int k = 0; k < 17; ++k) {
      if (k < 16) add_entry(d16, 0);
      add_entry(d17, 0);
      if (k < 16) d16[(size_t)k * kRow + 2 * 10 + 9] = 1.0f + 0.125f * k;
      d17[(size_t)k * kRow + 2 * 10 + 9] = 1.0f + 0.125f * k;
    }
    row("16 (gT quad, C) pairs for action 2", d16, g, x0, 1, 1, 1);
    row("17 (gT quad, C) pairs for action 2", d17, g, x0, 0, 0, 0);
    // the same gT, another raw T: a class of its own (the belief gather's T)
    Dict dq;
    for (int k = 0; k < 17; ++k) {
      add_entry(dq, 0);
      dq[(size_t)k * kRow + 2 * 10 + 2] = 0.7f + 0.01f * k;
    }
    row("17 T quads for action 2", dq, g, x0, 0, 0, 0);
  }
  {
    Dict d32, d33;
    for (int k = 0; k < 33; ++k) {
      if (k < 32) add_entry(d32, 0, 0.01f * (k + 1));
      add_entry(d33, 0, 0.01f * (k + 1));
    }
    row("32 L vectors", d32, g, x0, 1, 1, 1);
    row("33 L vectors", d33, g, x0, 0, 1, 1);
  }
  {
    pp2::GateCtx x = x0;
    x.belief_ok = false;
    row("clean, belief flag false", clean(), g, x, 0, 0, 0);
    x = x0;
    x.values_ok = false;
    row("clean, values flag false", clean(), g, x, 0, 0, 0);
    // full rows drop no term: the coded kernels stay on whatever the state
    Dict d = clean();
    d[4 * 10 + 0] = 0.25f;
    const pp2::DictProps p = pp2::dict_props(d.data(), 4, kRow, g);
    x.belief_ok = false;
    x.entries = 4;
    if (!pp2::gate_coded_active(p, x) || pp2::gate_sparse_rows(p, x)) {
      ++failures;
      std::printf("FAIL full rows with both flags false: coded kernels on the full rows\n");
    }
  }
  // the switches
  {
    pp2::GateCtx x = x0;
    x.resident = false;
    row("TUNE_RESIDENT 0", clean(), g, x, 0, 0, 1);
    x = x0;
    x.use_coded = false;
    row("TUNE_CODED_MODEL 0", clean(), g, x, 0, 0, 0);
    x = x0;
    x.cpt = 2;
    row("2 cells per lane", clean(), g, x, 0, 0, 0);
    x = x0;
    x.norm_block = 31;
    row("norm block 31", clean(), g, x, 0, 1, 1);
    x.norm_block = 30;
    row("norm block 30", clean(), g, x, 1, 1, 1);
    x = x0;
    x.sharded = true;
    row("comm / group", clean(), g, x, 0, 0, 1);
    x = x0;
    x.ncus = 0;
    row("no CU count", clean(), g, x, 0, 0, 1);
  }
  row("no dictionary", Dict(), g, x0, 0, 0, 0);
  // the plane scan of an upload that got no dictionary
  {
    std::vector<float> p(1000, 0.5f);
    double m = -1.0;
    p[17] = 4.0f;
    bool ok = pp2::plane_finite_nonneg(p.data(), p.size(), &m) && m == 4.0;
    for (float v : {-0.0f, -1.0f, inf, nan, -inf}) {
      p[999] = v;
      ok = ok && !pp2::plane_finite_nonneg(p.data(), p.size(), &m);
    }
    ok = ok && pp2::plane_finite_nonneg(p.data(), 0, nullptr);
    ok = ok && pp2::gamma_bound_ok(0.95f, 5.0) && !pp2::gamma_bound_ok(1.0f, 0.0) &&
         !pp2::gamma_bound_ok(-0.0f - 0.5f, 0.0) && !pp2::gamma_bound_ok(0.95f, 3.0e38) &&
         !pp2::gamma_bound_ok(nan, 1.0);
    if (!ok) {
      ++failures;
      std::printf("FAIL plane scan / gamma bound\n");
    }
  }
  // the row-sum rule of the evaluators' TILES routes: every T row sums to at
  // most 1 + 2^-20 in fp64
  {
    auto bounded = [&](const char* name, const Dict& d, bool want) {
      ++rows;
      if (pp2::dict_rows_bounded(d.data(), (int)(d.size() / kRow), kRow) != want) {
        ++failures;
        std::printf("FAIL row sums, %s: want %d\n", name, (int)want);
      }
    };
    // the last entry's action-6 row (support {3, 4, 6, 7}) as {0.5, 0.5, x, 0}
    auto with_row = [&](float x) {
      Dict d = clean();
      float* r = &d[3 * kRow + 6 * 10];
      for (int i = 0; i < 9; ++i) r[i] = 0.0f;
      r[3] = 0.5f;
      r[4] = 0.5f;
      r[6] = x;
      return d;
    };
    bounded("generated-like", clean(), true);
    bounded("sum exactly 1", with_row(0.0f), true);
    bounded("sum exactly 1 + 2^-20", with_row(0x1p-20f), true);
    bounded("sum 1 + 2^-20 + 2^-43 (one fp64 step past the bound)", with_row(0x1p-20f + 0x1p-43f),
            false);
    bounded("sum 1 + 2^-19", with_row(0x1p-19f), false);
    bounded("a NaN entry", with_row(nan), false);
    bounded("an inf entry", with_row(inf), false);
    {
      Dict d = clean();  // sub-stochastic and all-zero rows
      for (int a = 0; a < 9; ++a)
        for (int i = 0; i < 9; ++i) {
          d[1 * kRow + a * 10 + i] *= 0.5f;
          d[2 * kRow + a * 10 + i] = 0.0f;
        }
      bounded("sub-stochastic and all-zero rows", d, true);
    }
    {
      Dict d = with_row(0x1p-19f);  // the first entry's first row instead of the last's
      Dict e = clean();
      for (int i = 0; i < 9; ++i) e[i] = d[3 * kRow + 6 * 10 + i];
      bounded("sum 1 + 2^-19 in the first row", e, false);
    }
    bounded("an empty dictionary", Dict(), true);
    ++rows;
    if (!pp2::dict_rows_bounded(nullptr, 0, kRow)) {
      ++failures;
      std::printf("FAIL row sums, no rows and no storage\n");
    }
  }
  std::printf("%d rows, %d failures\n", rows, failures);
  if (failures) return 1;
  std::printf("all rows hold\n");
  return 0;
}
