// pp2_dict_props.h -- the scalar properties of a model dictionary and the
// path predicates built on them: which models and states may use the sparse
// LDS rows, the tile-resident loop and the tile-resident sweeps (DESIGN.md
// §2.1, §3.2).  Host code with no HIP call in it (tests/
// resident_gates_check.cpp runs it stand-alone); pp2_runtime.cpp calls it.
//
// One invariant carries all three paths: every belief and every value that a
// kernel reads is finite and >= +0 (sign bit clear).
//   * The sparse rows drop the T == +0 terms of the belief gather and of the
//     Bellman backup.  fmaf(+0, v, acc) == acc only for a finite v (+0 * inf
//     and +0 * NaN are NaN), and the dropped leading terms leave acc at the
//     dense chain's +0 only while no partial sum is -0.
//   * The resident kernels hand edge rows of b and J between tiles with the
//     slot's tag bit in bit 31 of every word: a negative word is read as its
//     absolute value, or never matches its tag and the wait times out.
//   * The masked form keeps blocked cells' b and J as +0 and multiplies them
//     by a finite weight.
// The model keeps the invariant when
//   values:  every T entry finite and >= +0, every C finite and >= +0,
//            0 <= gamma < 1, max C / (1 - gamma) < FLT_MAX / 2
//            (J starts at +0, never decreases below +0 and stays bounded);
//   beliefs: every T and L entry finite and >= +0.
// The gates below therefore use ONE condition on T -- finite and >= +0, on and
// off the support, -0 refused like a negative weight -- for the sparse rows,
// the resident sweeps and the resident loop alike (t_nonneg).  An L entry
// that breaks its condition concerns the belief alone: the dictionary stays
// sparse and the sweeps may stay resident, the loop may not.
//
// The invariant is a property of the STATE, not of the model in force: b and
// J outlive a model change.  The context therefore keeps two state flags
// (GateCtx::belief_ok, values_ok):
//   * belief_ok is set by pp2_belief_set (true iff every entry of the new
//     belief is finite and >= +0) and cleared by every belief update or loop
//     step that runs under a model failing the beliefs condition;
//   * values_ok is set by pp2_mdp_reset and cleared by every sweep or loop
//     step that runs under a model failing the values condition;
//   * a model whose dictionary could not be built (dict_n == 0) is judged by a
//     host scan of the uploaded planes; generated models meet both conditions.
// The planes' pad columns (x in [width, wp)) are part of the state too: the
// kernels compute a pad lane from its own stale word and the resident loop
// hands whole rows over, so pp2_belief_set zeroes the owned rows' pads (a NaN
// or -0 left by a non-finite or negative-mass belief) and pp2_mdp_reset the
// whole value planes.
// A cleared flag keeps the context on the dense kernels (coded_active is
// false on a sparse dictionary; full-row dictionaries drop no term and need
// neither flag) until the state is set again.  Uploading a clean model over a
// state produced under a bad one does NOT set the flags.
#pragma once
#include <stdint.h>

#include <array>
#include <cfloat>
#include <cstring>
#include <vector>

#include "pp2_masked.h"

namespace pp2 {

namespace props_detail {
// (pp2_internal.h: kFactK, kResLK, kDictL, kResidentRing; pp2_runtime.cpp
// asserts the agreement)
constexpr int kFactK = 16;
constexpr int kLK = 32;
constexpr int kL = 90;
constexpr int kRing = 32;
}  // namespace props_detail

// +0 <= v < +inf (sign bit clear, not inf or NaN)
inline bool finite_nonneg(float v) { return masked_detail::bits(v) < 0x7f800000u; }
inline bool finite_bits(float v) { return (masked_detail::bits(v) & 0x7f800000u) != 0x7f800000u; }

// finite_nonneg over a plane of the dense model; *vmax: its largest entry
inline bool plane_finite_nonneg(const float* p, size_t n, double* vmax) {
  uint32_t worst = 0u;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t b = masked_detail::bits(p[i]);
    worst = b > worst ? b : worst;  // (unsigned order == float order while all pass)
  }
  if (worst >= 0x7f800000u) return false;
  float m;
  std::memcpy(&m, &worst, 4);
  if (vmax) *vmax = (double)m;
  return true;
}

// 0 <= gamma < 1 and cmax / (1 - gamma) < FLT_MAX / 2: J stays finite
inline bool gamma_bound_ok(float gamma, double cmax) {
  return gamma >= 0.0f && gamma < 1.0f && !(cmax / (1.0 - (double)gamma) >= 0.5 * (double)FLT_MAX);
}

struct DictProps {
  bool t_finite = false;   // every T entry finite
  bool t_nonneg = false;   // every T entry finite and >= +0
  bool l_nonneg = false;   // every L entry finite and >= +0
  bool cost_ok = false;    // every C finite and >= +0, gamma and the bound as above
  bool off_zero = false;   // every T entry off its action's support is +0 (bits)
  bool fact_ok = false;    // <= kFactK distinct (gT quad, C, T quad) classes per action
  bool lcls_ok = false;    // <= kResLK distinct L vectors
  bool tl_nonneg() const { return t_nonneg && l_nonneg; }
  // the sparse (factored) rows; implies the values condition on the model
  bool sparse() const { return cost_ok && off_zero && t_nonneg && fact_ok; }
  // the resident class tables (QR, LT) on top of them
  bool rfact() const { return sparse() && lcls_ok; }
  bool values_model_ok() const { return t_nonneg && cost_ok; }
  bool belief_model_ok() const { return tl_nonneg(); }
};

// dict: E rows of dict_row floats, [a][T_a0 .. T_a8, C_a] at 10 * a, L[16] at kDictL
inline DictProps dict_props(const float* dict, int E, int dict_row, float gamma) {
  using namespace masked_detail;
  DictProps p;
  p.t_finite = p.t_nonneg = p.l_nonneg = p.off_zero = true;
  double cmax = 0.0;
  bool c_ok = true;
  for (int e = 0; e < E; ++e) {
    const float* d = dict + (size_t)e * dict_row;
    for (int a = 0; a < 9; ++a) {
      for (int i = 0; i < 9; ++i) {
        const float t = d[a * 10 + i];
        if (!finite_bits(t)) p.t_finite = false;
        if (!finite_nonneg(t)) p.t_nonneg = false;
        bool in = false;
        for (int j = 0; j < kN[a]; ++j) in |= kS[a][j] == i;
        if (!in && bits(t) != 0u) p.off_zero = false;
      }
      const float cv = d[a * 10 + 9];
      if (!finite_nonneg(cv)) c_ok = false;
      else if ((double)cv > cmax) cmax = (double)cv;
    }
    for (int z = 0; z < 16; ++z)
      if (!finite_nonneg(d[props_detail::kL + z])) p.l_nonneg = false;
  }
  p.cost_ok = c_ok && gamma_bound_ok(gamma, cmax);
  // classes per action, keyed as build_model_dict keys them: fl(gamma * T) on
  // the support, C_a, raw T on the support
  p.fact_ok = true;
  for (int a = 0; a < 9 && p.fact_ok; ++a) {
    std::vector<std::array<uint32_t, 9>> pairs;
    for (int e = 0; e < E && p.fact_ok; ++e) {
      const float* d = dict + (size_t)e * dict_row;
      std::array<uint32_t, 9> key{};
      for (int j = 0; j < kN[a]; ++j) {
        const float r = d[a * 10 + kS[a][j]];
        key[j] = bits(gamma * r);
        key[5 + j] = bits(r);
      }
      key[4] = bits(d[a * 10 + 9]);
      size_t k = 0;
      while (k < pairs.size() && pairs[k] != key) ++k;
      if (k == pairs.size()) {
        if ((int)k >= props_detail::kFactK) p.fact_ok = false;
        else pairs.push_back(key);
      }
    }
  }
  p.lcls_ok = true;
  {
    std::vector<std::array<uint32_t, 16>> lcls;
    for (int e = 0; e < E && p.lcls_ok; ++e) {
      std::array<uint32_t, 16> key;
      std::memcpy(key.data(), dict + (size_t)e * dict_row + props_detail::kL, 64);
      size_t k = 0;
      while (k < lcls.size() && lcls[k] != key) ++k;
      if (k == lcls.size()) {
        if ((int)k >= props_detail::kLK) p.lcls_ok = false;
        else lcls.push_back(key);
      }
    }
  }
  return p;
}

// Every T row of the dictionary sums to at most 1 + 2^-20 (the nine entries
// added in fp64 in index order; a NaN entry fails): the TILES routes of the
// policy evaluator and of the occupancy ask it of an uploaded model, so that P
// stays below 2 and N below 2 * horizon over the 65536 steps a call may ask
// for and every value they multiply by a dropped +0 is finite.  An empty
// dictionary has no row that breaks it.
inline bool dict_rows_bounded(const float* dict, int E, int dict_row) {
  for (int e = 0; e < E; ++e)
    for (int a = 0; a < 9; ++a) {
      double s = 0.0;
      for (int i = 0; i < 9; ++i) s += (double)dict[(size_t)e * dict_row + a * 10 + i];
      if (!(s <= 1.0 + 0x1p-20)) return false;
    }
  return true;
}

// The context's switches and state flags that the predicates read.
struct GateCtx {
  bool resident = true;     // PP2_TUNE_RESIDENT
  bool use_coded = true;    // PP2_TUNE_CODED_MODEL
  int cpt = 4;              // cells per lane
  int norm_block = 8;       // PP2_TUNE_NORM_BLOCK
  bool sharded = false;     // an RCCL communicator or a shard group
  int ncus = 1;             // CUs of the device
  int entries = 1;          // dictionary entries (0: no dictionary)
  bool belief_ok = true;    // the belief meets the invariant
  bool values_ok = true;    // the values meet the invariant
};

// the coded kernels run (else the dense ones); a sparse dictionary needs both
// state flags, full rows drop no term and need neither
inline bool gate_coded_active(const DictProps& p, const GateCtx& x) {
  return x.use_coded && x.entries > 0 && x.cpt == 4 &&
         (!p.sparse() || (x.belief_ok && x.values_ok));
}
// the coded kernels run on the sparse rows
inline bool gate_sparse_rows(const DictProps& p, const GateCtx& x) {
  return gate_coded_active(p, x) && p.sparse();
}
// the model and state conditions of the tile-resident loop (the shard runs
// add their own; an unsharded context also needs !sharded and a plan)
inline bool gate_resident_model(const DictProps& p, const GateCtx& x) {
  return x.resident && gate_sparse_rows(p, x) && p.t_finite && p.tl_nonneg() && p.rfact() &&
         x.norm_block <= props_detail::kRing - 2 && x.ncus > 0;
}
inline bool gate_loop_resident(const DictProps& p, const GateCtx& x) {
  return !x.sharded && gate_resident_model(p, x);
}
// the tile-resident sweeps (pp2_mdp_sweep(n >= 2), pp2_mdp_solve), before the
// plan lookup: J is finite and >= +0 and stays so -- sparse() holds the
// model's part (t_nonneg, cost_ok), gate_coded_active the state's
inline bool gate_sweep_resident(const DictProps& p, const GateCtx& x) {
  return x.resident && !x.sharded && gate_sparse_rows(p, x) && p.t_finite && p.t_nonneg &&
         x.ncus > 0;
}
// whether masked_admit is worth asking (whole, unsharded grid with a halo row)
inline bool gate_masked_precheck(const DictProps& p, bool whole_grid_with_halo) {
  return p.rfact() && p.tl_nonneg() && p.t_finite && whole_grid_with_halo;
}

}  // namespace pp2
