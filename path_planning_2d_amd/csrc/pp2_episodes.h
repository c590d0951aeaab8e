// pp2_episodes.h -- private: batched closed-loop policy episodes
// (pp2_episodes.hip kernels, pp2_episodes.cpp C ABI; include/pp2.h "episodes").
//
// One 256-thread workgroup keeps one episode's belief in LDS (two planes,
// ping-pong, with zero halo rows and zero x pads) and runs the whole horizon in
// one launch: control, motion, observation, belief update, rescale.  The
// dynamic LDS of a workgroup, in floats from its start:
//   ct     CT of the factored sweep rows ([9][kFactK] x 4 floats, C_a at .x):
//          the step cost C[s][u]
//   rf     the class tables (QR raw T quads, LT L columns: kResTab floats),
//          then the LX bytes of the E entries
//   cls    [9][pad4(E)] bytes: 4 * (class of entry e for action u), the float
//          offset of its quad in QR / CT -- the IW records transposed, so that
//          a step's gathers index one dense E-byte table (a 16-B IW record
//          per entry puts every read on 16 of the 64 banks)
//   code   the code plane, uint16 [H + 2][ps] (off-grid cells and pads: 0)
//   red    reduction scratch (kEpRedFloats)
//   b[2]   the belief planes, fp32 [H + 2][ps] + 4
//   asum   the alpha instance only, K != 9: two buffers of per-wave sums,
//          [2][kEpAlphaChunk] quads (w0..w3 of a vector) -- on top of the
//          layout above, which is the MODE and QMDP instances' whole LDS
//   sums   the lookahead instance only, in asum's place: two buffers of
//          per-wave sums, [2][16 z x kLaK vectors] quads (w0..w3 of a pair),
//   ltt    ... then the L columns transposed, [kResLK classes][16 z]
// with ps = wp + 4: cell (y, x) of a plane sits at (y + 1) * ps + 4 + x, so
// x = -1 is the row's last left pad and x = wp the next row's first.
//
// Placement.  The above is the LDS placement (PP2_EPISODES_LDS), which admits
// the grids whose planes fit kDictLdsMaxBytes.  The global placement
// (PP2_EPISODES_GLOBAL; k_episodes<POLICY, true>, all four policies) keeps the
// tables, red and asum (the lookahead: sums and ltt in its place) in LDS --
// ct | rf | cls | red | asum, episode_lds_global -- and the planes in one
// device allocation of the batch (the scratch):
//   planes  [workgroups][2] belief planes of ep_plane_stride floats, the LDS
//           planes' own indexing; zeroed once when allocated: a step writes the
//           interior quads only, so halo rows and x pads stay zero
//   b0img   the padded image of b0, same indexing, built per run
//           (k_episode_pad): step 0 of every episode reads it in place of a
//           per-episode copy, and an episode without a step stores it
//   code    the padded uint16 code plane, built per run, read by all
// Workgroups of a global launch = min(episodes, CUs x per-CU count,
// kEpScratchCapBytes / bytes of a workgroup's two planes), at least 1; the
// per-CU count is what the instance's registers admit, at most kEpMaxPerCu.  A
// workgroup is one wave per SIMD, and the three global instances take 121
// (MODE), 127 (QMDP) and 118 (alpha) VGPRs, which is 4 waves per SIMD
// (512 / 128): kEpGlobalPerCu = 4.  More workgroups than that would only queue
// behind the resident ones and widen the scratch.  The global lookahead
// instance takes 225 VGPRs, 2 waves per SIMD: kEpGlobalLookaheadPerCu = 2, and
// its launch is min(episodes, workgroups the scratch holds, CUs x 2) workgroups
// on the first plane pairs of the same scratch (the b0 image and the code plane
// stay behind all of the scratch's pairs, wherever they were first placed).
//
// The world and resumed segments (k_episodes<POLICY, GLOBAL, true>, the EXT
// instances: a run with a world attached, or pp2_episodes_resume).  A plain run
// launches the eight instances above, unchanged.  The EXT instances grow no LDS
// layout -- the world's code plane, class bytes, costs, T quads, LX bytes and L
// columns are loads at wave-uniform indices from the world context's own
// device tables, about two dozen words a step -- and stay inside the same
// register budgets, with no private segment, so they share the per-CU
// constants below:
//   VGPRs        MODE  QMDP  alpha  lookahead
//   LDS          117   123   118    220        (plain)
//   LDS, EXT     112   108   118    220
//   global       121   127   118    225        (plain)
//   global, EXT  120   114   120    229
// A resumed episode continues from the batch's per-episode arrays: steps,
// status, cost, final cell, the stored belief [H][wp] and the discount d
// (EpisodeRun::disc, stored by every EXT launch; after a plain launch, which
// stores none, launch_episode_discounts makes it from the steps).
#pragma once
#include "pp2_internal.h"

namespace pp2 {

constexpr int kEpThreads = 256;
constexpr int kEpRedFloats = 48;
constexpr int kEpMaxPerCu = 8;  // workgroups per CU the grid is sized for
// global placement: workgroups per CU by the instances' VGPRs (see above), and
// the cap on the scratch that holds every workgroup's two planes
constexpr int kEpGlobalPerCu = 4;
// ... of the global lookahead instance k_episodes<3, true>: 225 VGPRs, no
// private scratch, 2 waves per SIMD (the LDS instance: 220, also 2)
constexpr int kEpGlobalLookaheadPerCu = 2;
constexpr long long kEpScratchCapBytes = 1LL << 30;
// The alpha-vector policy (k_episodes<2>): K vectors in blocks of
// kEpAlphaBlock accumulators, their per-wave sums staged per chunk of
// kEpAlphaChunk vectors (one barrier per chunk, two buffers).  K = 9 (FIB)
// takes the QMDP control phase's shape and no scratch.
constexpr int kEpAlphaBlock = 8;
constexpr int kEpAlphaChunk = 64;
constexpr int kEpAlphaMax = 4096;  // PBVI's own limit
inline __host__ __device__ int ep_alpha_floats(int K) { return K == 9 ? 0 : 2 * kEpAlphaChunk * 4; }

// The one-step lookahead policy (k_episodes<3>): per action, blocks of
// kLaZ x kLaK (observation, vector) accumulators, their per-wave sums staged
// per block (one barrier per block, two buffers).
constexpr int kLaZ = 16;
constexpr int kLaK = 4;
constexpr int kLaSums = kLaZ * kLaK * 4;  // floats of one buffer
inline __host__ __device__ int ep_lookahead_floats() { return 2 * kLaSums + kLaZ * kResLK; }

struct EpisodeLds {
  int ps, prows;                         // plane row stride (floats), plane rows
  int epad;                              // bytes per action of cls
  int ct, rf, cls, code, red, b0, b1;    // offsets in floats
  int total;                             // floats
};
constexpr int kEpCtFloats = 9 * kFactK * 4;
__host__ __device__ inline int ep_pad4(int n) { return (n + 3) & ~3; }
// floats of the tables in front of the code plane
__host__ __device__ inline int ep_table_floats(int E) {
  return kEpCtFloats + ep_pad4(kResTab + ((E + 3) >> 2)) + ep_pad4(9 * (ep_pad4(E) >> 2));
}
__host__ __device__ inline EpisodeLds episode_lds(const Geom& g, int E) {
  EpisodeLds l;
  l.ps = g.wp + 4;
  l.prows = g.rows + 2;
  l.epad = ep_pad4(E);
  const int plane = l.prows * l.ps + 4;
  const int codef = ep_pad4((l.prows * l.ps + 8) >> 1);
  l.ct = 0;
  l.rf = l.ct + kEpCtFloats;
  l.cls = l.rf + ep_pad4(kResTab + ((E + 3) >> 2));
  l.code = ep_table_floats(E);
  l.red = l.code + codef;
  l.b0 = l.red + kEpRedFloats;
  l.b1 = l.b0 + plane;
  l.total = l.b1 + plane;
  return l;
}
// The global placement's LDS: the tables and red (code, b0, b1 unused).
__host__ __device__ inline EpisodeLds episode_lds_global(const Geom& g, int E) {
  EpisodeLds l;
  l.ps = g.wp + 4;
  l.prows = g.rows + 2;
  l.epad = ep_pad4(E);
  l.ct = 0;
  l.rf = l.ct + kEpCtFloats;
  l.cls = l.rf + ep_pad4(kResTab + ((E + 3) >> 2));
  l.code = l.b0 = l.b1 = 0;
  l.red = ep_table_floats(E);
  l.total = l.red + kEpRedFloats;
  return l;
}
// ... its bytes (alpha_floats: ep_alpha_floats(K) of an alpha run,
// ep_lookahead_floats() of a lookahead run, else 0)
inline long long episode_global_lds_bytes(int E, int alpha_floats) {
  return 4LL * (ep_table_floats(E) + kEpRedFloats + alpha_floats);
}
// floats from one global plane to the next (a multiple of 64: 256-byte
// aligned planes), and uint16 of the padded code plane
inline long long ep_plane_stride(const Geom& g) {
  const long long plane = ((long long)g.rows + 2) * (g.wp + 4) + 4;
  return (plane + 63) & ~63LL;
}
inline long long ep_code_elems(const Geom& g) {
  return (((long long)g.rows + 2) * (g.wp + 4) + 8 + 7) & ~7LL;
}
// LDS bytes of one workgroup; a batch is admitted only if this is at most
// kDictLdsMaxBytes (64-bit: the planes of a large grid overflow int floats).
inline long long episode_lds_bytes(const Geom& g, int E) {
  const long long ps = g.wp + 4, prows = (long long)g.rows + 2;
  const long long plane = prows * ps + 4;
  const long long codef = (((prows * ps + 8) >> 1) + 3) & ~3LL;
  return 4 * (ep_table_floats(E) + codef + kEpRedFloats + 2 * plane);
}

// ... of the alpha instance with K vectors
inline long long episode_alpha_lds_bytes(const Geom& g, int E, int K) {
  return episode_lds_bytes(g, E) + 4LL * ep_alpha_floats(K);
}

// ... of the lookahead instance
inline long long episode_lookahead_lds_bytes(const Geom& g, int E) {
  return episode_lds_bytes(g, E) + 4LL * ep_lookahead_floats();
}

struct EpisodeRun {
  Geom g;
  int E;                     // dictionary entries
  const uint16_t* code;      // code plane (row 0, x 0)
  const float* rows;         // factored sweep rows
  const float* rfact;        // class tables, then the LX bytes
  const float* Q;            // [9][H][wp], pads +0
  const uint8_t* A;          // [H][wp]
  const float* alpha;        // alpha runs: [K][H][wp], pads +0
  const uint8_t* alpha_act;  // [K], every one <= 8
  int K;
  const float* b0;           // [H][wp], pads +0
  const int32_t* start;      // [episodes], y * W + x
  int episodes, horizon;
  unsigned long long seed;
  float gamma;
  int goal;                  // y * W + x
  int32_t* steps;            // [episodes]
  uint8_t* status;
  float* cost;
  int32_t* final_cell;
  float* beliefs;            // [episodes][H][wp]
  // trace, [horizon][episodes] (null: not recorded)
  uint8_t* tr_u;
  uint8_t* tr_z;
  int32_t* tr_cell;
  float* tr_q;               // [horizon][episodes][9]
  int32_t* tr_mode;
  int32_t* tr_best;          // alpha runs: the winning vector and its sum
  float* tr_bsum;
  // lookahead runs: the POMDP reward planes [9][H][wp], pads +0, and the trace
  const float* rplanes;
  float* tr_rew;             // [horizon][episodes][9]
  float* tr_lmax;            // [horizon][episodes][9][16]
  int32_t* tr_lidx;
  // global placement: workgroup w's planes at gplanes + w * 2 * gstride, the
  // padded b0 image and the padded code plane (null in an LDS launch)
  float* gplanes;
  long long gstride;         // floats of a plane (ep_plane_stride)
  const float* gb0;
  const uint16_t* gcode;
  // EXT launches only (a plain launch leaves all of these null / 0).
  // The world (null: the batch context's model is the world too): its code
  // plane (row 0, x 0, the geometry's row stride), factored sweep rows and
  // class tables in device memory, read in place; goal above is then the
  // world's goal cell, -1 if it lies off the grid.
  const uint16_t* w_code;
  const float* w_rows;
  const float* w_rfact;
  // resume != 0: continue every episode from steps / status / cost /
  // final_cell / disc / beliefs instead of start and b0
  int resume;
  float* disc;               // [episodes] the discount d, stored by every EXT launch
};

// Q[u][y][x] = k_mdp_sweep's cost of action u from J (sparse coded model).
hipError_t launch_episode_qplanes(hipStream_t st, const Geom& g, const uint16_t* code,
                                  const float* rows, int E, const float* J, float* Q, int ncus);
// Alpha planes [K][H][wp], pads +0, from the FIB planes (fib: row stride
// fib.rs, plane stride fib.ps; K = 9) or from PBVI's flat rows (rows: [K][ld],
// cell y * W + x); act_out[k] = acts[k], or k without acts (FIB); act_out may
// be null (the reward planes of a lookahead run: fib = the R plane set).
hipError_t launch_episode_alpha_planes(hipStream_t st, const Geom& g, const PlaneSet* fib,
                                       const float* rows, int ld, int K, float* out,
                                       const uint8_t* acts, uint8_t* act_out);
// policy: PP2_CONTROL_MODE (0), PP2_CONTROL_QMDP (1), 2, the alpha-vector
// policy over a.alpha, or 3, the one-step lookahead over a.alpha and
// a.rplanes.  hipErrorInvalidValue when the workgroup's LDS does not fit.
// global: the global-placement instance (a.gplanes, a.gb0 and a.gcode set,
// built by launch_episode_pad on the same stream; workgroups at most the
// plane pairs a.gplanes holds).
// ext: the EXT instance of the same policy and placement -- a world (a.w_*)
// and / or a resumed segment (a.resume), a.disc set; without it both must be
// absent, and the launch is the plain instance's.
hipError_t launch_episodes(hipStream_t st, const EpisodeRun& a, int policy, int workgroups,
                           bool global = false, bool ext = false);
// disc[e] = the discount after steps[e] steps (d = 1, then d = fl(d * gamma)
// per step): what an EXT launch stores, made up after a plain run.
hipError_t launch_episode_discounts(hipStream_t st, const int32_t* steps, float gamma,
                                    int episodes, float* disc);
// The padded images of a global launch: gcode[(y + 1) * ps + 4 + x] = code of
// cell (y, x), gb0 likewise from b0 [H][wp]; everything off the grid 0.
hipError_t launch_episode_pad(hipStream_t st, const Geom& g, const uint16_t* code,
                              const float* b0, uint16_t* gcode, float* gb0);

}  // namespace pp2
