/*
 * ref_driver.cpp -- runs the reference's own per-cell kernels on the host.
 * TEST INFRASTRUCTURE ONLY (see pp2_oracle.h).
 *
 * ref_build.py cuts the kernels' definitions out of the reference tree into
 * _ref/ref_mdp.inc and _ref/ref_pomdp.inc (never committed) and compiles this
 * file around them, once with -ffp-contract=fast (a*b+c contracted to fma,
 * like the reference's nvcc --use_fast_math build) and once with
 * -ffp-contract=off (the sensitivity control).  The MDP and POMDP sources
 * reuse names, so each set lives in a namespace of its own.
 *
 * Every entry point launches its kernel like the reference's host code does,
 * 8 x 8 blocks, but always with one block row and column more than the grid
 * needs, so the kernel's own bounds check runs at every size.  Layouts are the
 * oracle's (= the reference's): T[hw][9][9], L[hw][16], R/C[hw][9],
 * alphas [hw][9] (FIB) or [S][hw] (PBVI), idx = y*W + x.
 *
 * ftz != 0 sets x86 flush-to-zero and denormals-are-zero for the call (the
 * reference's device arithmetic flushes); MXCSR is saved and restored around
 * every call, so the caller's thread keeps its own floating-point mode.
 */
#include "ref_shim.h"

#include <vector>
#include <xmmintrin.h>

thread_local ref_uint3 threadIdx, blockIdx, blockDim, gridDim;

namespace ref_mdp {
#include "ref_mdp.inc"
}
namespace ref_pomdp {
#include "ref_pomdp.inc"
}

namespace {

struct MxcsrScope {
  unsigned saved;
  explicit MxcsrScope(int ftz) : saved(_mm_getcsr()) {
    const unsigned kFtz = 0x8000u, kDaz = 0x0040u;
    _mm_setcsr(ftz ? (saved | kFtz | kDaz) : (saved & ~(kFtz | kDaz)));
  }
  ~MxcsrScope() { _mm_setcsr(saved); }
};

/* one call of `cell` per thread of a 2-D launch that overhangs H x W */
template <class F>
void launch(int H, int W, F cell) {
  const unsigned kB = 8;
  blockDim = {kB, kB, 1};
  gridDim = {(unsigned)W / kB + 1, (unsigned)H / kB + 1, 1};
  for (unsigned by = 0; by < gridDim.y; ++by)
    for (unsigned bx = 0; bx < gridDim.x; ++bx)
      for (unsigned ty = 0; ty < kB; ++ty)
        for (unsigned tx = 0; tx < kB; ++tx) {
          blockIdx = {bx, by, 0};
          threadIdx = {tx, ty, 0};
          cell();
        }
}

template <class T>
T* mut(const T* p) { return const_cast<T*>(p); }

}  // namespace

extern "C" {

void ref_model_pomdp(int H, int W, const uint8_t* map, int gx, int gy, float* T, float* L,
                     float* R, int ftz) {
  MxcsrScope fp(ftz);
  launch(H, W, [&] { ref_pomdp::cudaGenerateModelData(H, W, gx, gy, map, T, L, R); });
}

void ref_model_mdp(int H, int W, const uint8_t* map, int gx, int gy, float* T, float* C,
                   int ftz) {
  MxcsrScope fp(ftz);
  launch(H, W, [&] { ref_mdp::cudaGenerateModelData(H, W, gx, gy, mut(map), T, C); });
}

void ref_mdp_sweep(int H, int W, float gamma, const float* T, const float* C, const float* J_in,
                   float* J_out, uint8_t* A, int ftz) {
  MxcsrScope fp(ftz);
  launch(H, W, [&] {
    ref_mdp::cudaOneStepValueIteration(H, W, gamma, mut(T), mut(C), mut(J_in), J_out, A);
  });
}

void ref_belief_update(int H, int W, const float* T, const float* L, const float* b_in, int u,
                       int z, float* b_out, int ftz) {
  MxcsrScope fp(ftz);
  launch(H, W, [&] {
    ref_pomdp::cudaBayesBeliefUpdate(H, W, T, L, b_in, (uint8_t)u, (uint8_t)z, b_out);
  });
}

void ref_fib_sweep(int H, int W, float gamma, const float* T, const float* L, const float* R,
                   const float* a_in, float* a_out, int ftz) {
  MxcsrScope fp(ftz);
  launch(H, W, [&] { ref_pomdp::cudaFIBValueIteration(H, W, gamma, T, L, R, a_in, a_out); });
}

/* One (a, o) of the PBVI backup: the kernel reads T[:, a, :] and L[:, o] as
 * planes of their own, which the reference's host code slices out the same
 * way before each launch. */
void ref_gamma_ao(int H, int W, float gamma, const float* T, const float* L, int a, int o, int S,
                  const float* alphas, float* out, int ftz) {
  const size_t n = (size_t)H * W;
  std::vector<float> ta(9 * n), lo(n);
  for (size_t i = 0; i < n; ++i) {
    memcpy(&ta[9 * i], T + 81 * i + 9 * a, 9 * sizeof(float));
    lo[i] = L[16 * i + o];
  }
  MxcsrScope fp(ftz);
  launch(H, W, [&] {
    ref_pomdp::cudaComputeGammaOA(H, W, (uint32_t)S, gamma, ta.data(), lo.data(), alphas, out);
  });
}

/* the calling thread's MXCSR, for the test that it is left as it was */
unsigned ref_mxcsr(void) { return _mm_getcsr(); }

}  // extern "C"
