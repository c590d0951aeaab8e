/*
 * ref_shim.h -- the few CUDA words the reference's per-cell kernels use, for a
 * host build.  TEST INFRASTRUCTURE ONLY (see pp2_oracle.h).
 *
 * The kernels named in ref_build.py use no shared memory, barriers, atomics,
 * cuRAND or cuBLAS: __global__ / __device__ vanish, and the launch indices
 * are thread-local variables that ref_driver.cpp sets before each call, one
 * call per thread of the launch.  The components are unsigned like CUDA's
 * uint3 / dim3, so the kernels' index arithmetic converts as it does there.
 */
#ifndef PP2_REF_SHIM_H
#define PP2_REF_SHIM_H

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define __global__
#define __device__
#define __host__

struct ref_uint3 {
  unsigned x, y, z;
};

extern thread_local ref_uint3 threadIdx, blockIdx, blockDim, gridDim;

#endif
