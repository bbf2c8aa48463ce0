// Pieces shared by the loader kernels.  Two groups:
//   clip front-ends   Normalize of a uint8 pixel and its parameters (pool_frontend.hip, ragged.hip, actor_cut_mix.hip)
//   unaligned runs    fp32 runs that start at any 4-byte phase of the 16-byte grid, and the batch permutation that names a run's
//                     source sample (blend.hip, fg_merge.hip)
// pool_frontend.hip is built with contraction on and the other four with -ffp-contract=off, so there is NO file-scope fp pragma here:
// it would reach the pooling kernels that follow the include.  normalize_u8, whose roundings are specified, switches contraction
// off at function scope.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- clip front-ends ---------------------------------------------------------------------------------------------------------------
// ClipNorm is the parameter struct of crop_normalize_ragged_kernel and of AcmArgs.  crop_normalize_kernel and bgmix_normalize_kernel
// (pool_frontend.hip) keep NormParams, and the two crop kernels keep their bodies written out: there is no shared crop body to look
// for (a shared one was measured slower, profiles/loader_kernel_dedupe.txt).  All of them normalise through normalize_u8.
struct ClipNorm {
  float mean[3], inv_std[3];
};

inline ClipNorm clip_norm(const float mean[3], const float inv_std[3]) {
  ClipNorm n;
  for (int c = 0; c < 3; ++c) {
    n.mean[c] = mean[c];
    n.inv_std[c] = inv_std[c];
  }
  return n;
}

// mmcv.imnormalize as the CPU restatement computes it: a subtraction and a product by the fp32 reciprocal, each rounded
__device__ __forceinline__ float normalize_u8(uint8_t v, float mean, float inv_std) {
#pragma clang fp contract(off)
  return ((float)v - mean) * inv_std;
}

// ---- unaligned fp32 runs -----------------------------------------------------------------------------------------------------------
// phase of p on the 16-byte grid, in floats
__device__ __forceinline__ int phase4(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// four floats from any 4-byte aligned address: one 16-byte, two 8-byte or four 4-byte loads, whichever the address allows
__device__ __forceinline__ float4 ld4_any(const float* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) return *reinterpret_cast<const float4*>(p);
  if ((a & 7) == 0) {
    const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}

// perm entries are validated by the caller before the upload; an entry outside [0, B) is treated as b itself here, so that no
// address outside the batch is ever formed
__device__ __forceinline__ int64_t source_of(const int64_t* __restrict__ perm, int b, int B) {
  const int64_t p = perm[b];
  return (p < 0 || p >= B) ? (int64_t)b : p;
}

}  // namespace
