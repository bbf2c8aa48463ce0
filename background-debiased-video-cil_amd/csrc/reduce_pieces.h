// The reductions of the step tail -- heads and losses (head_loss.hip), the distillation losses (pod_kd.hip, tc_kd.hip), the optimizer
// (optim.hip), the representation path (repr.hip) and the Grad-CAM sums (gradcam.hip) -- one definition each.  Included by common.h.
// No file-scope fp pragma: head_loss.hip, repr.hip and optim.hip are built with contraction on, pod_kd.hip, tc_kd.hip and gradcam.hip
// with contraction off, and every piece here takes its file's setting (only proxy_softmax has a product next to a sum, and only
// head_loss.hip uses it).
#pragma once
#include <hip/hip_runtime.h>

// ---- one wave (64 lanes): xor butterfly, every lane gets the result ------------------------------------------------------------
template <class T>
__device__ __forceinline__ T wave_sum(T v) {  // float, double, int
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) { return wave_sum(v); }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- the four waves of a 256-thread block ---------------------------------------------------------------------------------------
// The order in which the four wave totals are added is part of a kernel's result bits, so every call names it:
//   SumOrder::Sequential  ((w0 + w1) + w2) + w3   lsc_loss_kernel, softce_kernel, topk_acc_kernel, sqdiff_partial_kernel (head_loss.hip),
//                                                 multi_sqnorm_partial_kernel (optim.hip), the two render kernels of gradcam.hip
//   SumOrder::Pairwise    (w0 + w1) + (w2 + w3)   tc_sqdiff_partial_kernel (tc_kd.hip), repr_kernel, row_normalize_kernel, nme_kernel,
//                                                 herding_kernel (repr.hip)
// Three kernels keep their sum written out, because they were slower through the helper (profiles/tail_kernel_dedupe.txt):
// head_fwd_kernel (head_loss.hip, sequential), pod_profile_kernel and pod_frame_kernel (pod_kd.hip, pairwise).
// block_combine: v is the calling wave's value (lane 0's counts); block_sum: v is the thread's value.  Both hand EVERY thread the total
// and hold one __syncthreads() between the write of red and its reads.  REUSE = true puts another one first, for a red that an earlier
// call of the same kernel may still be reading; with the default the caller owns a red nobody has touched.
// block_combine's array form reduces NV values with that one barrier (red[NV][4]).
enum class SumOrder { Sequential, Pairwise };

template <SumOrder ORDER, class T>
__device__ __forceinline__ T sum4(const T* w) {
  if constexpr (ORDER == SumOrder::Sequential) return w[0] + w[1] + w[2] + w[3];
  else return (w[0] + w[1]) + (w[2] + w[3]);
}

template <SumOrder ORDER, bool REUSE = false, class T, int NV>
__device__ __forceinline__ void block_combine(T (&v)[NV], T (&red)[NV][4]) {
  if constexpr (REUSE) __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = sum4<ORDER>(red[i]);
}
template <SumOrder ORDER, bool REUSE = false, class T>
__device__ __forceinline__ T block_combine(T v, T (&red)[4]) {
  if constexpr (REUSE) __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return sum4<ORDER>(red);
}
template <SumOrder ORDER, bool REUSE = false, class T>
__device__ __forceinline__ T block_sum(T v, T (&red)[4]) {
  return block_combine<ORDER, REUSE>(wave_sum(v), red);
}

// ---- out[0] = (float)(sum_i (double)v[i] * scale): one wave, fp64, a fixed order, rounded once -----------------------------------
// Launched <<<1, 64>>> after a kernel that wrote n partial sums.  A template (T = the partials' type, deduced at the launch) so that
// only the files that launch it carry a copy; internal linkage, so each of them carries its own.
namespace {
template <class T>
__global__ void sum_finalize_kernel(const T* __restrict__ v, int n, double scale, float* __restrict__ out) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += (double)v[i];
  s = wave_sum_d(s);
  if (lane == 0) out[0] = (float)(s * scale);
}
}  // namespace

// ---- softmax statistics of one row, computed by one wave (every lane gets them) ---------------------------------------------------
__device__ __forceinline__ float wave_row_max(const float* __restrict__ row, int K, int lane) {
  float mx = -INFINITY;
  for (int k = lane; k < K; k += 64) mx = fmaxf(mx, row[k]);
  return wave_max(mx);
}
// mx = max_k row[k], es = sum_k expf(row[k] - mx)
__device__ __forceinline__ void wave_softmax_stats(const float* __restrict__ row, int K, int lane, float& mx, float& es) {
  mx = wave_row_max(row, K, lane);
  es = 0.f;
  for (int k = lane; k < K; k += 64) es += expf(row[k] - mx);
  es = wave_sum(es);
}

// The LSC head's softmax over the P proxies of one class, by one thread: mx = max_p c[p], den = sum_p e_p, num = sum_p e_p c[p],
// e_p = expf(c[p] - mx); the class similarity is num / den.
__device__ __forceinline__ void proxy_softmax(const float* __restrict__ c, int P, float& mx, float& den, float& num) {
  mx = c[0];
  for (int p = 1; p < P; ++p) mx = fmaxf(mx, c[p]);
  den = 0.f;
  num = 0.f;
  for (int p = 0; p < P; ++p) {
    const float e = expf(c[p] - mx);
    den += e;
    num += e * c[p];
  }
}

// ---- arg-max / arg-min with the first index winning a tie --------------------------------------------------------------------------
// BETTER(a, b): a beats b (ArgMax: a > b; an arg-min is the same with a < b).  A NaN beats nothing and is beaten by nothing, so a
// candidate that starts at (-inf, 0x7fffffff) comes back with that index when every value is NaN: the sentinel and what it means stay
// with the caller.  herding_kernel (repr.hip) keeps its cross-wave arg-min written out: it was slower through block_argbest.
struct ArgMax { __device__ bool operator()(float a, float b) const { return a > b; } };

template <class BETTER>
__device__ __forceinline__ void argbest_take(float& v, int& i, float ov, int oi) {
  if (BETTER()(ov, v) || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
// over the 64 lanes of a wave; every lane gets the winner
template <class BETTER>
__device__ __forceinline__ void wave_argbest(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argbest_take<BETTER>(v, i, ov, oi);
  }
}
// over the four waves of a block: (v, i) is the calling wave's winner (lane 0's counts); THREAD 0 ONLY gets the block's.  One
// __syncthreads() between the writes and thread 0's reads; bestv / besti must not be in use by an earlier call.
template <class BETTER>
__device__ __forceinline__ void block_argbest(float& v, int& i, float (&bestv)[4], int (&besti)[4]) {
  if ((threadIdx.x & 63) == 0) {
    bestv[threadIdx.x >> 6] = v;
    besti[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = bestv[0];
    i = besti[0];
    for (int w = 1; w < 4; ++w) argbest_take<BETTER>(v, i, bestv[w], besti[w]);
  }
}

// ---- four channels at a time -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4_add(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// pairwise: (x^2 + y^2) + (z^2 + w^2).  sqdiff_partial_kernel (head_loss.hip) adds its four squares left to right and keeps them written out.
__device__ __forceinline__ float f4_sq(const float4 a) { return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w); }
