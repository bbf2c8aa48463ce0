// Time-channel importance distillation (TCD: Park, Kang, Han, ICCV 2021) on the feature-distillation site of libs/cil/cil.py:519-541.
//
// cur / prev stored NHWC (N, H, W, C), N = B * T frames with row n = b * T + t; A = the importance map (T, C) fp32, mean 1:
//   loss = 1 / (N C H W) * sum_{n,h,w,c} A[n mod T, c] * (cur - prev)^2           (A == 1: the MSE of bdv_kd_mse_fwd)
//   dcur = g * 2 / (N C H W) * A[n mod T, c] * (cur - prev)                        (A == 1: bdv_kd_mse_bwd bit for bit)
//   S[t, c] += scale^2 * sum_{b,h,w} grad[b * T + t, h, w, c]^2                     (the estimator's accumulator, grad fp32)
//
// Passes.  Forward: tc_sqdiff_partial_kernel reads cur and prev once each plus the cache-resident table and writes one partial per
// block; sum_finalize_kernel (reduce_pieces.h) sums them in fp64 in one wave.  Backward: tc_bwd_kernel, one streaming pass, the upstream scalar read
// from device memory.  Accumulator: tc_sqgrad_partial_kernel reads grad once and writes one (T, C) slab per row partition;
// tc_slab_sum_kernel adds the slabs in ascending order into S (squares and sums in fp64: S is rounded once).  A thread of the loss
// kernels stays at one unit index inside the frame and one segment at a time, so its table entry is a register; a 16-byte unit never
// straddles a frame or a segment (C % 4 == 0).
// Every output location is written by exactly one thread and every sum has a fixed order: no atomics, run-to-run bitwise equal.
//
// Limits: C % 4 == 0; N % T == 0; H * W * C / 4 and N / T * H * W at most 2^30.  Compiled with -ffp-contract=off: the backward's
// products must round as bdv_kd_mse_bwd's do.
#include "common.h"

namespace {

constexpr int TC_BLOCKS = 1024;      // forward partials at most, as bdv_kd_mse_fwd's (one fp64 finalize wave reads them)
constexpr int TC_ACC_BLOCKS = 2048;  // accumulator blocks at most (channel slabs x T x row partitions)
constexpr int TC_BWD_BLOCKS = 1 << 20;
constexpr int64_t TC_MAX_UNITS = (int64_t)1 << 30;   // 16-byte units of a frame, rows of a segment: index + grid stride stays below 2^31

// the grid of a pass over B clips of T frames of FU 16-byte units, at most `cap` blocks: x = 256-unit chunks of a frame, y = segments,
// z = clips (blocks are dealt x first, then y: with every segment in the grid consecutive blocks walk the tensor front to back).  A thread keeps its unit index i inside the frame (so i % C4, its channel group, is computed once), walks the
// segments t (one table entry A[t][i % C4] each, held in registers) and inside a segment the clips: the inner loop is loads and
// arithmetic only.  With the table entry fetched per unit the bf16 forward ran at 1.4-1.7x kd_mse's time (tools/bench_kd_importance.py).
inline dim3 tc_grid(int B, int T, int64_t FU, int cap) {
  int64_t gx = (FU + 255) / 256;
  if (gx > cap) gx = cap;
  int64_t gy = cap / gx;
  if (gy > B) gy = B;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  int64_t gz = cap / (gx * gy);
  if (gz > T) gz = T;
  if (gz > 65535) gz = 65535;
  if (gz < 1) gz = 1;
  return dim3((unsigned)gx, (unsigned)gz, (unsigned)gy);
}

template <int ES>
__global__ __launch_bounds__(256) void tc_sqdiff_partial_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                                 const float4* __restrict__ A, float* __restrict__ partial, int B, int T,
                                                                 int FU, int C4) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int i = blockIdx.x * 256 + tid; i < FU; i += gridDim.x * 256) {
    const int c4 = i % C4;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
      const float4 w = A[(int64_t)t * C4 + c4];
      for (int c = blockIdx.z; c < B; c += gridDim.z) {
        const int64_t u = ((int64_t)c * T + t) * FU + i;
        const float4 x = act_ld4<ES>(a, u), y = act_ld4<ES>(b, u);
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        s += (w.x * (d0 * d0) + w.y * (d1 * d1)) + (w.z * (d2 * d2) + w.w * (d3 * d3));
      }
    }
  }
  s = block_sum<SumOrder::Pairwise>(s, red);
  if (tid == 0) partial[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

template <int ES>
__global__ __launch_bounds__(256) void tc_bwd_kernel(const void* __restrict__ a, const void* __restrict__ b, const float4* __restrict__ A,
                                                      const float* __restrict__ gdev, float ghost, void* __restrict__ da, int B, int T,
                                                      int FU, int C4) {
  const float c = ghost * gdev[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < FU; i += gridDim.x * 256) {
    const int c4 = i % C4;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
      const float4 w = A[(int64_t)t * C4 + c4];
      const float k0 = c * w.x, k1 = c * w.y, k2 = c * w.z, k3 = c * w.w;
      for (int n = blockIdx.z; n < B; n += gridDim.z) {
        const int64_t u = ((int64_t)n * T + t) * FU + i;
        const float4 x = act_ld4<ES>(a, u), y = act_ld4<ES>(b, u);
        act_st4<ES>(da, u, make_float4(k0 * (x.x - y.x), k1 * (x.y - y.y), k2 * (x.z - y.z), k3 * (x.w - y.w)));
      }
    }
  }
}

// The accumulator's first stage.  grid (channel slabs, T, P): block = segment t, a slab of CGW channel groups, row partition p of the
// R = B * H * W rows of that segment.  thread = (row lane rl, channel group cgl); it adds its rows in ascending order, then the row
// lanes are added in ascending order through LDS and the block writes its slab entries of partial[p][t][:].  Squares and sums are
// fp64 (the pass is bound by the one read of grad: 8 fp64 operations per 16 bytes), so S carries one rounding, the last.
template <int CGW>
__global__ __launch_bounds__(256) void tc_sqgrad_partial_kernel(const float4* __restrict__ g, double* __restrict__ partial, int T,
                                                                 int HW, int R, int C4) {
  constexpr int RL = 256 / CGW;
  __shared__ double acc[4][256];
  const int tid = threadIdx.x, cgl = tid % CGW, rl = tid / CGW;
  const int cg = blockIdx.x * CGW + cgl, t = blockIdx.y, p = blockIdx.z, P = gridDim.z;
  const bool active = cg < C4;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (active) {
#pragma unroll 4
    for (int r = p * RL + rl; r < R; r += P * RL) {
      const int b = r / HW, hw = r - b * HW;
      const float4 v = g[(((int64_t)b * T + t) * HW + hw) * C4 + cg];
      s0 += (double)v.x * (double)v.x;
      s1 += (double)v.y * (double)v.y;
      s2 += (double)v.z * (double)v.z;
      s3 += (double)v.w * (double)v.w;
    }
  }
  acc[0][tid] = s0;
  acc[1][tid] = s1;
  acc[2][tid] = s2;
  acc[3][tid] = s3;
  __syncthreads();
  if (rl == 0 && active) {
    double* __restrict__ out = partial + (((int64_t)p * T + t) * C4 + cg) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double tot = acc[q][cgl];
#pragma unroll
      for (int k = 1; k < RL; ++k) tot += acc[q][k * CGW + cgl];
      out[q] = tot;
    }
  }
}

// S[i] = fp32(S[i] + scale^2 * (partial[0][i] + partial[1][i] + ...)), one thread per (t, c)
__global__ __launch_bounds__(256) void tc_slab_sum_kernel(const double* __restrict__ partial, float* __restrict__ S, int P, int TC,
                                                           double scale2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= TC) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += partial[(int64_t)p * TC + i];
  S[i] = (float)((double)S[i] + scale2 * s);
}

inline int tc_cgw(int C4) { return C4 >= 64 ? 64 : 16; }
// row partitions of the accumulator: as many as give every row lane a row, at most TC_ACC_BLOCKS blocks in all
inline int tc_parts(int N, int T, int C, int HW) {
  const int C4 = C / 4, cgw = tc_cgw(C4), slabs = (C4 + cgw - 1) / cgw, RL = 256 / cgw;
  const int64_t R = (int64_t)(N / T) * HW;
  int64_t P = (R + RL - 1) / RL;
  int64_t cap = TC_ACC_BLOCKS / ((int64_t)slabs * T);
  if (cap < 1) cap = 1;
  if (P > cap) P = cap;
  return (int)P;
}

inline bool tc_dims_ok(int N, int T, int C, int H, int W) { return N > 0 && T > 0 && C > 0 && H > 0 && W > 0; }

}  // namespace

#define TC_STREAM ((hipStream_t)stream)

extern "C" size_t bdv_kd_tc_workspace_bytes(int N, int T, int C, int H, int W) {
  if (!tc_dims_ok(N, T, C, H, W) || C % 4 != 0 || N % T != 0) return 0;
  const int64_t HW = (int64_t)H * W, FU = HW * (C / 4);
  if (FU > TC_MAX_UNITS || (int64_t)(N / T) * HW > TC_MAX_UNITS) return 0;
  const dim3 grid = tc_grid(N / T, T, FU, TC_BLOCKS);
  const size_t fwd = (size_t)grid.x * grid.y * grid.z * sizeof(float);
  const size_t acc = (size_t)tc_parts(N, T, C, (int)HW) * T * C * sizeof(double);
  return fwd > acc ? fwd : acc;
}

#define TC_REQUIRE_SHAPE(name)                                                                                          \
  do {                                                                                                                  \
    BDV_REQUIRE(C % 4 == 0, name ": C=%d is not a multiple of 4", C);                                                   \
    BDV_REQUIRE(N % T == 0, name ": N=%d frames is not a multiple of T=%d segments", N, T);                              \
    BDV_REQUIRE((int64_t)H * W * (C / 4) <= TC_MAX_UNITS && (int64_t)(N / T) * H * W <= TC_MAX_UNITS,                   \
                name ": H=%d W=%d C=%d N=%d: a frame or a segment's rows exceed 2^30", H, W, C, N);                      \
  } while (0)

extern "C" int bdv_kd_tc_fwd(const void* cur, const void* prev, const float* importance, float* loss, int N, int T, int C, int H, int W,
                             void* workspace, size_t workspace_bytes, int act_dtype, void* stream) {
  BDV_REQUIRE_ACT(act_dtype, "bdv_kd_tc_fwd");
  BDV_REQUIRE(cur && prev && importance && loss && workspace && tc_dims_ok(N, T, C, H, W), "bdv_kd_tc_fwd: bad argument");
  TC_REQUIRE_SHAPE("bdv_kd_tc_fwd");
  BDV_REQUIRE(bdv_aligned16(cur) && bdv_aligned16(prev) && bdv_aligned16(importance) && bdv_aligned16(workspace),
              "bdv_kd_tc_fwd: alignment");
  BDV_REQUIRE_WORKSPACE("bdv_kd_tc_fwd", workspace_bytes, bdv_kd_tc_workspace_bytes(N, T, C, H, W));
  const int C4 = C / 4, FU = H * W * C4;
  const dim3 grid = tc_grid(N / T, T, FU, TC_BLOCKS);
  const int nb = (int)(grid.x * grid.y * grid.z);
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((tc_sqdiff_partial_kernel<ES>), grid, dim3(256), 0, TC_STREAM, cur, prev,
                                                   (const float4*)importance, (float*)workspace, N / T, T, FU, C4));
  BDV_LAUNCH_CHECK("bdv_kd_tc_fwd(partial)");
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, TC_STREAM, (const float*)workspace, nb,
                     1.0 / ((double)N * (double)FU * 4.0), loss);
  BDV_LAUNCH_CHECK("bdv_kd_tc_fwd(finalize)");
  return BDV_OK;
}

extern "C" int bdv_kd_tc_bwd(const void* cur, const void* prev, const float* importance, const float* gscale_dev, void* dcur, int N,
                             int T, int C, int H, int W, int act_dtype, void* stream) {
  BDV_REQUIRE_ACT(act_dtype, "bdv_kd_tc_bwd");
  BDV_REQUIRE(cur && prev && importance && gscale_dev && dcur && tc_dims_ok(N, T, C, H, W), "bdv_kd_tc_bwd: bad argument");
  TC_REQUIRE_SHAPE("bdv_kd_tc_bwd");
  BDV_REQUIRE(bdv_aligned16(cur) && bdv_aligned16(prev) && bdv_aligned16(importance) && bdv_aligned16(dcur), "bdv_kd_tc_bwd: alignment");
  const int C4 = C / 4, FU = H * W * C4;
  const int64_t numel = (int64_t)N * FU * 4;
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((tc_bwd_kernel<ES>), tc_grid(N / T, T, FU, TC_BWD_BLOCKS), dim3(256), 0, TC_STREAM, cur, prev,
                                                   (const float4*)importance, gscale_dev, 2.f / (float)numel, dcur, N / T, T, FU, C4));
  BDV_LAUNCH_CHECK("bdv_kd_tc_bwd");
  return BDV_OK;
}

extern "C" int bdv_tc_sqgrad_accum(const float* grad, float* S, float scale, int N, int T, int C, int H, int W, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  BDV_REQUIRE(grad && S && workspace && tc_dims_ok(N, T, C, H, W), "bdv_tc_sqgrad_accum: bad argument");
  TC_REQUIRE_SHAPE("bdv_tc_sqgrad_accum");
  BDV_REQUIRE(bdv_aligned16(grad) && bdv_aligned16(S) && bdv_aligned16(workspace), "bdv_tc_sqgrad_accum: alignment");
  BDV_REQUIRE_WORKSPACE("bdv_tc_sqgrad_accum", workspace_bytes, bdv_kd_tc_workspace_bytes(N, T, C, H, W));
  const int C4 = C / 4, HW = H * W, R = N / T * HW, cgw = tc_cgw(C4), P = tc_parts(N, T, C, HW);
  BDV_REQUIRE(T <= 65535, "bdv_tc_sqgrad_accum: T=%d exceeds 65535 segments", T);
  const dim3 grid((C4 + cgw - 1) / cgw, T, P);
  if (cgw == 64)
    hipLaunchKernelGGL((tc_sqgrad_partial_kernel<64>), grid, dim3(256), 0, TC_STREAM, (const float4*)grad, (double*)workspace, T, HW, R, C4);
  else
    hipLaunchKernelGGL((tc_sqgrad_partial_kernel<16>), grid, dim3(256), 0, TC_STREAM, (const float4*)grad, (double*)workspace, T, HW, R, C4);
  BDV_LAUNCH_CHECK("bdv_tc_sqgrad_accum(partial)");
  const int TC = T * C;
  hipLaunchKernelGGL(tc_slab_sum_kernel, dim3((TC + 255) / 256), dim3(256), 0, TC_STREAM, (const double*)workspace, S, P, TC, (double)scale * (double)scale);
  BDV_LAUNCH_CHECK("bdv_tc_sqgrad_accum(sum)");
  return BDV_OK;
}
