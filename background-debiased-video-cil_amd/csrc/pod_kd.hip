// Pooled-output distillation (PODNet, Douillard et al., ECCV 2020) in place of the pixel-wise MSE of libs/cil/cil.py:519-541.
//
// pod_spatial, cur / prev stored NHWC (N, H, W, C), a = cur^2, b = prev^2:
//   p_n = concat(sum_w a[n,h,w,c] as (H, C), sum_h a[n,h,w,c] as (W, C)),  q_n likewise from b
//   loss = mean_n | p_n / max(|p_n|, 1e-12) - q_n / max(|q_n|, 1e-12) |
// pod_flat, (N, D): loss = mean_n (1 - cur.prev / sqrt((|cur|^2 + 1e-12)(|prev|^2 + 1e-12)))   (F.cosine_embedding_loss, target 1)
//
// Passes of pod_spatial.  Forward: pod_profile_kernel reads cur and prev once each (grid.z picks the tensor) and writes the two
// profiles (N, H+W, C) fp32 plus one squared-norm partial per (frame, channel slab); pod_frame_kernel (one block per frame, reads
// the profiles only) writes the frame's distance and the profile gradient G (N, H+W, C); sum_finalize_kernel (reduce_pieces.h) sums the N
// distances in a fixed order.  Backward: pod_spatial_bwd_kernel reads cur and G and writes dcur = g * 2 * cur * (G[n,h,c] + G[n,H+w,c]).
// Every output location is written by exactly one thread and every sum has a fixed order: no atomics, run-to-run bitwise equal.
//
// Limits: C % 4 == 0 (16-byte lanes along C); H <= 64 and W <= 64 (POD_MAX_HW).  The column sums of a thread live in registers,
// 4 lanes x 16 float4 accumulators per channel group = 64 columns.  Rows cost no registers; H carries the same cap because no
// larger map is tested.  N <= 65535 (grid.y).  Compiled with -ffp-contract=off: p*ip - q*iq must be 0 when cur == prev, which a
// fused multiply-add would break.
#include "common.h"

namespace {

constexpr float POD_EPS = 1e-12f;   // F.normalize eps and cosine_embedding_loss EPSILON
constexpr int POD_MAX_HW = 64;
constexpr int POD_CG = 16;          // channel groups (float4) per slab: 16 lanes x 16 B (fp32) along C
constexpr int POD_WL = 4;           // column lanes per wave; the 4 waves of a block split the rows

// grid (S, N, 2): block = frame n, channel slab s, tensor z (0 = cur, 1 = prev).  lane = (wl, cgl): cgl = channel group inside the
// slab, wl = column lane; thread (wave, wl, cgl) reads the pixels (h, w) with h = wave (mod 4), w = wl (mod 4).
// Row sums: per thread over its <= JW columns in ascending w, then 2 xor-shuffle levels over wl.  Column sums: per thread over its
// rows in ascending h, then wave 0 + wave 1 + wave 2 + wave 3 through LDS in that order.
template <int ES> struct PodRaw { typedef float4 T; };
template <> struct PodRaw<2> { typedef bdv_u32x2_t T; };
template <int ES>
__device__ __forceinline__ float4 pod_widen(const typename PodRaw<ES>::T r) {
  if constexpr (ES == 4) return r;
  else return bdv_widen_bf16x4(r.x, r.y);
}
// a thread's JW column positions of one row, as loaded (act_ld4's access without the widening); zeros off the map
template <int ES, int JW>
__device__ __forceinline__ void pod_load_row(const void* __restrict__ x, int64_t rowbase, int W, int C4, int cg, int wl, bool active,
                                             typename PodRaw<ES>::T (&r)[JW]) {
  typedef typename PodRaw<ES>::T T;
#pragma unroll
  for (int j = 0; j < JW; ++j) {
    const int w = wl + POD_WL * j;
    if (active && w < W) r[j] = reinterpret_cast<const T*>(x)[(rowbase + w) * C4 + cg];
    else if constexpr (ES == 4) r[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    else r[j] = (T){0u, 0u};
  }
}

template <int ES, int JW>
__global__ __launch_bounds__(256) void pod_profile_kernel(const void* __restrict__ cur, const void* __restrict__ prev,
                                                           float4* __restrict__ prof, float* __restrict__ nrm, int N, int H, int W,
                                                           int C4, int S) {
  __shared__ float4 cs[JW * POD_WL * POD_CG];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cgl = lane & (POD_CG - 1), wl = lane / POD_CG;
  const int s = blockIdx.x, n = blockIdx.y, z = blockIdx.z;
  const int cg = s * POD_CG + cgl;
  const bool active = cg < C4;
  const void* __restrict__ x = z ? prev : cur;
  float4* __restrict__ P = prof + ((int64_t)z * N + n) * (int64_t)(H + W) * C4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 col[JW];
#pragma unroll
  for (int j = 0; j < JW; ++j) col[j] = z4;
  float sq = 0.f;
  // bf16 storage: a row is kept as loaded (2 registers per 4 channels) and the next row's loads are issued between the sums and
  // the shuffles of the current one; measured on the layer-1 map of R50 (tools/bench_pod_kd.py) 471 -> 221 us for the forward.
  // fp32 storage loads inside the iteration: the staged form needs 256 registers there (one wave per SIMD), 518 -> 866 us.
  constexpr bool STAGED = ES == 2;
  typename PodRaw<ES>::T nxt[STAGED ? JW : 1];
  if constexpr (STAGED)
    if (wave < H) pod_load_row<ES, JW>(x, ((int64_t)n * H + wave) * W, W, C4, cg, wl, active, nxt);
  for (int h = wave; h < H; h += 4) {
    float4 v[JW];
    if constexpr (STAGED) {
#pragma unroll
      for (int j = 0; j < JW; ++j) v[j] = pod_widen<ES>(nxt[j]);
    } else {
      pod_load_row<ES, JW>(x, ((int64_t)n * H + h) * W, W, C4, cg, wl, active, v);
    }
    float4 row = z4;
#pragma unroll
    for (int j = 0; j < JW; ++j) {
      const float4 a = make_float4(v[j].x * v[j].x, v[j].y * v[j].y, v[j].z * v[j].z, v[j].w * v[j].w);
      row = f4_add(row, a);
      col[j] = f4_add(col[j], a);
    }
    if constexpr (STAGED)
      if (h + 4 < H) pod_load_row<ES, JW>(x, ((int64_t)n * H + h + 4) * W, W, C4, cg, wl, active, nxt);
#pragma unroll
    for (int o = POD_CG; o < 64; o <<= 1) {
      row.x += __shfl_xor(row.x, o, 64);
      row.y += __shfl_xor(row.y, o, 64);
      row.z += __shfl_xor(row.z, o, 64);
      row.w += __shfl_xor(row.w, o, 64);
    }
    if (active && wl == 0) {
      P[(int64_t)h * C4 + cg] = row;
      sq += f4_sq(row);
    }
  }
#pragma unroll
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int j = 0; j < JW; ++j) {
        const int w = wl + POD_WL * j;
        const int idx = w * POD_CG + cgl;
        if (wv == 0) {
          cs[idx] = col[j];
        } else if (wv < 3) {
          cs[idx] = f4_add(cs[idx], col[j]);
        } else {
          const float4 tot = f4_add(cs[idx], col[j]);
          if (active && w < W) {
            P[(int64_t)(H + w) * C4 + cg] = tot;
            sq += f4_sq(tot);
          }
        }
      }
    }
    if (wv < 3) __syncthreads();
  }
  // the block sum (SumOrder::Pairwise) stays written out here and in pod_frame_kernel: through block_sum the forward missed its
  // timing on the layer-3 and layer-4 maps (profiles/tail_kernel_dedupe.txt)
  sq = wave_sum(sq);
  if (lane == 0) red[wave] = sq;
  __syncthreads();
  if (tid == 0) nrm[((int64_t)z * N + n) * S + s] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One block per frame.  d = p^ - q^ is formed element by element (not from dot products: cur close to prev must not cancel);
// dist = |d|, u = d / dist (0 at dist = 0), G = (u - m p^ (p^.u)) / max(|p|, eps) / N with m = [|p| >= eps], the mask torch's
// clamp_min backward applies inside F.normalize.
__global__ __launch_bounds__(256) void pod_frame_kernel(const float4* __restrict__ prof, const float* __restrict__ nrm,
                                                         float4* __restrict__ G, float* __restrict__ dist, int N, int L4, int S,
                                                         float invN) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
  const float4* __restrict__ p = prof + (int64_t)n * L4;
  const float4* __restrict__ q = prof + ((int64_t)N + n) * L4;
  float4* __restrict__ g = G + (int64_t)n * L4;
  double sp = 0.0, sq = 0.0;
  for (int s = 0; s < S; ++s) {
    sp += (double)nrm[(int64_t)n * S + s];
    sq += (double)nrm[((int64_t)N + n) * S + s];
  }
  const float np = sqrtf((float)sp), nq = sqrtf((float)sq);
  const float ip = 1.f / fmaxf(np, POD_EPS), iq = 1.f / fmaxf(nq, POD_EPS);
  float dd = 0.f, pd = 0.f;
  for (int i = tid; i < L4; i += 256) {
    const float4 a = p[i], b = q[i];
    const float4 ph = make_float4(a.x * ip, a.y * ip, a.z * ip, a.w * ip);
    const float4 d = make_float4(ph.x - b.x * iq, ph.y - b.y * iq, ph.z - b.z * iq, ph.w - b.w * iq);
    dd += f4_sq(d);
    pd += (ph.x * d.x + ph.y * d.y) + (ph.z * d.z + ph.w * d.w);
  }
  dd = wave_sum(dd);
  pd = wave_sum(pd);
  if (lane == 0) {
    red[0][wave] = dd;
    red[1][wave] = pd;
  }
  __syncthreads();
  dd = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  pd = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  const float ds = sqrtf(dd);
  if (tid == 0) dist[n] = ds;
  const bool zero = !(ds > 0.f);
  const float k = zero ? 0.f : ip * invN / ds;
  const float t = (zero || np < POD_EPS) ? 0.f : pd;
  for (int i = tid; i < L4; i += 256) {
    const float4 a = p[i], b = q[i];
    const float4 ph = make_float4(a.x * ip, a.y * ip, a.z * ip, a.w * ip);
    const float4 d = make_float4(ph.x - b.x * iq, ph.y - b.y * iq, ph.z - b.z * iq, ph.w - b.w * iq);
    g[i] = zero ? make_float4(0.f, 0.f, 0.f, 0.f)
                : make_float4((d.x - ph.x * t) * k, (d.y - ph.y * t) * k, (d.z - ph.z * t) * k, (d.w - ph.w * t) * k);
  }
}

// grid N*H: block = one row (n, h) of W * C4 channel groups
template <int ES>
__global__ __launch_bounds__(256) void pod_spatial_bwd_kernel(const void* __restrict__ cur, const float4* __restrict__ G,
                                                               const float* __restrict__ gdev, void* __restrict__ dcur, int H, int W,
                                                               int C4) {
  const int r = blockIdx.x, n = r / H, h = r - n * H;
  const float c = 2.f * gdev[0];
  const float4* __restrict__ gh = G + ((int64_t)n * (H + W) + h) * C4;
  const float4* __restrict__ gw = G + ((int64_t)n * (H + W) + H) * C4;
  const int64_t base = (int64_t)r * W * C4;
  const int cnt = W * C4;
  for (int i = threadIdx.x; i < cnt; i += 256) {
    const int w = i / C4, cg = i - w * C4;
    const float4 x = act_ld4<ES>(cur, base + i);
    const float4 a = gh[cg], b = gw[(int64_t)w * C4 + cg];
    act_st4<ES>(dcur, base + i,
                make_float4(c * (x.x * (a.x + b.x)), c * (x.y * (a.y + b.y)), c * (x.z * (a.z + b.z)), c * (x.w * (a.w + b.w))));
  }
}

// one wave per row; dunit = d(loss)/d(cur) for an upstream gradient of 1, fp32
template <int ES>
__global__ __launch_bounds__(256) void pod_flat_kernel(const void* __restrict__ cur, const void* __restrict__ prev,
                                                        float* __restrict__ rowloss, float4* __restrict__ dunit, int N, int D4,
                                                        float invN) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int64_t base = (int64_t)row * D4;
  float dot = 0.f, cc = 0.f, pp = 0.f;
  for (int i = lane; i < D4; i += 64) {
    const float4 x = act_ld4<ES>(cur, base + i), y = act_ld4<ES>(prev, base + i);
    dot += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
    cc += f4_sq(x);
    pp += f4_sq(y);
  }
  dot = wave_sum(dot);
  cc = wave_sum(cc);
  pp = wave_sum(pp);
  const float mc = cc + POD_EPS, mp = pp + POD_EPS;
  const float den = sqrtf(mc * mp);
  if (lane == 0) rowloss[row] = 1.f - dot / den;
  const float k = -invN / den, r = dot / mc;
  for (int i = lane; i < D4; i += 64) {
    const float4 x = act_ld4<ES>(cur, base + i), y = act_ld4<ES>(prev, base + i);
    dunit[base + i] = make_float4(k * (y.x - x.x * r), k * (y.y - x.y * r), k * (y.z - x.z * r), k * (y.w - x.w * r));
  }
}

inline int pod_slabs(int C) { return (C / 4 + POD_CG - 1) / POD_CG; }

}  // namespace

#define PK_STREAM ((hipStream_t)stream)

extern "C" size_t bdv_pod_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return ((size_t)2 * N * (H + W) * C + (size_t)2 * N * pod_slabs(C) + (size_t)N) * sizeof(float);
}

// what bdv_pod_spatial_fwd and bdv_pod_spatial_bwd ask of N, C, H, W
#define POD_REQUIRE_SHAPE(name)                                                                                              \
  do {                                                                                                                       \
    BDV_REQUIRE(C % 4 == 0, name ": C=%d is not a multiple of 4", C);                                                        \
    BDV_REQUIRE(H <= POD_MAX_HW && W <= POD_MAX_HW, name ": H=%d W=%d exceeds the %d x %d limit", H, W, POD_MAX_HW, POD_MAX_HW); \
    BDV_REQUIRE(N <= 65535, name ": N=%d exceeds 65535 frames", N);                                                          \
  } while (0)

extern "C" int bdv_pod_spatial_fwd(const void* cur, const void* prev, float* loss, float* G, int N, int C, int H, int W,
                                   void* workspace, size_t workspace_bytes, int act_dtype, void* stream) {
  BDV_REQUIRE_ACT(act_dtype, "bdv_pod_spatial_fwd");
  BDV_REQUIRE(cur && prev && loss && G && workspace && N > 0 && C > 0 && H > 0 && W > 0, "bdv_pod_spatial_fwd: bad argument");
  POD_REQUIRE_SHAPE("bdv_pod_spatial_fwd");
  BDV_REQUIRE(bdv_aligned16(cur) && bdv_aligned16(prev) && bdv_aligned16(G) && bdv_aligned16(workspace),
              "bdv_pod_spatial_fwd: alignment");
  BDV_REQUIRE_WORKSPACE("bdv_pod_spatial_fwd", workspace_bytes, bdv_pod_workspace_bytes(N, C, H, W));
  const int C4 = C / 4, S = pod_slabs(C), L4 = (H + W) * C4;
  float4* prof = (float4*)workspace;
  float* nrm = (float*)workspace + (size_t)2 * N * (H + W) * C;
  float* dist = nrm + (size_t)2 * N * S;
  const dim3 grid(S, N, 2);
#define POD_PROFILE(JW)                                                                                                      \
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((pod_profile_kernel<ES, JW>), grid, dim3(256), 0, PK_STREAM, cur, prev, prof, \
                                                   nrm, N, H, W, C4, S))
  if (W <= 2 * POD_WL) POD_PROFILE(2);
  else if (W <= 4 * POD_WL) POD_PROFILE(4);
  else if (W <= 8 * POD_WL) POD_PROFILE(8);
  else POD_PROFILE(16);
#undef POD_PROFILE
  BDV_LAUNCH_CHECK("bdv_pod_spatial_fwd(profile)");
  hipLaunchKernelGGL(pod_frame_kernel, dim3(N), dim3(256), 0, PK_STREAM, (const float4*)prof, (const float*)nrm, (float4*)G, dist, N,
                     L4, S, 1.f / (float)N);
  BDV_LAUNCH_CHECK("bdv_pod_spatial_fwd(frame)");
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, PK_STREAM, (const float*)dist, N, 1.0 / (double)N, loss);
  BDV_LAUNCH_CHECK("bdv_pod_spatial_fwd(mean)");
  return BDV_OK;
}

extern "C" int bdv_pod_spatial_bwd(const void* cur, const float* G, const float* gscale_dev, void* dcur, int N, int C, int H, int W,
                                   int act_dtype, void* stream) {
  BDV_REQUIRE_ACT(act_dtype, "bdv_pod_spatial_bwd");
  BDV_REQUIRE(cur && G && gscale_dev && dcur && N > 0 && C > 0 && H > 0 && W > 0, "bdv_pod_spatial_bwd: bad argument");
  POD_REQUIRE_SHAPE("bdv_pod_spatial_bwd");
  BDV_REQUIRE(bdv_aligned16(cur) && bdv_aligned16(G) && bdv_aligned16(dcur), "bdv_pod_spatial_bwd: alignment");
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((pod_spatial_bwd_kernel<ES>), dim3(N * H), dim3(256), 0, PK_STREAM, cur,
                                                   (const float4*)G, gscale_dev, dcur, H, W, C / 4));
  BDV_LAUNCH_CHECK("bdv_pod_spatial_bwd");
  return BDV_OK;
}

extern "C" int bdv_pod_flat(const void* cur, const void* prev, float* loss, float* dcur_unit, int N, int D, void* workspace,
                            size_t workspace_bytes, int act_dtype, void* stream) {
  BDV_REQUIRE_ACT(act_dtype, "bdv_pod_flat");
  BDV_REQUIRE(cur && prev && loss && dcur_unit && workspace && N > 0 && D > 0, "bdv_pod_flat: bad argument");
  BDV_REQUIRE(D % 4 == 0, "bdv_pod_flat: D=%d is not a multiple of 4", D);
  BDV_REQUIRE(bdv_aligned16(cur) && bdv_aligned16(prev) && bdv_aligned16(dcur_unit), "bdv_pod_flat: alignment");
  BDV_REQUIRE_WORKSPACE("bdv_pod_flat", workspace_bytes, bdv_pod_workspace_bytes(N, D, 1, 1));
  float* rowloss = (float*)workspace;
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((pod_flat_kernel<ES>), dim3((N + 3) / 4), dim3(256), 0, PK_STREAM, cur, prev, rowloss,
                                                   (float4*)dcur_unit, N, D / 4, 1.f / (float)N));
  BDV_LAUNCH_CHECK("bdv_pod_flat(rows)");
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, PK_STREAM, (const float*)rowloss, N, 1.0 / (double)N, loss);
  BDV_LAUNCH_CHECK("bdv_pod_flat(mean)");
  return BDV_OK;
}
