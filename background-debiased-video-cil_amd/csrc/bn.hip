// BatchNorm2d (train / eval) on NHWC [M][C] fp32, fused with ReLU and the residual add, plus the
// backward.  HBM-bound column reductions: partial sums per row-block (fp32), fixed-order final
// reduction in fp64 (deterministic, no atomics).
//
// Replaces UPSTREAM mmaction ConvModule.bn / .activate and the Bottleneck/BasicBlock
// `out + identity -> relu`.
#include "common.h"

namespace {

constexpr int MAX_RB_TIMES_C = 524288;  // partial-slab capacity in floats per quantity

struct BnGrid {
  int CVB;  // float4 column vectors per block
  int RL;   // row lanes per block (CVB * RL == 256)
  int CC;   // column chunks
  int RB;   // row blocks
  int rows_per_block;
};

BnGrid bn_grid(int64_t M, int C) {
  BnGrid b;
  const int cv = C / 4;
  b.CVB = cv < 64 ? cv : 64;
  b.RL = 256 / b.CVB;
  b.CC = (cv + b.CVB - 1) / b.CVB;
  int64_t rb = (M + 127) / 128;
  const int64_t cap = 2048 / b.CC > 0 ? 2048 / b.CC : 1;
  if (rb > cap) rb = cap;
  if (rb < 1) rb = 1;
  while (rb * C > MAX_RB_TIMES_C) --rb;
  b.RB = (int)rb;
  b.rows_per_block = (int)((M + rb - 1) / rb);
  return b;
}

bool bn_c_ok(int C) { return C >= 64 && (C % 256 == 0 || C == 64 || C == 128); }

// ---- float4 arithmetic: every kernel below forms its sums and gradients with these, so one edit here changes them all ------------
__device__ __forceinline__ void add4(float4& s, const float4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
// s += a * b
__device__ __forceinline__ void acc_mul4(float4& s, const float4 a, const float4 b) {
  s.x += a.x * b.x; s.y += a.y * b.y; s.z += a.z * b.z; s.w += a.w * b.w;
}
// The BatchNorm arithmetic, per element: the normalised value xhat, and the gradient of the train-mode BatchNorm with a, b, c =
// coef[0..2] (bn_bwd_finalize_tail).  The float4 forms below go through these component by component, each component's chain
// complete before the next starts (the order the kernels were compiled from before they shared this text).
__device__ __forceinline__ float bn_xhat(float v, float mu, float is) { return (v - mu) * is; }
__device__ __forceinline__ float bn_dx(float a, float b, float c, float g, float v, float mu, float is) {
  return a * (g - b - bn_xhat(v, mu, is) * c);
}
__device__ __forceinline__ float4 bn_xhat4(const float4 v, const float4 mu, const float4 is) {
  return make_float4(bn_xhat(v.x, mu.x, is.x), bn_xhat(v.y, mu.y, is.y), bn_xhat(v.z, mu.z, is.z), bn_xhat(v.w, mu.w, is.w));
}
// s += g * xhat: the second sum of every backward statistics pass
__device__ __forceinline__ void acc_g_xhat4(float4& s, const float4 g, const float4 v, const float4 mu, const float4 is) {
  s.x += g.x * bn_xhat(v.x, mu.x, is.x);
  s.y += g.y * bn_xhat(v.y, mu.y, is.y);
  s.z += g.z * bn_xhat(v.z, mu.z, is.z);
  s.w += g.w * bn_xhat(v.w, mu.w, is.w);
}
__device__ __forceinline__ float4 bn_dx4(const float4 a, const float4 b, const float4 c, const float4 g, const float4 v, const float4 mu,
                                         const float4 is) {
  float4 d;
  d.x = bn_dx(a.x, b.x, c.x, g.x, v.x, mu.x, is.x);
  d.y = bn_dx(a.y, b.y, c.y, g.y, v.y, mu.y, is.y);
  d.z = bn_dx(a.z, b.z, c.z, g.z, v.z, mu.z, is.z);
  d.w = bn_dx(a.w, b.w, c.w, g.w, v.w, mu.w, is.w);
  return d;
}

// ---- row blocks: the decomposition of the column reductions over [M][C] ----------------------------------------------------------
// Block (x, y) of grid (RB, CC) owns rows [r0, r1) of the CVB float4 columns from y * CVB; thread tid is row lane rl = tid / CVB of
// column cv = tid % CVB and walks rows r0 + rl, r0 + rl + RL, ...  (bn_grid: CVB * RL == 256)
struct RowBlock {
  int cv, rl, c4, CV;   // column in the block, row lane, float4 column index in the tensor, float4 columns of the tensor
  int64_t r0, r1;
  __device__ __forceinline__ RowBlock(int64_t M, int C, int CVB, int rows_per_block) {
    const int tid = threadIdx.x;
    cv = tid % CVB;
    rl = tid / CVB;
    c4 = blockIdx.y * CVB + cv;
    r0 = (int64_t)blockIdx.x * rows_per_block;
    r1 = r0 + rows_per_block;
    if (r1 > M) r1 = M;
    CV = C / 4;
  }
};
// The N sums of a block's row lanes -> row blockIdx.x of the N partial slabs [RB][CV]: row lane 0 of each column adds lanes
// 1 .. RL - 1 in lane order and stores.  (blockIdx.x is read behind the barrier, where the kernels read it before they shared this
// text: read at the top, the compiler forms the LDS addresses of the loop another way.)
template <int N>
__device__ __forceinline__ void rowblock_colsum_store(float4 (&s)[N], const RowBlock& rb, int CVB, int RL, float* const (&slab)[N]) {
  static_assert(N == 2 || N == 3, "two or three sums");
  __shared__ float4 sh[N][256];
  const int tid = threadIdx.x;
  sh[0][tid] = s[0];
  sh[1][tid] = s[1];
  if constexpr (N == 3) sh[2][tid] = s[2];
  __syncthreads();
  if (rb.rl == 0) {
    for (int k = 1; k < RL; ++k) {   // N is 2 or 3, written out: with loops over n in here the compiler unrolls the k loop another way
      const float4 a = sh[0][k * CVB + rb.cv], b = sh[1][k * CVB + rb.cv];
      float4 e;
      if constexpr (N == 3) e = sh[2][k * CVB + rb.cv];
      add4(s[0], a);
      add4(s[1], b);
      if constexpr (N == 3) add4(s[2], e);
    }
    // The stores keep the two forms the kernels had: the offset expression per store for two sums, one named
    // offset for three.  Either form for both N changes the code of the kernels that had the other.
    if constexpr (N == 2) {
      reinterpret_cast<float4*>(slab[0])[(int64_t)blockIdx.x * rb.CV + rb.c4] = s[0];
      reinterpret_cast<float4*>(slab[1])[(int64_t)blockIdx.x * rb.CV + rb.c4] = s[1];
    } else {
      const int64_t o = (int64_t)blockIdx.x * rb.CV + rb.c4;
      reinterpret_cast<float4*>(slab[0])[o] = s[0];
      reinterpret_cast<float4*>(slab[1])[o] = s[1];
      reinterpret_cast<float4*>(slab[2])[o] = s[2];
    }
  }
}

// ---- forward statistics ------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ y, float* __restrict__ psum,
                                                          float* __restrict__ psq, int64_t M, int C, int CVB, int RL,
                                                          int rows_per_block) {
  const RowBlock rb(M, C, CVB, rows_per_block);
  float4 s[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};   // sum y, sum y^2
  const float4* yp = reinterpret_cast<const float4*>(y);
  for (int64_t r = rb.r0 + rb.rl; r < rb.r1; r += RL) {
    const float4 v = yp[r * rb.CV + rb.c4];
    add4(s[0], v);
    acc_mul4(s[1], v, v);
  }
  rowblock_colsum_store<2>(s, rb, CVB, RL, {psum, psq});
}

// Fixed-order column sum of two [RB][C] fp32 slabs in fp64: 4 channels x FIN_LANES row-lanes per block (1024 threads).
// (Round 3 tried 16 channels per block with 16-byte row accesses -- a quarter of the memory transactions, the same summation order:
// 16.1 / 12.9 us per launch against 12.3 / 10.0 us for this form in the same profile; the kernel is bound by its fp64 adds and the
// load latency chain, which four times fewer blocks concentrate on four times fewer CUs.  Reverted; profiles/r03_notes.md.)
// The loop is a chain of dependent-latency loads (up to 25 088 partial rows for the stem), so the rows are spread over 256
// lanes per channel with four independent chains each; the lane sums are combined in a fixed order (16 groups of 16).
constexpr int FIN_LANES = 256;

// Row lane rl of channel c: the fp64 sums of rows rl, rl + 256, ... of the two slabs, as four independent chains that are combined at
// the end.  (It accumulates in locals and assigns xo / yo last: with the outputs initialised through the references at the top, the
// four finalize kernels came out with other code.)
__device__ __forceinline__ void slab_lane_chain(const float* __restrict__ a, const float* __restrict__ b, int RB, int C, int c, int rl,
                                                double& xo, double& yo) {
  double x = 0.0, y = 0.0;
  if (c < C) {
    double x1 = 0.0, x2 = 0.0, x3 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
    int r = rl;
    for (; r + 3 * FIN_LANES < RB; r += 4 * FIN_LANES) {
      const float a0 = a[(int64_t)r * C + c], a1 = a[(int64_t)(r + FIN_LANES) * C + c];
      const float a2 = a[(int64_t)(r + 2 * FIN_LANES) * C + c], a3 = a[(int64_t)(r + 3 * FIN_LANES) * C + c];
      const float b0 = b[(int64_t)r * C + c], b1 = b[(int64_t)(r + FIN_LANES) * C + c];
      const float b2 = b[(int64_t)(r + 2 * FIN_LANES) * C + c], b3 = b[(int64_t)(r + 3 * FIN_LANES) * C + c];
      x += (double)a0; x1 += (double)a1; x2 += (double)a2; x3 += (double)a3;
      y += (double)b0; y1 += (double)b1; y2 += (double)b2; y3 += (double)b3;
    }
    for (; r < RB; r += FIN_LANES) {
      x += (double)a[(int64_t)r * C + c];
      y += (double)b[(int64_t)r * C + c];
    }
    x = (x + x1) + (x2 + x3);
    y = (y + y1) + (y2 + y3);
  }
  xo = x;
  yo = y;
}

__device__ __forceinline__ void slab_colsum2(const float* __restrict__ a, const float* __restrict__ b, int RB, int C, int c,
                                             int rl, double (*sh)[FIN_LANES][5], double& sa, double& sb) {
  double x, y;
  slab_lane_chain(a, b, RB, C, c, rl, x, y);
  const int cl = threadIdx.x & 3;
  sh[0][rl][cl] = x;
  sh[1][rl][cl] = y;
  __syncthreads();
  double u = 0.0, v = 0.0;
  if (rl < 16) {  // lane rl sums lanes 16 rl .. 16 rl + 15, in order
    for (int k = 0; k < 16; ++k) {
      u += sh[0][16 * rl + k][cl];
      v += sh[1][16 * rl + k][cl];
    }
  }
  __syncthreads();
  if (rl < 16) {
    sh[0][rl][cl] = u;
    sh[1][rl][cl] = v;
  }
  __syncthreads();
  sa = 0.0;
  sb = 0.0;
  if (rl == 0) {
    for (int k = 0; k < 16; ++k) {
      sa += sh[0][k][cl];
      sb += sh[1][k][cl];
    }
  }
}

// ---- the same column sum over S blocks per channel group (S in {2, 4, 8, 16}) ---------------------------------------------
// The LANES are split over blocks, not the rows: block (cb, s) runs row-lanes [s * 256 / S, (s + 1) * 256 / S) of its four
// channels -- every lane runs slab_lane_chain for the lane it plays -- reduces its 16 / S groups of 16 lanes in lane order
// and publishes those group sums (fp64) to `scratch` [2][C / 4][16][4].  The last block to arrive for cb (one ticket from an
// atomic add on tickets[cb]; nobody spins, nobody waits for anybody) reads the 16 group sums in index order and does what the
// tail of slab_colsum2 does: with slab_lane_chain shared, the same sequence of fp64 additions, hence the same bits.
// Hand-off, the write-through form: every group sum is stored with a relaxed agent-scope atomic store (sc1: it goes through to
// memory, so no release fence and no L2 write-back is needed) -> every storing wave drains vmcnt -> barrier -> one lane takes the
// ticket with a relaxed agent-scope fetch_add; the block that draws S - 1 stores 0 back to the ticket (launches of one stream are
// ordered, so the next launch finds it zero) and tells its other threads through the padding column of `sh`; after the barrier
// lane 0 of each channel reads the sums with relaxed agent-scope atomic loads (sc1, vector path: EVERY load of a handed-off
// byte goes past this CU's L1, so no acquire fence either).
// Returns true in the threads that go on to the per-channel tail (local lane 0 of the last block).
__device__ __forceinline__ bool slab_colsum2_split(const float* __restrict__ a, const float* __restrict__ b, int RB, int C, int c,
                                                   int ll, int S, int s, double (*sh)[FIN_LANES][5], double* scratch,
                                                   unsigned* tickets, double& sa, double& sb) {
  const int nl = FIN_LANES / S;        // lanes of this block
  const int rl = s * nl + ll;          // the lane of slab_colsum2 this thread plays
  double x, y;
  slab_lane_chain(a, b, RB, C, c, rl, x, y);
  const int cl = threadIdx.x & 3;
  const int cb = blockIdx.x;
  sh[0][ll][cl] = x;
  sh[1][ll][cl] = y;
  __syncthreads();
  const int ng = nl / 16;              // groups of this block: global group index s * ng + ll
  unsigned long long* su = reinterpret_cast<unsigned long long*>(scratch) + ((size_t)cb * 16) * 4;
  unsigned long long* sv = su + (size_t)16 * C;     // second quantity: scratch + 16 * C doubles
  if (ll < ng) {  // local lane ll sums local lanes 16 ll .. 16 ll + 15, in order
    double u = 0.0, v = 0.0;
    for (int k = 0; k < 16; ++k) {
      u += sh[0][16 * ll + k][cl];
      v += sh[1][16 * ll + k][cl];
    }
    const int g = s * ng + ll;
    __hip_atomic_store(su + g * 4 + cl, (unsigned long long)__double_as_longlong(u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sv + g * 4 + cl, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(tickets + cb, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == (unsigned)(S - 1);
    if (last) __hip_atomic_store(tickets + cb, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[0][0][4] = last ? 1.0 : 0.0;    // the padding column: no lane sum lives there
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // no instruction: keeps the loads below behind the barrier
  sa = 0.0;
  sb = 0.0;
  if (sh[0][0][4] == 0.0 || ll != 0) return false;
  for (int k = 0; k < 16; ++k) {
    sa += __longlong_as_double((long long)__hip_atomic_load(su + k * 4 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    sb += __longlong_as_double((long long)__hip_atomic_load(sv + k * 4 + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  return c < C;
}

__device__ __forceinline__ void bn_finalize_tail(double s, double q, int c, int64_t M, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float eps, float momentum,
                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                 float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                 float* __restrict__ scale, float* __restrict__ shift) {
  const double mean = s / (double)M;
  double var = q / (double)M - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float meanf = (float)mean;
  save_mean[c] = meanf;
  save_invstd[c] = invstd;
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  shift[c] = beta[c] - meanf * sc;
  if (running_mean != nullptr) {
    const double unbiased = M > 1 ? var * (double)M / (double)(M - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * meanf;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

__global__ __launch_bounds__(4 * FIN_LANES) void bn_finalize_kernel(const float* __restrict__ psum, const float* __restrict__ psq, int RB,
                                                           int64_t M, int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float momentum,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                           float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double sh[2][FIN_LANES][5];
  const int c = blockIdx.x * 4 + (threadIdx.x & 3), rl = threadIdx.x >> 2;
  double s, q;
  slab_colsum2(psum, psq, RB, C, c, rl, sh, s, q);
  if (rl != 0 || c >= C) return;
  bn_finalize_tail(s, q, c, M, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd, scale, shift);
}

// grid (C / 4, S), 4 * FIN_LANES / S threads
__global__ __launch_bounds__(2 * FIN_LANES) void bn_finalize_split_kernel(const float* __restrict__ psum, const float* __restrict__ psq, int RB,
                                                                 int64_t M, int C, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, float momentum,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                 float* __restrict__ scale, float* __restrict__ shift,
                                                                 double* scratch, unsigned* tickets) {
  __shared__ double sh[2][FIN_LANES][5];
  const int c = blockIdx.x * 4 + (threadIdx.x & 3), ll = threadIdx.x >> 2;
  double s, q;
  if (!slab_colsum2_split(psum, psq, RB, C, c, ll, gridDim.y, blockIdx.y, sh, scratch, tickets, s, q)) return;
  bn_finalize_tail(s, q, c, M, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd, scale, shift);
}

__global__ void bn_eval_params_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                      float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = 1.f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * invstd;
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
}

// Streaming reads of tensors that are not touched again before they have left every cache (the raw conv output and the incoming
// gradient in the apply passes) are issued non-temporal, so that the tensors the next kernels read (the pass's own output) keep
// their place in L2 / Infinity Cache: 54.39 -> 53.51 ms per training step in one process (tools/ab_step.py).
// (second box: plain 55.20, level 1 54.68, level 2 54.50).  BDVCIL_BN_NT: 0 = plain loads, 1 = y / dout of bn_apply and
// bn_bwd_apply, 2 (default) = also the residual of bn_apply (the block input: next read in the backward pass).
static int bn_nt_level() {  // read per call (a getenv is nothing beside a launch): tools/ab_step.py flips it between rounds
  const char* e = getenv("BDVCIL_BN_NT");
  return e != nullptr ? atoi(e) : 2;
}
static bool bn_nt_enabled() { return bn_nt_level() != 0; }

// ---- apply -------------------------------------------------------------------------------
// ReLU sign mask: bit e of mask[] = (out[e] > 0) for flat element index e (one uint32 per 32 channels).
// Backward kernels read this 1-bit-per-element mask instead of re-reading the fp32 activation.
__device__ __forceinline__ unsigned nibble_gt0(const float4& o) {
  return (o.x > 0.f ? 1u : 0u) | (o.y > 0.f ? 2u : 0u) | (o.z > 0.f ? 4u : 0u) | (o.w > 0.f ? 8u : 0u);
}
__device__ __forceinline__ unsigned mask_nibble(const uint32_t* __restrict__ mask, int64_t i4) {
  return (mask[i4 >> 3] >> (4 * (int)(i4 & 7))) & 0xFu;
}
// ReLU sign bits of 4 channels derived from the conv output: the forward's own expression (bn_apply_kernel / the PRE loaders)
__device__ __forceinline__ unsigned derive_nibble(const float4 v, const float4 sc, const float4 sh) {
  return (fmaf(v.x, sc.x, sh.x) > 0.f ? 1u : 0u) | (fmaf(v.y, sc.y, sh.y) > 0.f ? 2u : 0u) | (fmaf(v.z, sc.z, sh.z) > 0.f ? 4u : 0u) |
         (fmaf(v.w, sc.w, sh.w) > 0.f ? 8u : 0u);
}
__device__ __forceinline__ float4 apply_nibble(float4 g, unsigned nib) {
  g.x = (nib & 1u) ? g.x : 0.f;
  g.y = (nib & 2u) ? g.y : 0.f;
  g.z = (nib & 4u) ? g.z : 0.f;
  g.w = (nib & 8u) ? g.w : 0.f;
  return g;
}
// The gradient behind a ReLU.  MODE (the kernels' RELU / SIGN): 0 = no ReLU, 1 = the forward's 1-bit mask at flat float4 index i,
// 2 = the sign bits the caller computes (sign2(): derive_nibble of y, or nibble_gt0 of the activation); sign2 runs for MODE 2 only.
// (The callers capture by value: with captures by reference half of the instantiations came out with other code.)
template <int MODE, class F>
__device__ __forceinline__ float4 relu_grad(const float4 g, const uint32_t* __restrict__ mask, int64_t i, F&& sign2) {
  if constexpr (MODE == 1) return apply_nibble(g, mask_nibble(mask, i));
  else if constexpr (MODE == 2) return apply_nibble(g, sign2());
  else return g;
}

// res_scale / res_shift (optional): the residual is itself a raw conv output that still needs its own BatchNorm
// (the downsample branch of a block): r = res * res_scale + res_shift is formed here instead of in a pass of its own.
// ES: bytes per element of y / res / out (common.h: 4 = fp32, 2 = bf16 storage)
template <bool RELU, bool RES, bool NT = false, bool NTR = false, int ES = 4>
__global__ __launch_bounds__(256) void bn_apply_kernel(const void* __restrict__ y, const float4* __restrict__ scale,
                                                        const float4* __restrict__ shift, const void* __restrict__ res,
                                                        const float4* __restrict__ res_scale, const float4* __restrict__ res_shift,
                                                        void* __restrict__ out, uint32_t* __restrict__ mask, int64_t n4, int CV) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // A thread's unit is 16 bytes = U groups of 4 channels (fp32: 1, bf16: 2).  n4 is a multiple of 8 (C % 32 == 0) and so is the
  // stride: the 8 / U lanes of one mask word stay together.
  constexpr int U = ActU<ES>::value;
  constexpr int LW = 8 / U;          // lanes per mask word
  for (int64_t iu = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iu < n4 / U; iu += stride) {
    float4 v[U], r[U], o[U];
    act_ld16<ES, NT>(y, iu, v);
    if (RES) act_ld16<ES, NTR>(res, iu, r);
    unsigned bits = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c4 = (int)((iu * U + u) % CV);
      const float4 sc = scale[c4], sh = shift[c4];
      o[u].x = fmaf(v[u].x, sc.x, sh.x);   // explicit: the conv loaders that apply this BatchNorm themselves (PRE) use the same expression
      o[u].y = fmaf(v[u].y, sc.y, sh.y);
      o[u].z = fmaf(v[u].z, sc.z, sh.z);
      o[u].w = fmaf(v[u].w, sc.w, sh.w);
      if (RES) {
        float4 q = r[u];
        if (res_scale != nullptr) {
          const float4 rs = res_scale[c4], rb = res_shift[c4];
          q.x = q.x * rs.x + rb.x; q.y = q.y * rs.y + rb.y; q.z = q.z * rs.z + rb.z; q.w = q.w * rs.w + rb.w;
        }
        add4(o[u], q);
      }
      if (RELU) {
        bits |= nibble_gt0(o[u]) << (4 * u);
        o[u].x = fmaxf(o[u].x, 0.f); o[u].y = fmaxf(o[u].y, 0.f); o[u].z = fmaxf(o[u].z, 0.f); o[u].w = fmaxf(o[u].w, 0.f);
      }
    }
    if (RELU && mask != nullptr) {
      unsigned m = bits << (4 * U * (threadIdx.x & (LW - 1)));
      m |= __shfl_xor(m, 1, 64);
      m |= __shfl_xor(m, 2, 64);
      if (LW == 8) m |= __shfl_xor(m, 4, 64);
      if ((threadIdx.x & (LW - 1)) == 0) mask[iu / LW] = m;
    }
    act_st16<ES>(out, iu, o);
  }
}

// ---- backward ----------------------------------------------------------------------------
// RELU: 0 = none, 1 = the forward's 1-bit mask, 2 = the sign derived from y (rscale / rshift: the unit's mask was never written)
template <int RELU, int ES = 4>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                              const void* __restrict__ y, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, float* __restrict__ p1,
                                                              float* __restrict__ p2, int64_t M, int C, int CVB, int RL,
                                                              int rows_per_block, const float* __restrict__ rscale,
                                                              const float* __restrict__ rshift) {
  const RowBlock rb(M, C, CVB, rows_per_block);
  const int c4 = rb.c4;
  const float4 mu = reinterpret_cast<const float4*>(mean)[c4];
  const float4 is = reinterpret_cast<const float4*>(invstd)[c4];
  float4 s[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};   // sum g, sum g * xhat
  for (int64_t r = rb.r0 + rb.rl; r < rb.r1; r += RL) {
    const int64_t i = r * rb.CV + c4;
    float4 g = act_ld4<ES>(dout, i);
    const float4 v = act_ld4<ES>(y, i);
    g = relu_grad<RELU>(g, mask, i, [=] {
      return derive_nibble(v, reinterpret_cast<const float4*>(rscale)[c4], reinterpret_cast<const float4*>(rshift)[c4]);
    });
    add4(s[0], g);
    acc_g_xhat4(s[1], g, v, mu, is);
  }
  rowblock_colsum_store<2>(s, rb, CVB, RL, {p1, p2});
}

// coef[0][c] = gamma*invstd, coef[1][c] = sum(g)/M, coef[2][c] = sum(g*xhat)/M
__device__ __forceinline__ void bn_bwd_finalize_tail(double s1, double s2, int c, int64_t M, int C, const float* __restrict__ gamma,
                                                     const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                     float* __restrict__ dbeta, float beta_acc, float* __restrict__ coef) {
  if (dgamma != nullptr) dgamma[c] = (beta_acc != 0.f ? beta_acc * dgamma[c] : 0.f) + (float)s2;
  if (dbeta != nullptr) dbeta[c] = (beta_acc != 0.f ? beta_acc * dbeta[c] : 0.f) + (float)s1;
  const float a = gamma[c] * invstd[c];
  coef[c] = a;
  coef[C + c] = (float)(s1 / (double)M);
  coef[2 * C + c] = (float)(s2 / (double)M);
}
__global__ __launch_bounds__(4 * FIN_LANES) void bn_bwd_finalize_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int RB,
                                                               int64_t M, int C, const float* __restrict__ gamma,
                                                               const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float beta_acc, float* __restrict__ coef) {
  __shared__ double sh[2][FIN_LANES][5];
  const int c = blockIdx.x * 4 + (threadIdx.x & 3), rl = threadIdx.x >> 2;
  double s1, s2;
  slab_colsum2(p1, p2, RB, C, c, rl, sh, s1, s2);
  if (rl != 0 || c >= C) return;
  bn_bwd_finalize_tail(s1, s2, c, M, C, gamma, invstd, dgamma, dbeta, beta_acc, coef);
}

// grid (C / 4, S), 4 * FIN_LANES / S threads (slab_colsum2_split)
__global__ __launch_bounds__(2 * FIN_LANES) void bn_bwd_finalize_split_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int RB,
                                                                     int64_t M, int C, const float* __restrict__ gamma,
                                                                     const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta, float beta_acc, float* __restrict__ coef,
                                                                     double* scratch, unsigned* tickets) {
  __shared__ double sh[2][FIN_LANES][5];
  const int c = blockIdx.x * 4 + (threadIdx.x & 3), ll = threadIdx.x >> 2;
  double s1, s2;
  if (!slab_colsum2_split(p1, p2, RB, C, c, ll, gridDim.y, blockIdx.y, sh, scratch, tickets, s1, s2)) return;
  bn_bwd_finalize_tail(s1, s2, c, M, C, gamma, invstd, dgamma, dbeta, beta_acc, coef);
}

template <int RELU, bool NT = false, int ES = 4>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                            const void* __restrict__ y, const float4* __restrict__ mean,
                                                            const float4* __restrict__ invstd, const float4* __restrict__ coef,
                                                            void* __restrict__ dy, int64_t n4, int CV,
                                                            const float4* __restrict__ rscale, const float4* __restrict__ rshift) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  constexpr int U = ActU<ES>::value;   // 16-byte units: U groups of 4 channels per thread (bn_apply_kernel)
  for (int64_t iu = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iu < n4 / U; iu += stride) {
    float4 gg[U], vv[U], dd[U];
    act_ld16<ES, NT>(dout, iu, gg);
    act_ld16<ES, NT>(y, iu, vv);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = iu * U + u;
      const int c4 = (int)(i % CV);
      const float4 v = vv[u], mu = mean[c4], is = invstd[c4];
      const float4 g = relu_grad<RELU>(gg[u], mask, i, [=] { return derive_nibble(v, rscale[c4], rshift[c4]); });
      const float4 a = coef[c4], b = coef[CV + c4], c = coef[2 * CV + c4];
      dd[u] = bn_dx4(a, b, c, g, v, mu, is);
    }
    act_st16<ES>(dy, iu, dd);
  }
}

// ---- two BatchNorms behind one masked gradient (a block with a downsample branch) ----------------------------------------
// g = dout (.) mask enters the block's last main unit (ya) and the downsample BatchNorm (yb).  Both kernels read dout and the mask
// once; they share RowBlock, rowblock_colsum_store, acc_g_xhat4 and bn_dx4 with bn_bwd_partial_kernel<1> / bn_bwd_apply_kernel<1>,
// so the partial rows and the gradients carry the bits of two separate bdv_bn_backward calls.
template <int ES = 4>
__global__ __launch_bounds__(256) void bn_bwd_partial_pair_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                                   const void* __restrict__ ya, const float* __restrict__ mean_a,
                                                                   const float* __restrict__ invstd_a, const void* __restrict__ yb,
                                                                   const float* __restrict__ mean_b, const float* __restrict__ invstd_b,
                                                                   float* __restrict__ p1, float* __restrict__ pa2,
                                                                   float* __restrict__ pb2, int64_t M, int C, int CVB, int RL,
                                                                   int rows_per_block) {
  const RowBlock rb(M, C, CVB, rows_per_block);
  const int c4 = rb.c4;
  const float4 mu = reinterpret_cast<const float4*>(mean_a)[c4];
  const float4 is = reinterpret_cast<const float4*>(invstd_a)[c4];
  const float4 mub = reinterpret_cast<const float4*>(mean_b)[c4];
  const float4 isb = reinterpret_cast<const float4*>(invstd_b)[c4];
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 s[3] = {z4, z4, z4};   // sum g (the same chain for both BatchNorms: one slab), sum g * xhat_a, sum g * xhat_b
  for (int64_t r = rb.r0 + rb.rl; r < rb.r1; r += RL) {
    const int64_t i = r * rb.CV + c4;
    float4 g = act_ld4<ES>(dout, i);
    const float4 v = act_ld4<ES>(ya, i);
    const float4 w = act_ld4<ES>(yb, i);
    g = apply_nibble(g, mask_nibble(mask, i));
    add4(s[0], g);
    acc_g_xhat4(s[1], g, v, mu, is);
    acc_g_xhat4(s[2], g, w, mub, isb);
  }
  rowblock_colsum_store<3>(s, rb, CVB, RL, {p1, pa2, pb2});
}

template <bool NT = false, int ES = 4>
__global__ __launch_bounds__(256) void bn_bwd_apply_pair_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                                 const void* __restrict__ ya, const float4* __restrict__ mean_a,
                                                                 const float4* __restrict__ invstd_a, const float4* __restrict__ coef_a,
                                                                 void* __restrict__ dya, const void* __restrict__ yb,
                                                                 const float4* __restrict__ mean_b, const float4* __restrict__ invstd_b,
                                                                 const float4* __restrict__ coef_b, void* __restrict__ dyb, int64_t n4,
                                                                 int CV) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  constexpr int U = ActU<ES>::value;   // 16-byte units: U groups of 4 channels per thread (bn_apply_kernel)
  for (int64_t iu = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iu < n4 / U; iu += stride) {
    float4 gg[U], vv[U], ww[U], da[U], db[U];
    act_ld16<ES, NT>(dout, iu, gg);
    act_ld16<ES, NT>(ya, iu, vv);
    act_ld16<ES, NT>(yb, iu, ww);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = iu * U + u;
      const int c4 = (int)(i % CV);
      const float4 g = apply_nibble(gg[u], mask_nibble(mask, i));
      {
        const float4 v = vv[u], mu = mean_a[c4], is = invstd_a[c4];
        const float4 a = coef_a[c4], b = coef_a[CV + c4], c = coef_a[2 * CV + c4];
        da[u] = bn_dx4(a, b, c, g, v, mu, is);
      }
      {
        const float4 v = ww[u], mu = mean_b[c4], is = invstd_b[c4];
        const float4 a = coef_b[c4], b = coef_b[CV + c4], c = coef_b[2 * CV + c4];
        db[u] = bn_dx4(a, b, c, g, v, mu, is);
      }
    }
    act_st16<ES>(dya, iu, da);
    act_st16<ES>(dyb, iu, db);
  }
}

// The same pass with R units per thread that share their channels: a thread's units lie L units apart, L = max(256, CV / U) a
// multiple of both the block and the channel period, so the ten per-channel vectors of the two BatchNorms are loaded once per
// thread instead of once per unit, and the 3 R streaming loads of a thread are in flight together.  A block covers R spans of
// 4 KB.  Per element the gradient is bn_dx4, as in bn_bwd_apply_kernel.
template <bool NT, int ES, int R>
__global__ __launch_bounds__(256) void bn_bwd_apply_pair_rows_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                                      const void* __restrict__ ya, const float4* __restrict__ mean_a,
                                                                      const float4* __restrict__ invstd_a, const float4* __restrict__ coef_a,
                                                                      void* __restrict__ dya, const void* __restrict__ yb,
                                                                      const float4* __restrict__ mean_b, const float4* __restrict__ invstd_b,
                                                                      const float4* __restrict__ coef_b, void* __restrict__ dyb, int64_t nu,
                                                                      int CV, int L) {
  constexpr int U = ActU<ES>::value;
  const int chunks = L / 256;
  const int64_t base = (int64_t)(blockIdx.x / chunks) * R * L + (int64_t)(blockIdx.x % chunks) * 256 + threadIdx.x;
  if (base >= nu) return;
  float4 mua[U], isa[U], aa[U], ba[U], ca[U], mub[U], isb[U], ab[U], bb[U], cb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c4 = (int)((base * U + u) % CV);
    mua[u] = mean_a[c4]; isa[u] = invstd_a[c4]; aa[u] = coef_a[c4]; ba[u] = coef_a[CV + c4]; ca[u] = coef_a[2 * CV + c4];
    mub[u] = mean_b[c4]; isb[u] = invstd_b[c4]; ab[u] = coef_b[c4]; bb[u] = coef_b[CV + c4]; cb[u] = coef_b[2 * CV + c4];
  }
  float4 gg[R][U], vv[R][U], ww[R][U];
  unsigned nib[R][U];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t iu = base + (int64_t)k * L;
    if (iu < nu) {
      act_ld16<ES, NT>(dout, iu, gg[k]);
      act_ld16<ES, NT>(ya, iu, vv[k]);
      act_ld16<ES, NT>(yb, iu, ww[k]);
#pragma unroll
      for (int u = 0; u < U; ++u) nib[k][u] = mask_nibble(mask, iu * U + u);
    }
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t iu = base + (int64_t)k * L;
    if (iu < nu) {
      float4 da[U], db[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 g = apply_nibble(gg[k][u], nib[k][u]);
        {
          const float4 v = vv[k][u], mu = mua[u], is = isa[u], a = aa[u], b = ba[u], c = ca[u];
          da[u] = bn_dx4(a, b, c, g, v, mu, is);
        }
        {
          const float4 v = ww[k][u], mu = mub[u], is = isb[u], a = ab[u], b = bb[u], c = cb[u];
          db[u] = bn_dx4(a, b, c, g, v, mu, is);
        }
      }
      act_st16<ES>(dya, iu, da);
      act_st16<ES>(dyb, iu, db);
    }
  }
}

// ---- BatchNorm(+ReLU) backward behind a MaxPool2d(3, 2, 1) (the stem) --------------------------------------------
// The gradient entering the BN+ReLU is the max-pool backward of dpool; it is gathered on the fly (pool_bwd_gather2x2)
// in both passes instead of being materialised: thread = (2x2 input block, 4 channels), grid.y strides (frame, block
// row).  256 % CV == 0, so a thread keeps its 4 channels and the per-block reduction groups threads by tid % CV.
template <bool APPLY, int ESD = 4>
__global__ __launch_bounds__(256) void bn_bwd_pool_kernel(const void* __restrict__ dpool, const uchar4* __restrict__ idx,
                                                           const uint32_t* __restrict__ mask, const float4* __restrict__ y,
                                                           const float4* __restrict__ mean, const float4* __restrict__ invstd,
                                                           const float4* __restrict__ coef, float4* __restrict__ dy,
                                                           float* __restrict__ p1, float* __restrict__ p2, int N, int H, int W,
                                                           int CV, int Ho, int Wo) {
  __shared__ float4 sh[2][256];
  const int tid = threadIdx.x;
  const int c4 = tid % CV;
  const float4 mu = mean[c4], is = invstd[c4];
  float4 ca, cb, cc;
  if (APPLY) {
    ca = coef[c4];
    cb = coef[CV + c4];
    cc = coef[2 * CV + c4];
  }
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  for (int row = blockIdx.y; row < N * Ho; row += gridDim.y) {
    const int n = row / Ho, i = row - n * Ho;
    const int64_t obase = (int64_t)n * Ho * Wo * CV;
    const int64_t ibase = (int64_t)n * H * W * CV;
    const bool down = i + 1 < Ho, h1ok = 2 * i + 1 < H;
    for (int q = blockIdx.x * blockDim.x + tid; q < Wo * CV; q += gridDim.x * blockDim.x) {
      const int j = q / CV;  // q % CV == c4
      const bool right = j + 1 < Wo, w1ok = 2 * j + 1 < W;
      float4 g[4];
      pool_bwd_gather2x2<ESD>(dpool, idx, obase + (i * Wo + j) * CV + c4, CV, Wo, right, down, g);
      const int64_t p00 = ibase + ((2 * i) * W + 2 * j) * CV + c4;
      const int64_t pix[4] = {p00, p00 + CV, p00 + (int64_t)W * CV, p00 + (int64_t)(W + 1) * CV};
      const bool ok[4] = {true, w1ok, h1ok, h1ok && w1ok};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!ok[k]) continue;
        const float4 gv = apply_nibble(g[k], mask_nibble(mask, pix[k]));
        const float4 v = y[pix[k]];
        const float4 xh = bn_xhat4(v, mu, is);   // ahead of the branch, as before this kernel took the helpers: inside the else,
                                                 // bn_bwd_pool_kernel<true, 2> comes out with other code of the same size
        if (APPLY) {
          dy[pix[k]] = bn_dx4(ca, cb, cc, gv, v, mu, is);
        } else {
          add4(s1, gv);
          acc_mul4(s2, gv, xh);
        }
      }
    }
  }
  if (!APPLY) {
    sh[0][tid] = s1;
    sh[1][tid] = s2;
    __syncthreads();
    if (tid < CV) {
      for (int k = 1; k < 256 / CV; ++k) {
        const float4 a = sh[0][k * CV + tid], b = sh[1][k * CV + tid];
        add4(s1, a);
        add4(s2, b);
      }
      const int64_t slab_row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
      reinterpret_cast<float4*>(p1)[slab_row * CV + tid] = s1;
      reinterpret_cast<float4*>(p2)[slab_row * CV + tid] = s2;
    }
  }
}

// ---- backward through an eval-mode BatchNorm (running statistics: constants of the step) -----------------------------------
// dz = dout (.) sign, dy = dz * scale with scale = gamma * invstd_running (bdv_bn_eval_params): the mean terms of the train-mode
// apply vanish, so dy does not wait for the column sums and the backward is ONE pass.  One multiply per element, never a division
// by gamma or scale (gamma = 0 and gamma < 0 are ordinary channels).
// SIGN: 0 = no ReLU, 1 = the forward's 1-bit mask, 2 = the sign of the activation tensor itself (act > 0: a unit whose affine is
// frozen keeps neither y nor a mask).  DZ: also write the masked gradient (the identity path and the downsample BatchNorm read it).

// No parameter gradients: the streaming form, one 16-byte unit per lane and iteration (bn_bwd_apply_kernel's decomposition).
template <int SIGN, bool DZ, bool NT = false, int ES = 4>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                           const void* __restrict__ act, const float4* __restrict__ scale,
                                                           void* __restrict__ dy, void* __restrict__ dz, int64_t n4, int CV) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  constexpr int U = ActU<ES>::value;
  for (int64_t iu = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; iu < n4 / U; iu += stride) {
    float4 gg[U], aa[U], dd[U];
    act_ld16<ES, NT>(dout, iu, gg);
    if (SIGN == 2) act_ld16<ES, false>(act, iu, aa);   // the activation is an operand of the weight gradient next: a plain load
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = iu * U + u;
      const float4 sc = scale[(int)(i % CV)];
      const float4 g = relu_grad<SIGN>(gg[u], mask, i, [=] { return nibble_gt0(aa[u]); });
      gg[u] = g;
      dd[u] = mul4(g, sc);
    }
    act_st16<ES>(dy, iu, dd);
    if (DZ) act_st16<ES>(dz, iu, gg);
  }
}

// With parameter gradients: bn_bwd_partial_kernel's block / lane decomposition and its two sums (RowBlock, add4, acc_g_xhat4,
// rowblock_colsum_store), with the running statistics as mean / invstd; the lane that has g in registers writes dy (and dz) on the way.
template <int SIGN, bool DZ, bool NT = false, int ES = 4>
__global__ __launch_bounds__(256) void bn_eval_bwd_stats_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                                 const void* __restrict__ act, const void* __restrict__ y,
                                                                 const float* __restrict__ scale, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, void* __restrict__ dy,
                                                                 void* __restrict__ dz, float* __restrict__ p1, float* __restrict__ p2,
                                                                 int64_t M, int C, int CVB, int RL, int rows_per_block) {
  const RowBlock rb(M, C, CVB, rows_per_block);
  const int c4 = rb.c4;
  const float4 mu = reinterpret_cast<const float4*>(mean)[c4];
  const float4 is = reinterpret_cast<const float4*>(invstd)[c4];
  const float4 sc = reinterpret_cast<const float4*>(scale)[c4];
  float4 s[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};   // sum g, sum g * xhat
  for (int64_t r = rb.r0 + rb.rl; r < rb.r1; r += RL) {
    const int64_t i = r * rb.CV + c4;
    float4 g = act_ld4<ES, NT>(dout, i);
    const float4 v = act_ld4<ES, NT>(y, i);
    float4 av;   // loaded here, not in the lambda: its copy of `act` would not be __restrict__
    if (SIGN == 2) av = act_ld4<ES>(act, i);
    g = relu_grad<SIGN>(g, mask, i, [=] { return nibble_gt0(av); });
    act_st4<ES>(dy, i, mul4(g, sc));
    if (DZ) act_st4<ES>(dz, i, g);
    add4(s[0], g);
    acc_g_xhat4(s[1], g, v, mu, is);
  }
  rowblock_colsum_store<2>(s, rb, CVB, RL, {p1, p2});
}

template <int ES = 4>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const void* __restrict__ dout, const uint32_t* __restrict__ mask,
                                                        const void* __restrict__ add, void* __restrict__ g, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 d = apply_nibble(act_ld4<ES>(dout, i), mask_nibble(mask, i));
    if (add != nullptr) {
      const float4 a = act_ld4<ES>(add, i);
      d.x += a.x; d.y += a.y; d.z += a.z; d.w += a.w;   // (through add4 the bf16 instantiation takes two more VGPRs)
    }
    act_st4<ES>(g, i, d);
  }
}

template <int ES = 4>
__global__ __launch_bounds__(256) void add_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                   void* __restrict__ out, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 x = act_ld4<ES>(a, i), y = act_ld4<ES>(b, i);
    act_st4<ES>(out, i, make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w));
  }
}

// ---- finalize launches ------------------------------------------------------------------------------------------------
// Blocks per channel group of the two finalize kernels.  One block streams rows * 32 bytes of 16-byte pieces through one CU; S
// blocks spread the same lanes over S CUs and pay a ticket and the last arriver's serial read of 1 KB (slab_colsum2_split):
// 1.0 - 1.5 us at S = 2 ... 4, more with every doubling of the block count.  Measured over the (rows, C) pairs of the R50 and
// I3D graphs (tools/bench_bn.py --finalize, table in profiles/r04_bn_finalize.txt): the split wins where a channel group has at
// least 2048 rows AND the two slabs together hold 3 MB or more (rows * C >= 6144 * 64) -- the stem (25 088 x 64: 61 -> 18.5 us),
// its max-pool backward (8192 x 64: 15.8 -> 7.2), layer 1 (6272 x 64 / 128 / 256: 8.1 -> 6.0, 22.5 -> 11.6, 29.0 -> 18.7) and
// the I3D layer-1 sites (3136 x 256: 16.3 -> 11.2) -- with 8 blocks from 8192 rows and 4 below; everything smaller is fastest on
// the one-block kernel (3 - 5 us), and 16 blocks never won.
int bn_fin_splits(int rows, int C) {
  if (rows < 2048 || (int64_t)rows * C < 6144 * 64) return 1;
  return rows >= 8192 ? 8 : 4;
}

// Scratch layout: FIN_TICKET_BYTES of ticket words (one per channel group: C <= FIN_TICKET_BYTES) at the start, then
// 2 x 16 x C doubles.  The tickets sit at a place that does not depend on C, so one buffer serves launches of every C: group sums
// of a wide launch never land on a ticket that a narrower launch expects to find zero.
constexpr size_t FIN_TICKET_BYTES = 4096;
size_t bn_fin_scratch_bytes(int C) { return FIN_TICKET_BYTES + (size_t)C * 256; }

// S: 1 = the one-block kernel, 2 / 4 / 8 / 16 = split, 0 = bn_fin_splits (1 without scratch).  Returns the S to launch or -1.
int bn_fin_resolve(int S, int rows, int C, const void* scratch, size_t scratch_bytes, const char* who) {
  if (!(S == 0 || S == 1 || S == 2 || S == 4 || S == 8 || S == 16)) {
    bdv_set_error("%s: splits %d (0 = planner, 1, 2, 4, 8 or 16)", who, S);
    return -1;
  }
  if (S == 0) S = scratch != nullptr && (size_t)C <= FIN_TICKET_BYTES ? bn_fin_splits(rows, C) : 1;
  if (S > 1 && (scratch == nullptr || !bdv_aligned16(scratch) || scratch_bytes < bn_fin_scratch_bytes(C) || C % 4 != 0 ||
                (size_t)C > FIN_TICKET_BYTES)) {
    bdv_set_error("%s: %d finalize blocks per channel group need C <= 4096 and bdv_bn_finalize_scratch_bytes(C) of zero-initialised scratch", who, S);
    return -1;
  }
  return S;
}

// One block per channel group (`one`), or S blocks (`split`, which takes the group-sum scratch and the tickets behind `a...`)
template <class K1, class KS, class... A>
void launch_fin(K1 one, KS split, int C, int S, void* scratch, hipStream_t s, A... a) {
  if (S == 1)
    hipLaunchKernelGGL(one, dim3((C + 3) / 4), dim3(4 * FIN_LANES), 0, s, a...);
  else
    hipLaunchKernelGGL(split, dim3(C / 4, S), dim3(4 * FIN_LANES / S), 0, s, a..., (double*)((char*)scratch + FIN_TICKET_BYTES),
                       (unsigned*)scratch);
}
void launch_bn_finalize(const float* psum, const float* psq, int rows, int64_t M, int C, const float* gamma, const float* beta, float eps,
                        float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* scale,
                        float* shift, int S, void* scratch, hipStream_t s) {
  launch_fin(bn_finalize_kernel, bn_finalize_split_kernel, C, S, scratch, s, psum, psq, rows, M, C, gamma, beta, eps, momentum,
             running_mean, running_var, save_mean, save_invstd, scale, shift);
}
void launch_bn_bwd_finalize(const float* q1, const float* q2, int rows, int64_t M, int C, const float* gamma, const float* invstd,
                            float* dgamma, float* dbeta, float beta_acc, float* coef, int S, void* scratch, hipStream_t s) {
  launch_fin(bn_bwd_finalize_kernel, bn_bwd_finalize_split_kernel, C, S, scratch, s, q1, q2, rows, M, C, gamma, invstd, dgamma, dbeta,
             beta_acc, coef);
}

// ---- what the entry points share ------------------------------------------------------------------------------------------
// grid of an elementwise pass over n4 groups of 4 channels: one 16-byte unit per thread (ActU: fp32 BDV_F32_UNITS groups, bf16 2)
dim3 act_grid(int64_t n4, int act_dtype) { return dim3(bdv_ew_grid(act_dtype == BDV_ACT_BF16 ? n4 / 2 : n4 / BDV_F32_UNITS)); }

// The workspace of bdv_bn_workspace_bytes: two partial slabs, then the 3*C apply coefficients
struct BnWs {
  float *p1, *p2, *coef;
};
int bn_ws_carve(void* workspace, size_t workspace_bytes, int C, const char* who, BnWs* w) {
  if (workspace_bytes < bdv_bn_workspace_bytes(0, C)) {
    bdv_set_error("%s: workspace too small", who);
    return BDV_EWORKSPACE;
  }
  w->p1 = (float*)workspace;
  w->p2 = w->p1 + MAX_RB_TIMES_C;
  w->coef = w->p2 + MAX_RB_TIMES_C;
  return BDV_OK;
}

// The two column sums a backward finalize reads: the caller's tile sums [2][stat_rows][C] (the producer of dout, a dgrad epilogue,
// already reduced per 128-row tile: no statistics pass) or the slabs p1 / p2 of this call's own pass, RB rows
struct BnSums {
  const float *q1, *q2;
  int rows;
  bool given;
};
BnSums bn_sums(const float* stat_partial, int stat_rows, int C, const float* p1, const float* p2, int RB) {
  if (stat_partial != nullptr) return {stat_partial, stat_partial + (size_t)stat_rows * C, stat_rows, true};
  return {p1, p2, RB, false};
}

// ---- template arguments from tables: the rows are the instantiations that exist, a launch looks its row up -----------------------
template <class Row, int N, class P>
int find_row(const Row (&table)[N], P&& match) {
  for (int i = 0; i < N; ++i)
    if (match(table[i])) return i;
  return -1;
}
// bn_apply_kernel<RELU, RES, NT, NTR>: non-temporal loads only in the ReLU forms (BDVCIL_BN_NT: 1 = y, 2 = also the residual)
struct BnApplyRow {
  bool relu, res, nt, ntr;
};
constexpr BnApplyRow kBnApplyRows[] = {{true, true, true, true},    {true, true, true, false},   {true, false, true, false},
                                       {true, true, false, false},  {true, false, false, false}, {false, true, false, false},
                                       {false, false, false, false}};
constexpr int kNumBnApplyRows = sizeof(kBnApplyRows) / sizeof(kBnApplyRows[0]);
// bn_bwd_apply_kernel<RELU, NT>: RELU 0 = none, 1 = mask, 2 = sign derived from y; no non-temporal form without ReLU
struct BnBwdApplyRow {
  int relu;
  bool nt;
};
constexpr BnBwdApplyRow kBnBwdApplyRows[] = {{2, true}, {2, false}, {1, true}, {1, false}, {0, false}};
constexpr int kNumBnBwdApplyRows = sizeof(kBnBwdApplyRows) / sizeof(kBnBwdApplyRows[0]);
// bn_eval_bwd_kernel / bn_eval_bwd_stats_kernel<SIGN, DZ, NT>: all 12 combinations exist; row I = (SIGN * 2 + DZ) * 2 + NT
constexpr int kNumBnEvalRows = 12;

template <int ES>
void launch_bn_bwd_partial(int relu_mode, const BnGrid& b, hipStream_t s, const void* dout, const uint32_t* relu_mask, const void* y,
                           const float* mean, const float* invstd, float* p1, float* p2, int64_t M, int C, const float* relu_scale,
                           const float* relu_shift) {
  static_index<3>(relu_mode, [&](auto mode) {
    hipLaunchKernelGGL((bn_bwd_partial_kernel<decltype(mode)::value, ES>), dim3(b.RB, b.CC), dim3(256), 0, s, dout, relu_mask, y, mean,
                       invstd, p1, p2, M, C, b.CVB, b.RL, b.rows_per_block, relu_scale, relu_shift);
  });
}

}  // namespace

extern "C" size_t bdv_bn_workspace_bytes(int64_t M, int C) {
  (void)M;
  // two partial slabs (<= MAX_RB_TIMES_C floats each) + 3*C coefficients
  return (size_t)(2 * MAX_RB_TIMES_C + 3 * (size_t)(C > 0 ? C : 0)) * sizeof(float);
}

extern "C" int bdv_bn_train_stats(const float* y, int64_t M, int C, const float* gamma, const float* beta, float eps,
                                  float momentum, float* running_mean, float* running_var, float* save_mean,
                                  float* save_invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  BDV_REQUIRE(y && gamma && beta && save_mean && save_invstd && scale && shift && workspace, "bdv_bn_train_stats: null pointer");
  BDV_REQUIRE(M > 0 && bn_c_ok(C), "bdv_bn_train_stats: unsupported M=%lld C=%d", (long long)M, C);
  BDV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bdv_bn_train_stats: running stats must come in pairs");
  BDV_REQUIRE(bdv_aligned16(y) && bdv_aligned16(workspace), "bdv_bn_train_stats: alignment");
  BnWs w;   // psum = p1, psq = p2; the coefficients are not used
  if (int e = bn_ws_carve(workspace, workspace_bytes, C, "bdv_bn_train_stats", &w)) return e;
  const BnGrid b = bn_grid(M, C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_partial_kernel, dim3(b.RB, b.CC), dim3(256), 0, s, y, w.p1, w.p2, M, C, b.CVB, b.RL, b.rows_per_block);
  BDV_LAUNCH_CHECK("bdv_bn_train_stats(partial)");
  launch_bn_finalize(w.p1, w.p2, b.RB, M, C, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd, scale, shift,
                     1, nullptr, s);
  BDV_LAUNCH_CHECK("bdv_bn_train_stats(finalize)");
  return BDV_OK;
}

extern "C" size_t bdv_bn_finalize_scratch_bytes(int C) { return C > 0 ? bn_fin_scratch_bytes(C) : 0; }

extern "C" int bdv_bn_finalize_splits(int rows, int C) { return rows > 0 && C > 0 && C % 4 == 0 ? bn_fin_splits(rows, C) : 1; }

extern "C" int bdv_bn_train_finalize_split(const float* partial, int rows, int64_t M, int C, const float* gamma, const float* beta,
                                           float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                           float* save_invstd, float* scale, float* shift, int splits, void* fin_scratch,
                                           size_t fin_scratch_bytes, void* stream) {
  BDV_REQUIRE(partial && gamma && beta && save_mean && save_invstd && scale && shift, "bdv_bn_train_finalize: null pointer");
  BDV_REQUIRE(rows > 0 && M > 0 && C > 0 && C % 4 == 0, "bdv_bn_train_finalize: bad shape");
  BDV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bdv_bn_train_finalize: running stats must come in pairs");
  const int S = bn_fin_resolve(splits, rows, C, fin_scratch, fin_scratch_bytes, "bdv_bn_train_finalize");
  if (S < 0) return BDV_EINVAL;
  launch_bn_finalize(partial, partial + (size_t)rows * C, rows, M, C, gamma, beta, eps, momentum, running_mean, running_var, save_mean,
                     save_invstd, scale, shift, S, fin_scratch, (hipStream_t)stream);
  BDV_LAUNCH_CHECK("bdv_bn_train_finalize");
  return BDV_OK;
}

extern "C" int bdv_bn_train_finalize(const float* partial, int rows, int64_t M, int C, const float* gamma, const float* beta,
                                     float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                     float* save_invstd, float* scale, float* shift, void* stream) {
  return bdv_bn_train_finalize_split(partial, rows, M, C, gamma, beta, eps, momentum, running_mean, running_var, save_mean, save_invstd,
                                     scale, shift, 1, nullptr, 0, stream);
}

extern "C" int bdv_bn_eval_params(int C, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* scale, float* shift, void* stream) {
  BDV_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && C > 0, "bdv_bn_eval_params: bad argument");
  hipLaunchKernelGGL(bn_eval_params_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, C, gamma, beta,
                     running_mean, running_var, eps, scale, shift);
  BDV_LAUNCH_CHECK("bdv_bn_eval_params");
  return BDV_OK;
}

extern "C" int bdv_bn_apply(const void* y, const float* scale, const float* shift, const void* res, const float* res_scale,
                            const float* res_shift, void* out, uint32_t* relu_mask, int64_t M, int C, int relu, int act_dtype,
                            void* stream) {
  BDV_REQUIRE(y && scale && shift && out, "bdv_bn_apply: null pointer");
  BDV_REQUIRE_ACT(act_dtype, "bdv_bn_apply");
  BDV_REQUIRE((res_scale == nullptr) == (res_shift == nullptr) && (res_scale == nullptr || res != nullptr),
              "bdv_bn_apply: res_scale and res_shift come together and need res");
  BDV_REQUIRE(bdv_aligned16(res_scale) && bdv_aligned16(res_shift), "bdv_bn_apply: alignment");
  BDV_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "bdv_bn_apply: bad shape");
  BDV_REQUIRE(relu_mask == nullptr || (relu && C % 32 == 0), "bdv_bn_apply: relu_mask needs relu and C %% 32 == 0");
  BDV_REQUIRE(bdv_aligned16(y) && bdv_aligned16(out) && bdv_aligned16(scale) && bdv_aligned16(shift) &&
                  (res == nullptr || bdv_aligned16(res)), "bdv_bn_apply: alignment");
  BDV_REQUIRE(act_dtype == BDV_ACT_F32 || C % 8 == 0, "bdv_bn_apply: bf16 tensors need C %% 8 == 0 (16-byte units)");
  const int64_t n4 = M * C / 4;
  const int CV = C / 4;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = act_grid(n4, act_dtype), blk(256);
  const float4 *sc = (const float4*)scale, *sh = (const float4*)shift;
  const float4 *rs = (const float4*)res_scale, *rb = (const float4*)res_shift;
  const BnApplyRow want = {relu != 0, res != nullptr, relu && bn_nt_enabled(), relu && res && bn_nt_level() >= 2};
  const int row = find_row(kBnApplyRows, [&](const BnApplyRow& r) {
    return r.relu == want.relu && r.res == want.res && r.nt == want.nt && r.ntr == want.ntr;
  });
  BDV_REQUIRE(row >= 0, "bdv_bn_apply: no kernel is compiled for relu %d, residual %d, non-temporal %d / %d", want.relu, want.res, want.nt,
              want.ntr);
  BDV_ACT_SWITCH(act_dtype, ES, static_index<kNumBnApplyRows>(row, [&](auto ri) {
    constexpr BnApplyRow r = kBnApplyRows[decltype(ri)::value];
    hipLaunchKernelGGL((bn_apply_kernel<r.relu, r.res, r.nt, r.ntr, ES>), grid, blk, 0, s, y, sc, sh, res, rs, rb, out, relu_mask, n4, CV);
  }));
  BDV_LAUNCH_CHECK("bdv_bn_apply");
  return BDV_OK;
}

extern "C" int bdv_bn_backward_split(const void* dout, const uint32_t* relu_mask, const void* y, const float* gamma,
                                     const float* save_mean, const float* save_invstd, void* dy, float* dgamma,
                                     float* dbeta, float beta_acc, int64_t M, int C, int relu, const float* stat_partial,
                                     int stat_rows, const float* relu_scale, const float* relu_shift, void* workspace,
                                     size_t workspace_bytes, int act_dtype, int splits, void* fin_scratch,
                                     size_t fin_scratch_bytes, void* stream) {
  BDV_REQUIRE(dout && y && gamma && save_mean && save_invstd && dy && workspace, "bdv_bn_backward: null pointer");
  BDV_REQUIRE_ACT(act_dtype, "bdv_bn_backward");
  BDV_REQUIRE(stat_partial == nullptr || (stat_rows > 0 && bdv_aligned16(stat_partial)), "bdv_bn_backward: bad stat_partial");
  const bool derive = relu && relu_mask == nullptr && relu_scale != nullptr;
  BDV_REQUIRE(!relu || derive || (relu_mask && C % 32 == 0), "bdv_bn_backward: relu needs the forward ReLU mask (C %% 32 == 0) or relu_scale / relu_shift");
  BDV_REQUIRE(!derive || (relu_shift != nullptr && bdv_aligned16(relu_scale) && bdv_aligned16(relu_shift)), "bdv_bn_backward: relu_scale / relu_shift");
  BDV_REQUIRE(M > 0 && bn_c_ok(C), "bdv_bn_backward: unsupported M=%lld C=%d", (long long)M, C);
  BDV_REQUIRE(act_dtype == BDV_ACT_F32 || C % 8 == 0, "bdv_bn_backward: bf16 tensors need C %% 8 == 0 (16-byte units)");
  BDV_REQUIRE(bdv_aligned16(dout) && bdv_aligned16(y) && bdv_aligned16(dy) && bdv_aligned16(workspace) &&
                  bdv_aligned16(save_mean) && bdv_aligned16(save_invstd), "bdv_bn_backward: alignment");
  BnWs w;
  if (int e = bn_ws_carve(workspace, workspace_bytes, C, "bdv_bn_backward", &w)) return e;
  const BnGrid b = bn_grid(M, C);
  const BnSums sums = bn_sums(stat_partial, stat_rows, C, w.p1, w.p2, b.RB);
  const int S = bn_fin_resolve(splits, sums.rows, C, fin_scratch, fin_scratch_bytes, "bdv_bn_backward");
  if (S < 0) return BDV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int relu_mode = derive ? 2 : relu ? 1 : 0;   // the kernels' RELU
  const bool nt = relu_mode != 0 && bn_nt_enabled();
  const int row = find_row(kBnBwdApplyRows, [&](const BnBwdApplyRow& r) { return r.relu == relu_mode && r.nt == nt; });
  BDV_REQUIRE(row >= 0, "bdv_bn_backward: no apply kernel is compiled for relu mode %d, non-temporal %d", relu_mode, (int)nt);
  if (!sums.given) {
    BDV_ACT_SWITCH(act_dtype, ES, launch_bn_bwd_partial<ES>(relu_mode, b, s, dout, relu_mask, y, save_mean, save_invstd, w.p1, w.p2, M, C,
                                                            relu_scale, relu_shift));
    BDV_LAUNCH_CHECK("bdv_bn_backward(partial)");
  }
  launch_bn_bwd_finalize(sums.q1, sums.q2, sums.rows, M, C, gamma, save_invstd, dgamma, dbeta, beta_acc, w.coef, S, fin_scratch, s);
  BDV_LAUNCH_CHECK("bdv_bn_backward(finalize)");
  const int64_t n4 = M * C / 4;
  const dim3 grid = act_grid(n4, act_dtype), blk(256);
  const float4 *rs4 = (const float4*)relu_scale, *rh4 = (const float4*)relu_shift;
  BDV_ACT_SWITCH(act_dtype, ES, static_index<kNumBnBwdApplyRows>(row, [&](auto ri) {
    constexpr BnBwdApplyRow r = kBnBwdApplyRows[decltype(ri)::value];
    hipLaunchKernelGGL((bn_bwd_apply_kernel<r.relu, r.nt, ES>), grid, blk, 0, s, dout, relu_mask, y, (const float4*)save_mean,
                       (const float4*)save_invstd, (const float4*)w.coef, dy, n4, C / 4, rs4, rh4);
  }));
  BDV_LAUNCH_CHECK("bdv_bn_backward(apply)");
  return BDV_OK;
}

extern "C" int bdv_bn_backward(const void* dout, const uint32_t* relu_mask, const void* y, const float* gamma,
                               const float* save_mean, const float* save_invstd, void* dy, float* dgamma,
                               float* dbeta, float beta_acc, int64_t M, int C, int relu, const float* stat_partial,
                               int stat_rows, const float* relu_scale, const float* relu_shift, void* workspace,
                               size_t workspace_bytes, int act_dtype, void* stream) {
  return bdv_bn_backward_split(dout, relu_mask, y, gamma, save_mean, save_invstd, dy, dgamma, dbeta, beta_acc, M, C, relu, stat_partial,
                               stat_rows, relu_scale, relu_shift, workspace, workspace_bytes, act_dtype, 1, nullptr, 0, stream);
}

extern "C" size_t bdv_bn_pair_workspace_bytes(int64_t M, int C) {
  (void)M;
  // three partial slabs (sum g is one slab for both BatchNorms) + 2 x 3*C coefficients
  return (size_t)(3 * MAX_RB_TIMES_C + 6 * (size_t)(C > 0 ? C : 0)) * sizeof(float);
}

extern "C" int bdv_bn_backward_pair(const void* dout, const uint32_t* relu_mask, const void* ya, const float* gamma_a,
                                    const float* mean_a, const float* invstd_a, const float* stat_partial_a, int stat_rows_a,
                                    void* dya, float* dgamma_a, float* dbeta_a, const void* yb, const float* gamma_b,
                                    const float* mean_b, const float* invstd_b, void* dyb, float* dgamma_b, float* dbeta_b,
                                    int64_t M, int C, void* workspace, size_t workspace_bytes, int act_dtype, int splits,
                                    void* fin_scratch, size_t fin_scratch_bytes, void* stream) {
  BDV_REQUIRE(dout && relu_mask && ya && gamma_a && mean_a && invstd_a && dya && yb && gamma_b && mean_b && invstd_b && dyb && workspace,
              "bdv_bn_backward_pair: null pointer");
  BDV_REQUIRE_ACT(act_dtype, "bdv_bn_backward_pair");
  BDV_REQUIRE(stat_partial_a == nullptr || (stat_rows_a > 0 && bdv_aligned16(stat_partial_a)), "bdv_bn_backward_pair: bad stat_partial");
  BDV_REQUIRE(M > 0 && bn_c_ok(C) && C % 32 == 0, "bdv_bn_backward_pair: unsupported M=%lld C=%d", (long long)M, C);
  BDV_REQUIRE(act_dtype == BDV_ACT_F32 || C % 8 == 0, "bdv_bn_backward_pair: bf16 tensors need C %% 8 == 0 (16-byte units)");
  BDV_REQUIRE(bdv_aligned16(dout) && bdv_aligned16(ya) && bdv_aligned16(yb) && bdv_aligned16(dya) && bdv_aligned16(dyb) &&
                  bdv_aligned16(workspace) && bdv_aligned16(mean_a) && bdv_aligned16(invstd_a) && bdv_aligned16(mean_b) &&
                  bdv_aligned16(invstd_b), "bdv_bn_backward_pair: alignment");
  BDV_REQUIRE(dya != dyb && (const void*)dya != dout && (const void*)dyb != dout, "bdv_bn_backward_pair: dya, dyb and dout must be distinct");
  if (workspace_bytes < bdv_bn_pair_workspace_bytes(M, C)) {
    bdv_set_error("bdv_bn_backward_pair: workspace too small");
    return BDV_EWORKSPACE;
  }
  const BnGrid b = bn_grid(M, C);
  float* p1 = (float*)workspace;   // three slabs: sum g (one for both BatchNorms), sum g * xhat_a, sum g * xhat_b; then the coefficients
  float* pa2 = p1 + MAX_RB_TIMES_C;
  float* pb2 = pa2 + MAX_RB_TIMES_C;
  float* coef_a = pb2 + MAX_RB_TIMES_C;
  float* coef_b = coef_a + 3 * (size_t)C;
  const BnSums sa = bn_sums(stat_partial_a, stat_rows_a, C, p1, pa2, b.RB);
  const int Sa = bn_fin_resolve(splits, sa.rows, C, fin_scratch, fin_scratch_bytes, "bdv_bn_backward_pair");
  const int Sb = bn_fin_resolve(splits, b.RB, C, fin_scratch, fin_scratch_bytes, "bdv_bn_backward_pair");
  if (Sa < 0 || Sb < 0) return BDV_EINVAL;
  const int64_t n4 = M * C / 4;
  // the apply pass: four units per thread where the unit stride can be a multiple of the block (256) and of the channel period
  // (tools/bench_bn.py --pair, whole pair call against two bdv_bn_backward calls at the four R50 downsample blocks: one unit per
  // thread -8.7 / -7.9 / -8.7 / -4.9 %, four units per thread -9.8 / -12.5 / -20.9 / -16.2 %; the wider C, the more the ten
  // per-channel vectors per unit cost)
  const int U_ = act_dtype == BDV_ACT_BF16 ? 2 : BDV_F32_UNITS;
  const int CVU = (C / 4) / U_;
  const int L = CVU > 256 ? CVU : 256;
  const bool rows4 = (C / 4) % U_ == 0 && L % CVU == 0 && L % 256 == 0;
  const int64_t nu = n4 / U_;
  const int64_t nblk = ((nu + (int64_t)4 * L - 1) / ((int64_t)4 * L)) * (L / 256);
  BDV_REQUIRE(!rows4 || nblk < (1ll << 31), "bdv_bn_backward_pair: tensor too large");
  hipStream_t s = (hipStream_t)stream;
  if (sa.given) {  // the last main unit's sums came out of a dgrad epilogue: the downsample BatchNorm's alone
    BDV_ACT_SWITCH(act_dtype, ES, launch_bn_bwd_partial<ES>(1, b, s, dout, relu_mask, yb, mean_b, invstd_b, p1, pb2, M, C, nullptr, nullptr));
  } else {
    BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((bn_bwd_partial_pair_kernel<ES>), dim3(b.RB, b.CC), dim3(256), 0, s, dout, relu_mask, ya,
                       mean_a, invstd_a, yb, mean_b, invstd_b, p1, pa2, pb2, M, C, b.CVB, b.RL, b.rows_per_block));
  }
  BDV_LAUNCH_CHECK("bdv_bn_backward_pair(partial)");
  // the two finalizes run one after the other on the stream: they may share the scratch and the tickets
  launch_bn_bwd_finalize(sa.q1, sa.q2, sa.rows, M, C, gamma_a, invstd_a, dgamma_a, dbeta_a, 0.f, coef_a, Sa, fin_scratch, s);
  BDV_LAUNCH_CHECK("bdv_bn_backward_pair(finalize a)");
  launch_bn_bwd_finalize(p1, pb2, b.RB, M, C, gamma_b, invstd_b, dgamma_b, dbeta_b, 0.f, coef_b, Sb, fin_scratch, s);
  BDV_LAUNCH_CHECK("bdv_bn_backward_pair(finalize b)");
  const dim3 blk(256);
  const float4 *mua = (const float4*)mean_a, *isa = (const float4*)invstd_a, *ca = (const float4*)coef_a;
  const float4 *mub = (const float4*)mean_b, *isb = (const float4*)invstd_b, *cb = (const float4*)coef_b;
  BDV_ACT_SWITCH(act_dtype, ES, static_index<2>(bn_nt_enabled(), [&](auto nt) {
    constexpr bool NT = decltype(nt)::value != 0;
    if (rows4)
      hipLaunchKernelGGL((bn_bwd_apply_pair_rows_kernel<NT, ES, 4>), dim3((unsigned)nblk), blk, 0, s, dout, relu_mask, ya, mua, isa, ca, dya,
                         yb, mub, isb, cb, dyb, nu, C / 4, L);
    else
      hipLaunchKernelGGL((bn_bwd_apply_pair_kernel<NT, ES>), act_grid(n4, act_dtype), blk, 0, s, dout, relu_mask, ya, mua, isa, ca, dya, yb,
                         mub, isb, cb, dyb, n4, C / 4);
  }));
  BDV_LAUNCH_CHECK("bdv_bn_backward_pair(apply)");
  return BDV_OK;
}

extern "C" int bdv_bn_eval_backward(const void* dout, const uint32_t* relu_mask, const void* relu_act, const void* y,
                                    const float* scale, const float* running_mean, const float* invstd, void* dy, void* dz,
                                    float* dgamma, float* dbeta, float beta_acc, int64_t M, int C, void* workspace,
                                    size_t workspace_bytes, int act_dtype, int splits, void* fin_scratch, size_t fin_scratch_bytes,
                                    void* stream) {
  BDV_REQUIRE(dout && scale && dy, "bdv_bn_eval_backward: null pointer (dout, scale and dy are required)");
  BDV_REQUIRE_ACT(act_dtype, "bdv_bn_eval_backward");
  BDV_REQUIRE(M > 0 && bn_c_ok(C), "bdv_bn_eval_backward: unsupported M=%lld C=%d", (long long)M, C);
  BDV_REQUIRE(relu_mask == nullptr || relu_act == nullptr, "bdv_bn_eval_backward: one ReLU sign source at most (relu_mask or relu_act)");
  BDV_REQUIRE(relu_mask == nullptr || C % 32 == 0, "bdv_bn_eval_backward: relu_mask needs C %% 32 == 0");
  BDV_REQUIRE(act_dtype == BDV_ACT_F32 || C % 8 == 0, "bdv_bn_eval_backward: bf16 tensors need C %% 8 == 0 (16-byte units)");
  BDV_REQUIRE(bdv_aligned16(dout) && bdv_aligned16(dy) && bdv_aligned16(dz) && bdv_aligned16(relu_act) && bdv_aligned16(y) &&
                  bdv_aligned16(scale) && (((uintptr_t)relu_mask) & 3) == 0, "bdv_bn_eval_backward: alignment");
  BDV_REQUIRE(dy != dz && (const void*)dy != dout && (dz == nullptr || (const void*)dz != dout),
              "bdv_bn_eval_backward: dy, dz and dout must be distinct");
  const bool stats = dgamma != nullptr || dbeta != nullptr;
  const int sign = relu_mask != nullptr ? 1 : relu_act != nullptr ? 2 : 0;
  const bool nt = bn_nt_enabled();
  hipStream_t s = (hipStream_t)stream;
  const int row = (sign * 2 + (dz != nullptr)) * 2 + nt;   // kNumBnEvalRows
  if (!stats) {   // dy = dz * scale alone: no y, no workspace, no reduction
    const int64_t n4 = M * C / 4;
    const dim3 grid = act_grid(n4, act_dtype), blk(256);
    BDV_ACT_SWITCH(act_dtype, ES, static_index<kNumBnEvalRows>(row, [&](auto ri) {
      constexpr int I = decltype(ri)::value;
      hipLaunchKernelGGL((bn_eval_bwd_kernel<I / 4, (I / 2) % 2 != 0, I % 2 != 0, ES>), grid, blk, 0, s, dout, relu_mask, relu_act,
                         (const float4*)scale, dy, dz, n4, C / 4);
    }));
    BDV_LAUNCH_CHECK("bdv_bn_eval_backward");
    return BDV_OK;
  }
  BDV_REQUIRE(y && running_mean && invstd && workspace, "bdv_bn_eval_backward: dgamma / dbeta need y, running_mean, invstd and a workspace");
  BDV_REQUIRE(bdv_aligned16(running_mean) && bdv_aligned16(invstd) && bdv_aligned16(workspace), "bdv_bn_eval_backward: alignment");
  BDV_REQUIRE((const void*)dy != y && (dz == nullptr || (const void*)dz != y), "bdv_bn_eval_backward: dy / dz must not alias y");
  BnWs w;
  if (int e = bn_ws_carve(workspace, workspace_bytes, C, "bdv_bn_eval_backward", &w)) return e;
  const BnGrid b = bn_grid(M, C);
  const int S = bn_fin_resolve(splits, b.RB, C, fin_scratch, fin_scratch_bytes, "bdv_bn_eval_backward");
  if (S < 0) return BDV_EINVAL;
  BDV_ACT_SWITCH(act_dtype, ES, static_index<kNumBnEvalRows>(row, [&](auto ri) {
    constexpr int I = decltype(ri)::value;
    hipLaunchKernelGGL((bn_eval_bwd_stats_kernel<I / 4, (I / 2) % 2 != 0, I % 2 != 0, ES>), dim3(b.RB, b.CC), dim3(256), 0, s, dout,
                       relu_mask, relu_act, y, scale, running_mean, invstd, dy, dz, w.p1, w.p2, M, C, b.CVB, b.RL, b.rows_per_block);
  }));
  BDV_LAUNCH_CHECK("bdv_bn_eval_backward(pass)");
  // the train-mode finalize: fixed-order fp64 column sums -> dgamma / dbeta (beta_acc as bdv_bn_backward).  Its apply coefficients
  // go to the workspace unread; `scale` stands in for the gamma they are formed from.
  launch_bn_bwd_finalize(w.p1, w.p2, b.RB, M, C, scale, invstd, dgamma, dbeta, beta_acc, w.coef, S, fin_scratch, s);
  BDV_LAUNCH_CHECK("bdv_bn_eval_backward(finalize)");
  return BDV_OK;
}

extern "C" int bdv_bn_backward_maxpool_split(const void* dpool, const uint8_t* pool_idx, const uint32_t* relu_mask, const float* y,
                                             const float* gamma, const float* save_mean, const float* save_invstd, float* dy,
                                             float* dgamma, float* dbeta, float beta_acc, int N, int H, int W, int C, void* workspace,
                                             size_t workspace_bytes, int dpool_dtype, int splits, void* fin_scratch,
                                             size_t fin_scratch_bytes, void* stream) {
  BDV_REQUIRE(dpool && pool_idx && relu_mask && y && gamma && save_mean && save_invstd && dy && workspace,
              "bdv_bn_backward_maxpool: null pointer");
  BDV_REQUIRE_ACT(dpool_dtype, "bdv_bn_backward_maxpool");
  BDV_REQUIRE(N > 0 && H > 1 && W > 1 && C >= 32 && C % 32 == 0 && 256 % (C / 4) == 0,
              "bdv_bn_backward_maxpool: unsupported shape (C must be 32, 64, 128, 256, 512 or 1024)");
  BDV_REQUIRE(bdv_aligned16(dpool) && bdv_aligned16(y) && bdv_aligned16(dy) && bdv_aligned16(workspace) &&
                  bdv_aligned16(save_mean) && bdv_aligned16(save_invstd) && (((uintptr_t)pool_idx) & 3) == 0,
              "bdv_bn_backward_maxpool: alignment");
  const int64_t M = (int64_t)N * H * W;
  BDV_REQUIRE(M * (C / 4) < (1ll << 31), "bdv_bn_backward_maxpool: tensor too large");
  BnWs w;
  if (int e = bn_ws_carve(workspace, workspace_bytes, C, "bdv_bn_backward_maxpool", &w)) return e;
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1, CV = C / 4;
  const int gx = (Wo * CV + 255) / 256;
  int gy = N * Ho;
  const int cap = MAX_RB_TIMES_C / C / gx;  // slab rows = gx * gy
  if (gy > cap) gy = cap;
  if (gy > 4096) gy = 4096;
  BDV_REQUIRE(gy >= 1, "bdv_bn_backward_maxpool: row too wide for the partial slab");
  const int S = bn_fin_resolve(splits, gx * gy, C, fin_scratch, fin_scratch_bytes, "bdv_bn_backward_maxpool");
  if (S < 0) return BDV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(gx, gy), blk(256);
  auto pass = [&](auto apply) {   // statistics (coef and dy unused) or apply (p1 and p2 unused)
    constexpr bool APPLY = decltype(apply)::value;
    BDV_ACT_SWITCH(dpool_dtype, ES, hipLaunchKernelGGL((bn_bwd_pool_kernel<APPLY, ES>), grid, blk, 0, s, dpool, (const uchar4*)pool_idx,
                       relu_mask, (const float4*)y, (const float4*)save_mean, (const float4*)save_invstd,
                       APPLY ? (const float4*)w.coef : nullptr, APPLY ? (float4*)dy : nullptr, APPLY ? nullptr : w.p1,
                       APPLY ? nullptr : w.p2, N, H, W, CV, Ho, Wo));
  };
  pass(std::false_type{});
  BDV_LAUNCH_CHECK("bdv_bn_backward_maxpool(partial)");
  launch_bn_bwd_finalize(w.p1, w.p2, gx * gy, M, C, gamma, save_invstd, dgamma, dbeta, beta_acc, w.coef, S, fin_scratch, s);
  BDV_LAUNCH_CHECK("bdv_bn_backward_maxpool(finalize)");
  pass(std::true_type{});
  BDV_LAUNCH_CHECK("bdv_bn_backward_maxpool(apply)");
  return BDV_OK;
}

extern "C" int bdv_bn_backward_maxpool(const void* dpool, const uint8_t* pool_idx, const uint32_t* relu_mask, const float* y,
                                       const float* gamma, const float* save_mean, const float* save_invstd, float* dy,
                                       float* dgamma, float* dbeta, float beta_acc, int N, int H, int W, int C, void* workspace,
                                       size_t workspace_bytes, int dpool_dtype, void* stream) {
  return bdv_bn_backward_maxpool_split(dpool, pool_idx, relu_mask, y, gamma, save_mean, save_invstd, dy, dgamma, dbeta, beta_acc, N, H, W,
                                       C, workspace, workspace_bytes, dpool_dtype, 1, nullptr, 0, stream);
}

extern "C" int bdv_relu_bwd(const void* dout, const uint32_t* relu_mask, const void* add, void* g, int64_t numel, int act_dtype,
                            void* stream) {
  BDV_REQUIRE(dout && relu_mask && g && numel > 0 && numel % 32 == 0, "bdv_relu_bwd: bad argument");
  BDV_REQUIRE_ACT(act_dtype, "bdv_relu_bwd");
  BDV_REQUIRE(bdv_aligned16(dout) && bdv_aligned16(g) && (!add || bdv_aligned16(add)), "bdv_relu_bwd: alignment");
  const int64_t n4 = numel / 4;
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((relu_bwd_kernel<ES>), dim3(bdv_ew_grid(n4)), dim3(256), 0, (hipStream_t)stream, dout,
                     relu_mask, add, g, n4));
  BDV_LAUNCH_CHECK("bdv_relu_bwd");
  return BDV_OK;
}

extern "C" int bdv_add(const void* a, const void* b, void* out, int64_t numel, int act_dtype, void* stream) {
  BDV_REQUIRE(a && b && out && numel > 0 && numel % 4 == 0, "bdv_add: bad argument");
  BDV_REQUIRE_ACT(act_dtype, "bdv_add");
  BDV_REQUIRE(bdv_aligned16(a) && bdv_aligned16(b) && bdv_aligned16(out), "bdv_add: alignment");
  const int64_t n4 = numel / 4;
  BDV_ACT_SWITCH(act_dtype, ES, hipLaunchKernelGGL((add_kernel<ES>), dim3(bdv_ew_grid(n4)), dim3(256), 0, (hipStream_t)stream, a, b, out, n4));
  BDV_LAUNCH_CHECK("bdv_add");
  return BDV_OK;
}
