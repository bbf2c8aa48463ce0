// fp32 GEMM out of TWO fp16 pieces per operand ("f16x2"): each operand is multiplied by a power of two that
// puts its largest entry into [2^14, 2^15), cut into hi = f16(x) and lo = f16(x - hi) (round to nearest even), and C = A * B^T is
// accumulated in fp32 from hi*hi + hi*lo + lo*hi with v_mfma_f32_32x32x16_f16, then multiplied by 1 / (S_a * S_b).
// Reports
//   1. the issue rate of v_mfma_f32_32x32x16_f16 beside v_mfma_f32_32x32x16_bf16, from the in-kernel clock (cycles per MFMA of one
//      wave with four independent accumulators) and from the wall time of a grid that fills the machine;
//   2. whether the MFMA honours fp16 SUBNORMAL A / B inputs (the low piece of an entry more than ~2^14 below the tensor's maximum
//      is subnormal): a product of a subnormal and a normal number, exact in fp32, against zero;
//   3. the GEMM's rate in fp32-equivalent TFLOP/s and its error against an fp64 reference on sampled rows, next to a plain fp32
//      FMA chain over the same rows, for well-scaled operands and for rows 2^-12 .. 2^-26 below the tensor's maximum.
// Both operands are K-contiguous ([M][K] and [N][K]) and pre-split; block tile 128 x 128, 4 waves (2 x 2), BK = 32, one LDS stage
// (the loop of gemm_bf16x3.hip with two planes).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int BK = 32;
constexpr int LDK = BK + 8;  // row pitch in halves: 80 bytes, keeps the 16-byte fragment reads of 8 rows on distinct banks

#define CHECK(x)                                                                      \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));       \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

// ---- 1. MFMA rate -------------------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void mfma_rate_kernel(float* __restrict__ out, long long* __restrict__ cycles, int iters) {
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  f16x8 ah, bh;
  bf16x8 ab, bb;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ah[e] = (_Float16)(0.001f * (float)((int)(threadIdx.x & 63) + e));
    bh[e] = (_Float16)(0.002f * (float)((int)(threadIdx.x & 63) - e));
    ab[e] = (__bf16)(0.001f * (float)((int)(threadIdx.x & 63) + e));
    bb[e] = (__bf16)(0.002f * (float)((int)(threadIdx.x & 63) - e));
  }
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (F16) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[j], 0, 0, 0);
      else acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ab, bb, acc[j], 0, 0, 0);
    }
  }
  const long long t1 = clock64();
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[j][e];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
}

template <bool F16>
static void mfma_rate(const char* name) {
  const int blocks = 256 * 2, iters = 20000;     // four waves per block, one per SIMD; two blocks per CU
  float* out;
  long long* cyc;
  CHECK(hipMalloc(&out, (size_t)blocks * 256 * sizeof(float)));
  CHECK(hipMalloc(&cyc, (size_t)blocks * sizeof(long long)));
  hipLaunchKernelGGL(mfma_rate_kernel<F16>, dim3(blocks), dim3(256), 0, 0, out, cyc, 100);
  CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(mfma_rate_kernel<F16>, dim3(blocks), dim3(256), 0, 0, out, cyc, iters);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  long long h[8];
  CHECK(hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost));
  const double flop = 2.0 * 32 * 32 * 16 * 4.0 * iters * 4.0 * blocks;
  printf("%-34s %6.2f clock64 ticks per MFMA of a wave (two waves per SIMD: half of it each)  %7.1f TFLOP/s over %d workgroups (%.3f ms)\n",
         name, (double)h[0] / (4.0 * iters), flop / ms / 1e9, blocks, ms);
  CHECK(hipFree(out));
  CHECK(hipFree(cyc));
}

// ---- 2. fp16 subnormal inputs ---------------------------------------------------------------------------------------------------
// A[row][k] = a for k = 0 (else 0), B[col][k] = b for k = 0: every C element = a * b.  One wave.
__global__ __launch_bounds__(64) void subnormal_kernel(float* __restrict__ out, const u16* __restrict__ ab) {
  f16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = b[e] = (_Float16)0.f;
  if ((threadIdx.x >> 5) == 0) {      // lanes 0..31 hold k = 0..7 of the 16-deep step
    a[0] = __builtin_bit_cast(_Float16, ab[0]);
    b[0] = __builtin_bit_cast(_Float16, ab[1]);
  }
  f32x16 c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  out[threadIdx.x] = c[0];
}

static float subnormal_probe(u16 a_bits, u16 b_bits) {
  u16 h[2] = {a_bits, b_bits};
  u16* d;
  float* out;
  CHECK(hipMalloc(&d, sizeof(h)));
  CHECK(hipMalloc(&out, 64 * sizeof(float)));
  CHECK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(subnormal_kernel, dim3(1), dim3(64), 0, 0, out, d);
  float r[64];
  CHECK(hipMemcpy(r, out, sizeof(r), hipMemcpyDeviceToHost));
  CHECK(hipFree(d));
  CHECK(hipFree(out));
  return r[0];
}

// ---- 3. the GEMM ------------------------------------------------------------------------------------------------------------------
// planes[0 | 1][rows][K] = hi | lo of x * scale
__global__ void split2_kernel(const float* __restrict__ x, u16* __restrict__ planes, size_t n, float scale) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = x[i] * scale;
  const _Float16 hi = (_Float16)a;
  const _Float16 lo = (_Float16)(a - (float)hi);
  planes[i] = __builtin_bit_cast(u16, hi);
  planes[n + i] = __builtin_bit_cast(u16, lo);
}

template <int BM, int BN>
__global__ __launch_bounds__(256) void gemm_f16x2_kernel(const u16* __restrict__ A, const u16* __restrict__ B, float* __restrict__ C, int M, int N,
                                                         int K, float unscale) {
  constexpr int NT = 256, WM = 2, WN = 2;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int AV = BM * BK / 8 / NT, BV = BN * BK / 8 / NT;  // 16-byte vectors per thread per plane
  __shared__ __attribute__((aligned(16))) u16 As[2][BM * LDK];
  __shared__ __attribute__((aligned(16))) u16 Bs[2][BN * LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int nbn = N / BN;
  const int bm = blockIdx.x / nbn, bn = blockIdx.x - bm * nbn;
  const size_t planeA = (size_t)M * K, planeB = (size_t)N * K;
  const int r = lane & 31, h = lane >> 5;
  u32x4 ra[2 * AV], rb[2 * BV];
  auto gload = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const int idx = tid + NT * v, row = idx >> 2, kv = idx & 3;
        ra[p * AV + v] = *reinterpret_cast<const u32x4*>(A + p * planeA + (size_t)(bm * BM + row) * K + kt * BK + 8 * kv);
      }
#pragma unroll
      for (int v = 0; v < BV; ++v) {
        const int idx = tid + NT * v, row = idx >> 2, kv = idx & 3;
        rb[p * BV + v] = *reinterpret_cast<const u32x4*>(B + p * planeB + (size_t)(bn * BN + row) * K + kt * BK + 8 * kv);
      }
    }
  };
  auto sstore = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int v = 0; v < AV; ++v) {
        const int idx = tid + NT * v, row = idx >> 2, kv = idx & 3;
        *reinterpret_cast<u32x4*>(&As[p][row * LDK + 8 * kv]) = ra[p * AV + v];
      }
#pragma unroll
      for (int v = 0; v < BV; ++v) {
        const int idx = tid + NT * v, row = idx >> 2, kv = idx & 3;
        *reinterpret_cast<u32x4*>(&Bs[p][row * LDK + 8 * kv]) = rb[p * BV + v];
      }
    }
  };
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nk = K / BK;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
    sstore();
    __syncthreads();
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      f16x8 a[2][TM], b[2][TN];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
          a[p][i] = *reinterpret_cast<const f16x8*>(&As[p][(wm * (BM / WM) + 32 * i + r) * LDK + 16 * s + 8 * h]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          b[p][j] = *reinterpret_cast<const f16x8*>(&Bs[p][(wn * (BN / WN) + 32 * j + r) * LDK + 16 * s + 8 * h]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {  // smallest terms first
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][i], b[1][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[1][i], b[0][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0][i], b[0][j], acc[i][j], 0, 0, 0);
        }
    }
  }
  // C/D layout of the 32x32 MFMAs: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = bm * BM + wm * (BM / WM) + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int col = bn * BN + wn * (BN / WN) + 32 * j + r;
        C[(size_t)row * N + col] = acc[i][j][e] * unscale;
      }
}

static float pow2_scale(const float* x, size_t n) {  // 2^(14 - floor(log2 max|x|)); 1 for an all-zero tensor
  float m = 0.f;
  for (size_t i = 0; i < n; ++i) m = fmaxf(m, fabsf(x[i]));
  if (m == 0.f) return 1.f;
  int ex;
  frexpf(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
  return ldexpf(1.f, 14 - (ex - 1));
}

// weak_rows: rows 8 q + 5 of A are scaled by 2^-(12 + 2 q') so that they lie below the fp16-normal range after scaling
static void gemm_case(const char* name, int M, int N, int K, bool weak_rows) {
  float* hA = (float*)malloc((size_t)M * K * 4);
  float* hB = (float*)malloc((size_t)N * K * 4);
  srand(1);
  for (size_t i = 0; i < (size_t)M * K; ++i) hA[i] = (float)rand() / RAND_MAX * 2.f - 1.f;
  for (size_t i = 0; i < (size_t)N * K; ++i) hB[i] = ((float)rand() / RAND_MAX * 2.f - 1.f) * 0.05f;
  const int nrows = 8;
  int rows[nrows];
  for (int q = 0; q < nrows; ++q) rows[q] = (int)(((long long)q * 1237 + 5) % M);
  if (weak_rows)
    for (int q = 0; q < nrows; ++q)
      for (int k = 0; k < K; ++k) hA[(size_t)rows[q] * K + k] = ldexpf(hA[(size_t)rows[q] * K + k], -(12 + 2 * q));
  double* ref = (double*)malloc((size_t)nrows * N * sizeof(double));
  double* f32c = (double*)malloc((size_t)nrows * N * sizeof(double));
  double scale = 0;
  for (int q = 0; q < nrows; ++q)
    for (int n = 0; n < N; ++n) {
      double s = 0;
      float f = 0.f;
      for (int k = 0; k < K; ++k) {
        s += (double)hA[(size_t)rows[q] * K + k] * (double)hB[(size_t)n * K + k];
        f = fmaf(hA[(size_t)rows[q] * K + k], hB[(size_t)n * K + k], f);
      }
      ref[(size_t)q * N + n] = s;
      f32c[(size_t)q * N + n] = (double)f;
      scale = fmax(scale, fabs(s));
    }
  const float sa = pow2_scale(hA, (size_t)M * K), sb = pow2_scale(hB, (size_t)N * K);
  float *dA32, *dB32, *dC;
  u16 *dA, *dB;
  CHECK(hipMalloc(&dA32, (size_t)M * K * 4));
  CHECK(hipMalloc(&dB32, (size_t)N * K * 4));
  CHECK(hipMalloc(&dA, (size_t)M * K * 4));
  CHECK(hipMalloc(&dB, (size_t)N * K * 4));
  CHECK(hipMalloc(&dC, (size_t)M * N * 4));
  CHECK(hipMemcpy(dA32, hA, (size_t)M * K * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dB32, hB, (size_t)N * K * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(split2_kernel, dim3((unsigned)(((size_t)M * K + 255) / 256)), dim3(256), 0, 0, dA32, dA, (size_t)M * K, sa);
  hipLaunchKernelGGL(split2_kernel, dim3((unsigned)(((size_t)N * K + 255) / 256)), dim3(256), 0, 0, dB32, dB, (size_t)N * K, sb);
  CHECK(hipDeviceSynchronize());
  const dim3 grid((M / 128) * (N / 128));
  const float unscale = 1.f / (sa * sb);
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL((gemm_f16x2_kernel<128, 128>), grid, dim3(256), 0, 0, dA, dB, dC, M, N, K, unscale);
  CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int iters = 20;
  CHECK(hipEventRecord(e0));
  for (int i = 0; i < iters; ++i) hipLaunchKernelGGL((gemm_f16x2_kernel<128, 128>), grid, dim3(256), 0, 0, dA, dB, dC, M, N, K, unscale);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  ms /= iters;
  float* hC = (float*)malloc((size_t)N * sizeof(float));
  printf("%s: %dx%dx%d  S_a = 2^%d  S_b = 2^%d  %7.3f ms  %7.1f TFLOP/s (fp32-equivalent)\n", name, M, N, K, ilogbf(sa), ilogbf(sb), ms,
         2.0 * M * N * K / ms / 1e9);
  double max16 = 0, max32 = 0;
  for (int q = 0; q < nrows; ++q) {
    CHECK(hipMemcpy(hC, dC + (size_t)rows[q] * N, N * sizeof(float), hipMemcpyDeviceToHost));
    double rs = 0, r16 = 0, r32 = 0;
    for (int n = 0; n < N; ++n) {
      rs = fmax(rs, fabs(ref[(size_t)q * N + n]));
      r16 = fmax(r16, fabs((double)hC[n] - ref[(size_t)q * N + n]));
      r32 = fmax(r32, fabs(f32c[(size_t)q * N + n] - ref[(size_t)q * N + n]));
    }
    max16 = fmax(max16, r16);
    max32 = fmax(max32, r32);
    if (weak_rows)
      printf("  row 2^-%d below the maximum: max err / max|row of C|  f16x2 %.3e   fp32 FMA chain %.3e\n", 12 + 2 * q, r16 / rs, r32 / rs);
  }
  printf("  max err / max|C| over the sampled rows:  f16x2 %.3e   fp32 FMA chain %.3e\n", max16 / scale, max32 / scale);
  free(hA); free(hB); free(ref); free(f32c); free(hC);
  CHECK(hipFree(dA32)); CHECK(hipFree(dB32)); CHECK(hipFree(dA)); CHECK(hipFree(dB)); CHECK(hipFree(dC));
}

int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 8192, N = argc > 2 ? atoi(argv[2]) : 4096, K = argc > 3 ? atoi(argv[3]) : 2304;
  if (M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % BK) {
    fprintf(stderr, "M, N multiples of 128 and K a multiple of 32\n");
    return 1;
  }
  mfma_rate<true>("v_mfma_f32_32x32x16_f16");
  mfma_rate<false>("v_mfma_f32_32x32x16_bf16");
  // 0x0001 = 2^-24 (the smallest subnormal), 0x0200 = 2^-15, 0x6400 = 2^10, 0x3c00 = 1
  struct { u16 a, b; double want; const char* what; } probes[] = {
      {0x0200, 0x6400, ldexp(1.0, -5), "A = 2^-15 (subnormal) x B = 2^10"},
      {0x6400, 0x0200, ldexp(1.0, -5), "A = 2^10 x B = 2^-15 (subnormal)"},
      {0x0001, 0x3c00, ldexp(1.0, -24), "A = 2^-24 (smallest subnormal) x B = 1"},
      {0x0001, 0x0001, ldexp(1.0, -48), "A = 2^-24 x B = 2^-24 (both subnormal)"},
  };
  bool honoured = true;
  for (auto& p : probes) {
    const float got = subnormal_probe(p.a, p.b);
    printf("fp16 subnormal input: %-42s -> %.6e (exact product %.6e)%s\n", p.what, (double)got, p.want, (double)got == p.want ? "" : "  FLUSHED");
    honoured = honoured && (double)got == p.want;
  }
  printf("v_mfma_f32_32x32x16_f16 %s fp16 subnormal A / B inputs\n", honoured ? "HONOURS" : "FLUSHES");
  gemm_case("f16x2, 3 products, 128x128", M, N, K, false);
  gemm_case("f16x2, 3 products, 128x128, weak rows", M, N, K, true);
  return 0;
}
