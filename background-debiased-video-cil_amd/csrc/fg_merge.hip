// Foreground merging after FAME (Ding et al., "Motion-aware Contrastive Video Representation Learning via Foreground-background
// Merging", CVPR 2022) -- BEYOND THE REFERENCE: the reference has no such augmentation, and the upstream FAME code is not vendored,
// so the definition is the one of DESIGN.md 4.11 (parity unpinned).  A foreground mask per clip from the clip itself (frame
// differences, blurred, refined by a colour histogram), then every background pixel of clip b takes the pixel of clip perm[b]:
//   bdv_fg_motion_q      stages 1-3: motion map d, separable Gaussian blur g, per-clip min/max, 8-bit quantised map q
//   bdv_fg_hist_refine   stages 4-5: per-clip colour histograms F (sum of q) and N (count), uint32; refined map s
//   bdv_fg_select        stage 6:    exact k-th largest value of s per clip (radix select on the float bits), mask and count
//   bdv_fg_merge         stage 7:    in-place merge, gather-then-assign for any index vector
// Everything is fp32 with sums in the stated order; built with -ffp-contract=off so every product and sum is rounded on its own,
// which is what the torch restatement (tests/fg_merge_oracle.py) computes.  The histograms are integer atomics (LDS partials per
// workgroup, then one global add per non-empty bin), hence independent of arrival order.
//
// Layouts (BDV_FG_*): a clip is T frames of 3 colour planes over H*W pixels.  TCHW (B,T,3,H,W), CTHW (B,3,T,H,W) are planar, THWC4
// is the NHWC4 frames tensor (B*T,H,W,4) whose fourth lane takes no part in the mask and moves with its pixel in the merge.
//
// Addressing.  The passes that read the clip give a thread four pixels: four consecutive ones in the planar layouts (one ld4_any
// per plane: a 16-byte, two 8-byte or four 4-byte loads, whichever the plane's address allows -- a sample with odd H*W puts its
// planes at every 4-byte phase), four pixels 256 apart in NHWC4 (one 16-byte load each, consecutive lanes on consecutive pixels).
// The merge lays 16-byte units on the grid of the DESTINATION address, as blend.hip does, so every wide store is aligned.
#include "common.h"
#include "loader_pieces.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                        // pixels per thread in the clip-reading passes
constexpr int kBlockPix = kThreads * kPix;     // pixels per workgroup there
constexpr int kMaxTaps = 129;
constexpr int kMaxBins = 16 * 16 * 16;
constexpr int kSelThreads = 1024;

struct Clip {
  int64_t S, tstride, cstride;      // floats per sample, per frame step, per channel step
  int T, HW, inner;                 // inner: floats per pixel step (1 planar, 4 NHWC4)
};

struct Taps {
  float w[kMaxTaps];
};

struct Colour {
  float lo[3], s[3];
};

// pixel j (0..3) of this thread inside its workgroup's run of kBlockPix pixels
template <int INNER>
__device__ __forceinline__ int pix_of(int j) {
  return INNER == 1 ? (int)blockIdx.x * kBlockPix + (int)threadIdx.x * kPix + j : (int)blockIdx.x * kBlockPix + (int)threadIdx.x + kThreads * j;
}

// the three colours of this thread's four pixels of the frame at fp; pixels past HW read as 0
template <int INNER>
__device__ __forceinline__ void load_px(const float* __restrict__ fp, const Clip& g, float (&v)[3][kPix]) {
  if constexpr (INNER == 1) {
    const int p0 = pix_of<1>(0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* plane = fp + c * g.cstride;
      if (p0 + kPix <= g.HW) {
        const float4 a = ld4_any(plane + p0);
        v[c][0] = a.x, v[c][1] = a.y, v[c][2] = a.z, v[c][3] = a.w;
      } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j) v[c][j] = p0 + j < g.HW ? plane[p0 + j] : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int p = pix_of<4>(j);
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p < g.HW) a = ld4_any(fp + (int64_t)p * 4);
      v[0][j] = a.x, v[1][j] = a.y, v[2][j] = a.z;
    }
  }
}

// ---- stage 1: d[b,p] = (sum_t sum_c |x[t+1] - x[t]|) / (T - 1), one accumulator per pixel, t outer, c inner ------------------------
template <int INNER>
__global__ __launch_bounds__(kThreads) void fg_motion_kernel(const float* __restrict__ x, float* __restrict__ d, Clip g) {
  const int b = blockIdx.y;
  const float* xb = x + (int64_t)b * g.S;
  float prev[3][kPix], cur[3][kPix], acc[kPix] = {0.f, 0.f, 0.f, 0.f};
  load_px<INNER>(xb, g, prev);
  for (int t = 1; t < g.T; ++t) {
    load_px<INNER>(xb + (int64_t)t * g.tstride, g, cur);
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc[j] = acc[j] + fabsf(cur[c][j] - prev[c][j]);
        prev[c][j] = cur[c][j];
      }
    }
  }
  const float den = (float)(g.T - 1);
  float* db = d + (int64_t)b * g.HW;
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int p = pix_of<INNER>(j);
    if (p < g.HW) db[p] = acc[j] / den;
  }
}

// ---- stage 2: separable Gaussian, reflect border (edge not repeated), taps in ascending order -----------------------------------
__device__ __forceinline__ int reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// min and max of 32-bit keys over a workgroup of kThreads (non-negative floats order as their bits); every thread gets the result
__device__ __forceinline__ void block_minmax(uint32_t& lo, uint32_t& hi) {
  __shared__ uint32_t slo[kThreads / 64], shi[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo, hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) slo[threadIdx.x >> 6] = lo, shi[threadIdx.x >> 6] = hi;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    lo = slo[w] < lo ? slo[w] : lo, hi = shi[w] > hi ? shi[w] : hi;
  }
}

// ALONG_W: out[b,h,w] = sum_j w[j] * in[b,h,reflect(w+j-r)]; !ALONG_W: the same along h, and the workgroup's min / max of the result
// go to part[b][blockIdx.x] = {min bits, max bits}.  No atomics: 784 adds per clip onto one word cost 17 x the blur itself.
template <bool ALONG_W>
__global__ __launch_bounds__(kThreads) void fg_blur_kernel(const float* __restrict__ in, float* __restrict__ out, uint32_t* __restrict__ part,
                                                           int H, int W, int k, Taps taps) {
  const int b = blockIdx.y, HW = H * W;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t lo = 0xffffffffu, hi = 0u;
  if (p < HW) {
    const float* src = in + (int64_t)b * HW;
    const int h = p / W, w = p - h * W, r = k >> 1;
    float acc = 0.f;
    for (int j = 0; j < k; ++j) {
      const float v = ALONG_W ? src[h * W + reflect(w + j - r, W)] : src[reflect(h + j - r, H) * W + w];
      acc = acc + taps.w[j] * v;      // no contraction in this file
    }
    out[(int64_t)b * HW + p] = acc;
    lo = hi = __float_as_uint(acc);
  }
  if (!ALONG_W) {
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
      uint32_t* dst = part + 2 * ((int64_t)b * gridDim.x + blockIdx.x);
      dst[0] = lo, dst[1] = hi;
    }
  }
}

// ---- stage 3: q = (uint8)floor(255 * (g - lo) / (hi - lo + 1e-8f) + 0.5), 0 everywhere when hi == lo --------------------------------
// every workgroup reduces the clip's partial pairs itself (a few hundred words out of L2); the first one records mm[b] = {lo, hi}
__global__ __launch_bounds__(kThreads) void fg_quant_kernel(const float* __restrict__ gmap, const uint32_t* __restrict__ part, uint32_t* __restrict__ mm,
                                                            uint8_t* __restrict__ q, int HW) {
  const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t ulo = 0xffffffffu, uhi = 0u;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += kThreads) {
    const uint32_t l2 = part[2 * ((int64_t)b * gridDim.x + i)], h2 = part[2 * ((int64_t)b * gridDim.x + i) + 1];
    ulo = l2 < ulo ? l2 : ulo, uhi = h2 > uhi ? h2 : uhi;
  }
  block_minmax(ulo, uhi);
  if (blockIdx.x == 0 && threadIdx.x == 0) mm[2 * b] = ulo, mm[2 * b + 1] = uhi;
  if (p >= HW) return;
  const float lo = __uint_as_float(ulo), hi = __uint_as_float(uhi);
  float v = 0.f;
  if (hi != lo) {
    const float m = (gmap[(int64_t)b * HW + p] - lo) / ((hi - lo) + 1e-8f);
    v = floorf(255.0f * m + 0.5f);
  }
  q[(int64_t)b * HW + p] = v >= 1.f ? (v >= 255.f ? (uint8_t)255 : (uint8_t)(int)v) : (uint8_t)0;      // a NaN gives 0
}

// ---- stage 4: colour histograms ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int colour_bin(float x, float lo, float s, int n) {
  const float v = floorf((x - lo) * s);
  return v >= 1.f ? (v >= (float)(n - 1) ? n - 1 : (int)v) : 0;      // a NaN falls into bin 0
}

// F[b,i] += q, N[b,i] += 1 for every pixel of every frame; the bin index goes to idx (B, T, HWp) as 16 bits for stage 5
template <int INNER>
__global__ __launch_bounds__(kThreads) void fg_hist_kernel(const float* __restrict__ x, const uint8_t* __restrict__ q, uint16_t* __restrict__ idx,
                                                           uint32_t* __restrict__ F, uint32_t* __restrict__ N, Clip g, int n, Colour col,
                                                           int HWp) {
  __shared__ uint32_t sF[kMaxBins], sN[kMaxBins];
  const int b = blockIdx.y, nb = n * n * n;
  for (int i = threadIdx.x; i < nb; i += kThreads) sF[i] = 0u, sN[i] = 0u;
  __syncthreads();
  uint32_t qv[kPix];
  bool ok[kPix];
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int p = pix_of<INNER>(j);
    ok[j] = p < g.HW;
    qv[j] = ok[j] ? q[(int64_t)b * g.HW + p] : 0u;
  }
  const float* xb = x + (int64_t)b * g.S;
  float v[3][kPix];
  for (int t = 0; t < g.T; ++t) {
    load_px<INNER>(xb + (int64_t)t * g.tstride, g, v);
    uint16_t* row = idx + ((int64_t)b * g.T + t) * HWp;
    int bin[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int b0 = colour_bin(v[0][j], col.lo[0], col.s[0], n), b1 = colour_bin(v[1][j], col.lo[1], col.s[1], n),
                b2 = colour_bin(v[2][j], col.lo[2], col.s[2], n);
      bin[j] = (b0 * n + b1) * n + b2;
      if (ok[j]) {
        atomicAdd(&sF[bin[j]], qv[j]);
        atomicAdd(&sN[bin[j]], 1u);
      }
    }
    if (INNER == 1 && ok[kPix - 1]) {      // four consecutive pixels from a multiple of 4, HWp a multiple of 4: an aligned 8-byte store
      *reinterpret_cast<ushort4*>(row + pix_of<1>(0)) = make_ushort4((uint16_t)bin[0], (uint16_t)bin[1], (uint16_t)bin[2], (uint16_t)bin[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPix; ++j)
        if (ok[j]) row[pix_of<INNER>(j)] = (uint16_t)bin[j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    const uint32_t cn = sN[i], cf = sF[i];
    if (cn) atomicAdd(&N[(int64_t)b * nb + i], cn);
    if (cf) atomicAdd(&F[(int64_t)b * nb + i], cf);
  }
}

// ---- stage 5: s[b,p] = (sum_t F[i_t] / (255 * N[i_t])) / T, t ascending ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fg_refine_kernel(const uint16_t* __restrict__ idx, const uint32_t* __restrict__ F,
                                                             const uint32_t* __restrict__ N, float* __restrict__ s, int T, int HW, int HWp, int nb) {
  __shared__ float ratio[kMaxBins];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    const uint32_t cn = N[(int64_t)b * nb + i];
    ratio[i] = cn ? (float)F[(int64_t)b * nb + i] / (255.0f * (float)cn) : 0.f;
  }
  __syncthreads();
  const int p0 = (blockIdx.x * kThreads + threadIdx.x) * kPix;
  if (p0 >= HW) return;
  const bool full = p0 + kPix <= HW;
  float acc[kPix] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; ++t) {
    const uint16_t* row = idx + ((int64_t)b * T + t) * HWp + p0;
    uint16_t i4[kPix] = {0, 0, 0, 0};
    if (full) {
      const ushort4 u = *reinterpret_cast<const ushort4*>(row);
      i4[0] = u.x, i4[1] = u.y, i4[2] = u.z, i4[3] = u.w;
    } else {
#pragma unroll
      for (int j = 0; j < kPix; ++j)
        if (p0 + j < HW) i4[j] = row[j];
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) acc[j] = acc[j] + ratio[i4[j] < nb ? i4[j] : nb - 1];
  }
  const float den = (float)T;
#pragma unroll
  for (int j = 0; j < kPix; ++j)
    if (p0 + j < HW) s[(int64_t)b * HW + p0 + j] = acc[j] / den;
}

// ---- stage 6: exact selection, one workgroup per clip --------------------------------------------------------------------------
// key: the bits of a non-negative float order as the float; a negative value (none is ever produced by stage 5) counts as zero
__device__ __forceinline__ uint32_t sel_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? 0u : u;
}

// Radix select, most significant byte first: after four passes `prefix` is the key of the kfg-th largest value.  A wave counts into
// a histogram of its own, so an LDS add never waits on more than the 64 lanes of one instruction.
__global__ __launch_bounds__(kSelThreads) void fg_select_kernel(const float* __restrict__ s, int HW, int kfg, float* __restrict__ v,
                                                                uint8_t* __restrict__ mask, int32_t* __restrict__ count) {
  constexpr int kWaves = kSelThreads / 64;
  __shared__ uint32_t hist[kWaves][256];
  __shared__ uint32_t sh_prefix, sh_k, sh_count;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const float* sb = s + (int64_t)b * HW;
  if (tid == 0) sh_prefix = 0u, sh_k = (uint32_t)kfg, sh_count = 0u;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < kWaves * 256; i += kSelThreads) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t prefix = sh_prefix;
    for (int i = tid; i < HW; i += kSelThreads) {
      const uint32_t key = sel_key(sb[i]);
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[wave][(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 256) {
      uint32_t c = 0;
#pragma unroll
      for (int wv = 0; wv < kWaves; ++wv) c += hist[wv][tid];
      hist[0][tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t k = sh_k, cum = 0;
      int d = 255;
      for (; d > 0; --d) {
        const uint32_t c = hist[0][d];
        if (cum + c >= k) break;
        cum += c;
      }
      sh_prefix = prefix | ((uint32_t)d << shift);
      sh_k = k - cum;
    }
    __syncthreads();
  }
  const uint32_t vkey = sh_prefix;
  uint32_t cnt = 0;
  for (int i = tid; i < HW; i += kSelThreads) {
    const uint32_t key = sel_key(sb[i]);
    const bool fg = key >= vkey && key > 0u;
    mask[(int64_t)b * HW + i] = fg ? 1 : 0;
    cnt += fg ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0 && cnt) atomicAdd(&sh_count, cnt);
  __syncthreads();
  if (tid == 0) {
    count[b] = (int32_t)sh_count;
    v[b] = __uint_as_float(vkey);
  }
}

// ---- stage 7: merge ------------------------------------------------------------------------------------------------------------
struct MergeArgs {
  const uint8_t* mask;
  const int32_t* count;
  const int64_t* perm;
  const uint8_t* apply;
  const int32_t* slot;
  float* scratch;
  int64_t S, L;            // floats per sample; floats per run (a colour plane, or a whole NHWC4 frame)
  int B, HW, nslots;
  uint32_t nruns, U;       // runs per sample; 16-byte units per run = (L + 6) / 4
};

__device__ __forceinline__ bool merge_active(const MergeArgs& a, int b) {
  return a.apply[b] != 0 && source_of(a.perm, b, a.B) != b && a.count[b] > 0;
}

// A clip b is merged when apply[b], perm[b] != b and count[b] > 0.  Its source clip may itself be merged in this call: then
// PACK copies the pixels b needs (its background) from x[perm[b]] into the scratch slot of b, and the second pass writes them into
// x[b]; a source that stays as it is is read directly by the second pass.  Nothing else is read or written.
template <int INNER, bool PACK>
__global__ __launch_bounds__(kThreads) void fg_merge_kernel(float* x, MergeArgs a) {
  const int b = blockIdx.z;
  if (!merge_active(a, b)) return;
  const int p = (int)source_of(a.perm, b, a.B);
  const bool staged = merge_active(a, p);
  const int sl = a.slot[b];
  if (staged && (sl < 0 || sl >= a.nslots)) return;      // the host assigns a slot to every such clip; never an address outside the scratch
  if (PACK && !staged) return;
  const uint32_t r = blockIdx.y, u = blockIdx.x * kThreads + threadIdx.x;      // run of the sample, 16-byte unit of the run
  float* drow = (PACK ? a.scratch + (int64_t)sl * a.S : x + (int64_t)b * a.S) + (int64_t)r * a.L;
  const float* srow = (PACK || !staged ? x + (int64_t)p * a.S : a.scratch + (int64_t)sl * a.S) + (int64_t)r * a.L;
  const uint8_t* mb = a.mask + (int64_t)b * a.HW;
  const int64_t e0 = 4 * (int64_t)u - phase4(drow);
  if (u >= a.U || e0 >= a.L) return;
  if (e0 >= 0 && e0 + 4 <= a.L) {      // a whole unit inside the run: one aligned 16-byte store at most, whatever the mask looks like
    uint32_t m;                          // the four mask bytes of the unit's elements
    if (INNER == 4 && (e0 & 3) == 0) {
      m = mb[e0 >> 2] ? 0x01010101u : 0u;            // NHWC4 on the pixel grid: one mask byte decides the unit
    } else if (INNER == 1 && ((reinterpret_cast<uintptr_t>(mb) + (uintptr_t)e0) & 3) == 0) {
      m = *reinterpret_cast<const uint32_t*>(mb + e0);
    } else {
      m = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) m |= (uint32_t)mb[(e0 + k) / INNER] << (8 * k);
    }
    const bool f0 = m & 0xffu, f1 = m & 0xff00u, f2 = m & 0xff0000u, f3 = m & 0xff000000u;
    if (f0 && f1 && f2 && f3) return;                // all foreground: nothing moves
    float4 v = ld4_any(srow + e0);
    if (!PACK && m != 0u) {                          // a mixed unit: the foreground elements keep the destination's values.  (PACK
      const float4 d = *reinterpret_cast<const float4*>(drow + e0);      // copies the whole unit: the assign pass ignores the rest)
      v.x = f0 ? d.x : v.x, v.y = f1 ? d.y : v.y, v.z = f2 ? d.z : v.z, v.w = f3 ? d.w : v.w;
    }
    *reinterpret_cast<float4*>(drow + e0) = v;
    return;
  }
  bool bg[4];
  int nbg = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t e = e0 + k;
    bg[k] = e >= 0 && e < a.L && mb[e / INNER] == 0;
    nbg += bg[k] ? 1 : 0;
  }
  if (nbg == 4) {
    *reinterpret_cast<float4*>(drow + e0) = ld4_any(srow + e0);
  } else if (nbg) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (bg[k]) drow[e0 + k] = srow[e0 + k];
  }
}

bool fg_clip(Clip& g, int T, int H, int W, int layout) {
  const int64_t HW = (int64_t)H * W;
  g.T = T, g.HW = (int)HW;
  if (layout == BDV_FG_TCHW) g.inner = 1, g.S = 3 * HW * T, g.tstride = 3 * HW, g.cstride = HW;
  else if (layout == BDV_FG_CTHW) g.inner = 1, g.S = 3 * HW * T, g.tstride = HW, g.cstride = HW * T;
  else if (layout == BDV_FG_THWC4) g.inner = 4, g.S = 4 * HW * T, g.tstride = 4 * HW, g.cstride = 1;
  else return false;
  return true;
}

// shared shape checks: a batch of B <= 65535 clips (grid y) whose sample fits 31 bits of pixels
#define FG_REQUIRE_SHAPE(name)                                                                                                      \
  BDV_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && W > 0, name ": B %d T %d H %d W %d (B <= 65535)", B, T, H, W);              \
  BDV_REQUIRE((int64_t)H * W <= (int64_t)1 << 24 && (int64_t)T * H * W <= (int64_t)1 << 28, name ": clip of %d x %d x %d too large", T, H, W)

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int bdv_fg_motion_q(const float* x, int B, int T, int H, int W, int layout, const float* taps_host, int k, float* d, float* tmp,
                               float* g, uint32_t* partials, uint32_t* minmax, uint8_t* q, void* stream) {
  BDV_REQUIRE(x && taps_host && d && tmp && g && partials && minmax && q, "bdv_fg_motion_q: null pointer");
  FG_REQUIRE_SHAPE("bdv_fg_motion_q");
  BDV_REQUIRE(T >= 2, "bdv_fg_motion_q: T %d: a motion map needs two frames", T);
  Clip c;
  BDV_REQUIRE(fg_clip(c, T, H, W, layout), "bdv_fg_motion_q: layout %d (BDV_FG_TCHW = 0 | BDV_FG_THWC4 = 1 | BDV_FG_CTHW = 2)", layout);
  BDV_REQUIRE(k >= 1 && k <= kMaxTaps && (k & 1) == 1 && k / 2 < H && k / 2 < W, "bdv_fg_motion_q: %d taps on a %d x %d map (odd, <= %d, radius inside the map)",
              k, H, W, kMaxTaps);
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(d) & 3) == 0 && (reinterpret_cast<uintptr_t>(tmp) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(g) & 3) == 0 && (reinterpret_cast<uintptr_t>(minmax) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(partials) & 3) == 0,
              "bdv_fg_motion_q: alignment");
  Taps taps;
  for (int j = 0; j < kMaxTaps; ++j) taps.w[j] = j < k ? taps_host[j] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gclip(blocks_for(c.HW, kBlockPix), B), gmap(blocks_for(c.HW, kThreads), B);
  if (c.inner == 1) hipLaunchKernelGGL(fg_motion_kernel<1>, gclip, dim3(kThreads), 0, st, x, d, c);
  else hipLaunchKernelGGL(fg_motion_kernel<4>, gclip, dim3(kThreads), 0, st, x, d, c);
  BDV_LAUNCH_CHECK("bdv_fg_motion_q(motion)");
  hipLaunchKernelGGL(fg_blur_kernel<true>, gmap, dim3(kThreads), 0, st, (const float*)d, tmp, partials, H, W, k, taps);
  BDV_LAUNCH_CHECK("bdv_fg_motion_q(blur w)");
  hipLaunchKernelGGL(fg_blur_kernel<false>, gmap, dim3(kThreads), 0, st, (const float*)tmp, g, partials, H, W, k, taps);
  BDV_LAUNCH_CHECK("bdv_fg_motion_q(blur h)");
  hipLaunchKernelGGL(fg_quant_kernel, gmap, dim3(kThreads), 0, st, (const float*)g, (const uint32_t*)partials, minmax, q, c.HW);
  BDV_LAUNCH_CHECK("bdv_fg_motion_q(quantise)");
  return BDV_OK;
}

extern "C" int bdv_fg_hist_refine(const float* x, const uint8_t* q, int B, int T, int H, int W, int layout, int bins, const float lo_host[3],
                                  const float scale_host[3], uint16_t* idx, uint32_t* F, uint32_t* N, float* s, void* stream) {
  BDV_REQUIRE(x && q && lo_host && scale_host && idx && F && N && s, "bdv_fg_hist_refine: null pointer");
  FG_REQUIRE_SHAPE("bdv_fg_hist_refine");
  BDV_REQUIRE(bins >= 2 && bins <= 16, "bdv_fg_hist_refine: bins %d outside 2..16", bins);
  BDV_REQUIRE(255ull * (uint64_t)T * (uint64_t)H * (uint64_t)W < (1ull << 32), "bdv_fg_hist_refine: 255 * T * H * W = 255 * %d * %d * %d does not fit uint32",
              T, H, W);
  Clip c;
  BDV_REQUIRE(fg_clip(c, T, H, W, layout), "bdv_fg_hist_refine: layout %d (BDV_FG_TCHW = 0 | BDV_FG_THWC4 = 1 | BDV_FG_CTHW = 2)", layout);
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7) == 0 && (reinterpret_cast<uintptr_t>(F) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(N) & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 3) == 0,
              "bdv_fg_hist_refine: alignment (idx: 8 bytes)");
  Colour col;
  for (int i = 0; i < 3; ++i) col.lo[i] = lo_host[i], col.s[i] = scale_host[i];
  const int nb = bins * bins * bins, HWp = (c.HW + 3) & ~3;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(F, 0, (size_t)B * nb * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(N, 0, (size_t)B * nb * sizeof(uint32_t), st);
  BDV_REQUIRE(e == hipSuccess, "bdv_fg_hist_refine: clearing the histograms failed: %s", hipGetErrorString(e));
  const dim3 gclip(blocks_for(c.HW, kBlockPix), B);
  if (c.inner == 1) hipLaunchKernelGGL(fg_hist_kernel<1>, gclip, dim3(kThreads), 0, st, x, q, idx, F, N, c, bins, col, HWp);
  else hipLaunchKernelGGL(fg_hist_kernel<4>, gclip, dim3(kThreads), 0, st, x, q, idx, F, N, c, bins, col, HWp);
  BDV_LAUNCH_CHECK("bdv_fg_hist_refine(histogram)");
  hipLaunchKernelGGL(fg_refine_kernel, gclip, dim3(kThreads), 0, st, (const uint16_t*)idx, (const uint32_t*)F, (const uint32_t*)N, s, T, c.HW, HWp, nb);
  BDV_LAUNCH_CHECK("bdv_fg_hist_refine(refine)");
  return BDV_OK;
}

extern "C" int bdv_fg_select(const float* s, int B, int HW, int k_fg, float* v, uint8_t* mask, int32_t* count, void* stream) {
  BDV_REQUIRE(s && v && mask && count, "bdv_fg_select: null pointer");
  BDV_REQUIRE(B > 0 && HW > 0 && HW <= 1 << 24, "bdv_fg_select: B %d, H * W %d", B, HW);
  BDV_REQUIRE(k_fg >= 1 && k_fg <= HW, "bdv_fg_select: k_fg %d outside 1..%d", k_fg, HW);
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(s) & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 3) == 0 && (reinterpret_cast<uintptr_t>(count) & 3) == 0,
              "bdv_fg_select: alignment");
  hipLaunchKernelGGL(fg_select_kernel, dim3(B), dim3(kSelThreads), 0, (hipStream_t)stream, s, HW, k_fg, v, mask, count);
  BDV_LAUNCH_CHECK("bdv_fg_select");
  return BDV_OK;
}

extern "C" int bdv_fg_merge(float* x, const uint8_t* mask, const int32_t* count, const int64_t* perm, const uint8_t* apply, const int32_t* slot,
                            int nslots, int B, int T, int H, int W, int layout, void* scratch, size_t scratch_bytes, void* stream) {
  BDV_REQUIRE(x && mask && count && perm && apply && slot, "bdv_fg_merge: null pointer");
  FG_REQUIRE_SHAPE("bdv_fg_merge");
  Clip c;
  BDV_REQUIRE(fg_clip(c, T, H, W, layout), "bdv_fg_merge: layout %d (BDV_FG_TCHW = 0 | BDV_FG_THWC4 = 1 | BDV_FG_CTHW = 2)", layout);
  BDV_REQUIRE(nslots >= 0 && nslots <= B, "bdv_fg_merge: %d scratch slots for %d clips", nslots, B);
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "bdv_fg_merge: alignment");
  if (nslots > 0) {
    BDV_REQUIRE(scratch != nullptr, "bdv_fg_merge: null scratch");
    BDV_REQUIRE(bdv_aligned16(scratch), "bdv_fg_merge: scratch alignment");
    BDV_REQUIRE(scratch_bytes >= (size_t)nslots * (size_t)c.S * sizeof(float), "bdv_fg_merge: scratch %zu bytes, need %zu", scratch_bytes,
                (size_t)nslots * (size_t)c.S * sizeof(float));
  }
  MergeArgs a;
  a.mask = mask, a.count = count, a.perm = perm, a.apply = apply, a.slot = slot, a.scratch = (float*)scratch;
  a.S = c.S, a.B = B, a.HW = c.HW, a.nslots = nslots;
  if (c.inner == 1) a.L = c.HW, a.nruns = 3u * (uint32_t)T;
  else a.L = 4 * (int64_t)c.HW, a.nruns = (uint32_t)T;
  a.U = (uint32_t)((a.L + 6) / 4);
  BDV_REQUIRE(a.nruns <= 65535u, "bdv_fg_merge: T %d too large (3 * T <= 65535)", T);
  const dim3 grid(blocks_for(a.U, kThreads), a.nruns, B);      // unit, run, clip
  hipStream_t st = (hipStream_t)stream;
  if (nslots > 0) {
    if (c.inner == 1) hipLaunchKernelGGL((fg_merge_kernel<1, true>), grid, dim3(kThreads), 0, st, x, a);
    else hipLaunchKernelGGL((fg_merge_kernel<4, true>), grid, dim3(kThreads), 0, st, x, a);
    BDV_LAUNCH_CHECK("bdv_fg_merge(pack)");
  }
  if (c.inner == 1) hipLaunchKernelGGL((fg_merge_kernel<1, false>), grid, dim3(kThreads), 0, st, x, a);
  else hipLaunchKernelGGL((fg_merge_kernel<4, false>), grid, dim3(kThreads), 0, st, x, a);
  BDV_LAUNCH_CHECK("bdv_fg_merge(assign)");
  return BDV_OK;
}
