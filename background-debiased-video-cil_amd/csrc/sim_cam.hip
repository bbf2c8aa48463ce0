// Simulated-camera-motion backgrounds: the reference's sim_cam_motion_bg_extract
// (cil_tools/extract_background.py:78-99) -- every frame through torchvision's RandomResizedCrop(size=100) as a float image,
// exact zeros turned into missing values, np.nanmedian / np.nanmean over time, .astype(uint8).
//
//   bdv_resized_crop_f32         (device) uint8 frames + one box per frame -> fp32 crops resized to one size: ATen's
//                                upsample_bilinear2d (antialias 0) or _upsample_bilinear2d_aa (antialias 1) on the float crop
//   bdv_temporal_nanreduce_f32   (device) ragged batch of fp32 stacks -> per position the median / mean of the present values,
//                                truncated to uint8
//
// This file is built with -ffp-contract=off: no product below may be fused into the addition that follows it.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// ---- resized crop -----------------------------------------------------------------------------------------------------------------
struct CropGeom {
  int H, W, Sh, Sw;
};

// ATen's linear source index (area_pixel_compute_source_index, align_corners=False) with guard_index_and_lambda: the two taps
// and the weight of the second one
struct LinTap {
  int i0, i1;
  float l;
};
__host__ __device__ __forceinline__ LinTap lin_tap(int d, float scale, int n) {
  // ONE rounding: ATen's vectorised CPU builds (AVX2, AVX512) contract this product and sum.  The two forms differ by an ulp of
  // the index -- up to 8e-3 of a grey level in the fraction at 320-pixel boxes; measured against torch 2.10 on the CPU, the
  // fused form stays within 3.1e-5 of it and the unfused one reaches 1.7e-3.  Nothing else in this file is fused.
  float f = fmaf(scale, (float)d + 0.5f, -0.5f);
  f = f < 0.f ? 0.f : f;
  int i0 = (int)f;
  i0 = i0 < n - 1 ? i0 : n - 1;
  float l = f - (float)i0;
  l = l < 0.f ? 0.f : l > 1.f ? 1.f : l;
  LinTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < n - 1 ? 1 : 0);
  t.l = l;
  return t;
}

// one output pixel, 2 x 2 bilinear: columns first, then rows (ATen's interpolate<2>)
__host__ __device__ __forceinline__ void crop_pixel_linear(const uint8_t* __restrict__ img, const CropGeom& g, int top, int left, int h,
                                                           int w, int oy, int ox, float (&out)[3]) {
  const float sh = (float)h / (float)g.Sh, sw = (float)w / (float)g.Sw;
  const LinTap ty = lin_tap(oy, sh, h), tx = lin_tap(ox, sw, w);
  const float hy = 1.f - ty.l, hx = 1.f - tx.l;
  const uint8_t* r0 = img + (size_t)(top + ty.i0) * g.W * 3;
  const uint8_t* r1 = img + (size_t)(top + ty.i1) * g.W * 3;
  const int x0 = (left + tx.i0) * 3, x1 = (left + tx.i1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t0 = hx * (float)r0[x0 + c] + tx.l * (float)r0[x1 + c];
    const float t1 = hx * (float)r1[x0 + c] + tx.l * (float)r1[x1 + c];
    out[c] = hy * t0 + ty.l * t1;
  }
}

// ATen's antialiased weights of one output index (_compute_indices_min_size_weights_aa with the triangle filter): the window
// [lo, lo + n) of the box axis, and what the unnormalised weights sum to.  The mixed float / double steps are ATen's.
struct AaAxis {
  int lo, n;
  float center, invscale, total;
};
__host__ __device__ __forceinline__ float aa_raw_weight(const AaAxis& a, int j) {
  float x = (float)(((double)((float)(j + a.lo) - a.center) + 0.5) * (double)a.invscale);
  x = x < 0.f ? -x : x;
  return x < 1.f ? 1.f - x : 0.f;
}
__host__ __device__ __forceinline__ AaAxis aa_axis(int d, float scale, int size) {
  AaAxis a;
  const float support = scale >= 1.f ? scale : 1.f;
  a.center = (float)((double)scale * ((double)d + 0.5));
  a.invscale = scale >= 1.f ? (float)(1.0 / (double)scale) : 1.f;
  long long lo = (long long)((double)(a.center - support) + 0.5);
  lo = lo > 0 ? lo : 0;
  long long hi = (long long)((double)(a.center + support) + 0.5);
  hi = hi < size ? hi : size;
  a.lo = (int)lo;
  a.n = (int)(hi - lo);
  a.total = 0.f;
  for (int j = 0; j < a.n; ++j) a.total += aa_raw_weight(a, j);
  return a;
}
__host__ __device__ __forceinline__ float aa_weight(const AaAxis& a, int j) {
  const float w = aa_raw_weight(a, j);
  return a.total != 0.f ? w / a.total : w;
}

// one output pixel, separable triangle filter: each contributing row is filtered horizontally (ATen's first pass, whose fp32
// result it keeps in a temporary), then the rows are combined (the second pass).  The weights are recomputed per tap, so that a
// reduction of any factor needs no table.
__host__ __device__ __forceinline__ void crop_pixel_aa(const uint8_t* __restrict__ img, const CropGeom& g, int top, int left, int h, int w,
                                                       int oy, int ox, float (&out)[3]) {
  const AaAxis ay = aa_axis(oy, (float)h / (float)g.Sh, h), ax = aa_axis(ox, (float)w / (float)g.Sw, w);
  out[0] = out[1] = out[2] = 0.f;
  for (int r = 0; r < ay.n; ++r) {
    const uint8_t* row = img + ((size_t)(top + ay.lo + r) * g.W + left + ax.lo) * 3;
    float t[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < ax.n; ++j) {
      const float wx = aa_weight(ax, j);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = (float)row[j * 3 + c] * wx;
        t[c] = j == 0 ? p : t[c] + p;
      }
    }
    const float wy = aa_weight(ay, r);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p = t[c] * wy;
      out[c] = r == 0 ? p : out[c] + p;
    }
  }
}

// one thread = one output pixel (three floats)
template <bool kAA>
__global__ __launch_bounds__(256) void resized_crop_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ boxes,
                                                            float* __restrict__ out, CropGeom g, long long total) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int per = g.Sh * g.Sw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int f = (int)(i / per), r = (int)(i - (long long)f * per);
    const int oy = r / g.Sw, ox = r - oy * g.Sw;
    const int32_t* b = boxes + (size_t)f * 4;
    const uint8_t* img = frames + (size_t)f * g.H * g.W * 3;
    float v[3];
    if (kAA)
      crop_pixel_aa(img, g, b[0], b[1], b[2], b[3], oy, ox, v);
    else
      crop_pixel_linear(img, g, b[0], b[1], b[2], b[3], oy, ox, v);
    float* o = out + i * 3;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
  }
}

// ---- NaN-aware temporal reduce ----------------------------------------------------------------------------------------------------
// One lane owns one position.  Median: a float's bits become a key that orders as the floats do (sign bit set for the non-negative
// ones, all bits flipped for the negative ones), and the lower middle order statistic of the present values is found most
// significant nibble first: eight passes over the stack, each counting the nibbles of the keys that share the nibbles chosen so
// far.  Counters sit in LDS at (nibble * 256 + lane) as in temporal_median_kernel: a lane only touches its own 16 dwords, all in
// bank (lane % 64) -- no conflicts, no barriers.  For an even count the upper middle value is the lower one again (ties), the next
// occupied nibble of the last pass, or the smallest key above the chosen prefix, kept as a running minimum over the passes.
constexpr int kRedThreads = 256;

__device__ __forceinline__ unsigned float_key(unsigned u) { return (u & 0x80000000u) ? ~u : u | 0x80000000u; }
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
__device__ __forceinline__ bool is_missing(unsigned u, bool zero_is_missing) {
  const unsigned m = u & 0x7fffffffu;
  return m > 0x7f800000u || (zero_is_missing && m == 0u);
}
// np.ndarray.astype(np.uint8) of the float on x86 for 0 <= v < 256 (truncation); saturated outside, NaN -> 0
__device__ __forceinline__ unsigned char trunc_u8(float v) { return (unsigned char)(v >= 255.f ? 255 : v > 0.f ? (int)v : 0); }

__global__ __launch_bounds__(kRedThreads) void nanmedian_kernel(const unsigned* __restrict__ frames, const long long* __restrict__ first,
                                                                 const int* __restrict__ counts, unsigned P, int zero_is_missing,
                                                                 unsigned char* __restrict__ out) {
  __shared__ unsigned hist[16 * kRedThreads];
  const unsigned tid = threadIdx.x;
  const unsigned p = blockIdx.x * kRedThreads + tid;
  if (p >= P) return;
  const int v = blockIdx.y;
  const int F = counts[v];
  const bool zm = zero_is_missing != 0;
  const unsigned* src = frames + (size_t)first[v] * P + p;
  unsigned char* dst = out + (size_t)v * P + p;
  unsigned* h = hist + tid;
  unsigned prefix = 0, rank = 0, n = 0;
  unsigned above = 0xffffffffu;        // no present value has this key (it is a NaN's)
  unsigned below = 0, c = 0, d = 0;
  for (int shift = 28; shift >= 0; shift -= 4) {
#pragma unroll
    for (int s = 0; s < 16; ++s) h[s * kRedThreads] = 0u;
    auto count = [&](unsigned u) {
      const unsigned key = float_key(u);
      const unsigned hi = shift == 28 ? 0u : key >> (shift + 4);
      const bool present = !is_missing(u, zm);
      const unsigned cand = present && hi > prefix ? key : 0xffffffffu;
      above = cand < above ? cand : above;
      atomicAdd(h + ((key >> shift) & 15u) * kRedThreads, present && hi == prefix ? 1u : 0u);
    };
    int f = 0;
    for (; f + 4 <= F; f += 4) {       // four loads in flight per lane
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = src[(size_t)(f + j) * P];
#pragma unroll
      for (int j = 0; j < 4; ++j) count(w[j]);
    }
    for (; f < F; ++f) count(src[(size_t)f * P]);
    if (shift == 28) {
#pragma unroll
      for (int s = 0; s < 16; ++s) n += h[s * kRedThreads];
      if (n == 0) {                    // every frame missing here: numpy's NaN, which its cast turns into 0
        *dst = 0;
        return;
      }
      rank = (n - 1) >> 1;             // the lower middle value (the middle one for odd n)
    }
    below = 0;
    for (d = 0; d < 15; ++d) {
      c = h[d * kRedThreads];
      if (below + c > rank) break;
      below += c;
    }
    if (d == 15) c = h[15 * kRedThreads];
    if (shift > 0) rank -= below;
    prefix = (prefix << 4) | d;
  }
  const float a = key_float(prefix);
  float m = a;
  if ((n & 1u) == 0) {
    unsigned kb = prefix;              // below + c > rank + 1: the upper middle value is a tie of the lower one
    if (below + c <= rank + 1) {
      kb = above;
      for (unsigned l = d + 1; l < 16; ++l)
        if (h[l * kRedThreads]) {
          kb = (prefix & ~15u) | l;
          break;
        }
    }
    m = (a + key_float(kb)) * 0.5f;
  }
  *dst = trunc_u8(m);
}

// np.nanmean over axis 0: the present values added in frame order in fp32, divided by their count
__global__ __launch_bounds__(kRedThreads) void nanmean_kernel(const float* __restrict__ frames, const long long* __restrict__ first,
                                                               const int* __restrict__ counts, unsigned P, int zero_is_missing,
                                                               unsigned char* __restrict__ out) {
  const unsigned p = blockIdx.x * kRedThreads + threadIdx.x;
  if (p >= P) return;
  const int v = blockIdx.y;
  const int F = counts[v];
  const bool zm = zero_is_missing != 0;
  const float* src = frames + (size_t)first[v] * P + p;
  float sum = 0.f;
  unsigned n = 0;
  auto add = [&](float x) {
    if (!is_missing(__float_as_uint(x), zm)) {
      sum += x;
      ++n;
    }
  };
  int f = 0;
  for (; f + 4 <= F; f += 4) {
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = src[(size_t)(f + j) * P];
#pragma unroll
    for (int j = 0; j < 4; ++j) add(w[j]);
  }
  for (; f < F; ++f) add(src[(size_t)f * P]);
  out[(size_t)v * P + p] = n ? trunc_u8(sum / (float)n) : (unsigned char)0;
}

}  // namespace

extern "C" int bdv_resized_crop_f32(const uint8_t* frames, int F, int H, int W, const int32_t* boxes, const int32_t* boxes_host, int out_h,
                                    int out_w, int antialias, float* out, void* stream) {
  BDV_REQUIRE(frames && boxes && boxes_host && out, "bdv_resized_crop_f32: null pointer");
  BDV_REQUIRE(F > 0 && H > 0 && W > 0 && out_h > 0 && out_w > 0 && out_h <= 16384 && out_w <= 16384,
              "bdv_resized_crop_f32: bad sizes (F=%d, %d x %d -> %d x %d)", F, H, W, out_h, out_w);
  BDV_REQUIRE((long long)H * W * 3 < (1ll << 31), "bdv_resized_crop_f32: frame too large");
  BDV_REQUIRE(antialias == 0 || antialias == 1, "bdv_resized_crop_f32: antialias %d (0 | 1)", antialias);
  for (int f = 0; f < F; ++f) {
    const int32_t* b = boxes_host + (size_t)f * 4;
    BDV_REQUIRE(b[0] >= 0 && b[1] >= 0 && b[2] >= 1 && b[3] >= 1 && (long long)b[0] + b[2] <= H && (long long)b[1] + b[3] <= W,
                "bdv_resized_crop_f32: frame %d: box (top %d, left %d, %d x %d) leaves the %d x %d frame", f, b[0], b[1], b[2], b[3], H, W);
  }
  CropGeom g{H, W, out_h, out_w};
  const long long total = (long long)F * out_h * out_w;
  const unsigned blocks = (unsigned)bdv_ew_grid(total);
  if (antialias)
    hipLaunchKernelGGL(resized_crop_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, frames, boxes, out, g, total);
  else
    hipLaunchKernelGGL(resized_crop_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, frames, boxes, out, g, total);
  BDV_LAUNCH_CHECK("bdv_resized_crop_f32");
  return BDV_OK;
}

extern "C" int bdv_temporal_nanreduce_f32(const float* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                                          const int64_t* first_host, const int32_t* counts_host, int V, int64_t P, int mode,
                                          int zero_is_missing, uint8_t* out, void* stream) {
  BDV_REQUIRE(frames && first && counts && first_host && counts_host && out, "bdv_temporal_nanreduce_f32: null pointer");
  BDV_REQUIRE(V > 0 && V <= 65535 && P > 0 && P < (1ll << 31) - 1024, "bdv_temporal_nanreduce_f32: bad batch (V=%d, P=%lld)", V, (long long)P);
  BDV_REQUIRE(mode == 0 || mode == 1, "bdv_temporal_nanreduce_f32: mode %d (0 = median | 1 = mean)", mode);
  if (int rc = bdv_check_video_runs("bdv_temporal_nanreduce_f32", first_host, counts_host, V, total_frames)) return rc;
  dim3 grid((unsigned)((P + kRedThreads - 1) / kRedThreads), (unsigned)V);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL(nanmedian_kernel, grid, dim3(kRedThreads), 0, s, reinterpret_cast<const unsigned*>(frames), (const long long*)first,
                       counts, (unsigned)P, zero_is_missing, out);
  else
    hipLaunchKernelGGL(nanmean_kernel, grid, dim3(kRedThreads), 0, s, frames, (const long long*)first, counts, (unsigned)P, zero_is_missing, out);
  BDV_LAUNCH_CHECK("bdv_temporal_nanreduce_f32");
  return BDV_OK;
}
