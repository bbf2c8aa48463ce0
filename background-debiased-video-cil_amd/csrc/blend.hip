// Clip blending for train_cfg.blending and VideoMix (UPSTREAM mmaction/datasets/blending_utils.py, libs/cil/icarl_video_mix.py:59):
//   bdv_blend_mix_f32   out[b] = lam * x[b] + (1 - lam) * x[perm[b]]                      (MixupBlending.do_blending)
//   bdv_blend_box_f32   x[b, :, r1:r2, c1:c2, :] = x[perm[b], :, r1:r2, c1:c2, :], in place (CutmixBlending.do_blending, tubemix)
// Both are pure memory traffic in fp32.  Built with -ffp-contract=off: the two products and the sum of the mix are rounded
// separately, which is torch's `lam * x + (1 - lam) * x[perm]` bit for bit.
//
// Addressing.  A thread moves one 16-byte unit of a destination run (a whole sample for the mix, one box row, or a merged run of box
// rows, for the copy).  Units are laid on the 16-byte grid of the DESTINATION address, so every wide store is aligned whatever the
// sample size (210 floats per sample put every odd sample on an 8-byte boundary) and whatever the box column; the units that hang
// over the ends of the run are written element by element.  A source run generally sits at another phase of that grid (another
// sample, a scratch row): ld4_any reads it as one 16-byte, two 8-byte or four 4-byte loads, whichever its address allows.  That
// choice is the same for every unit of a run, so a wave does not diverge on it.
#include "common.h"
#include "loader_pieces.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float mix1(float lam, float om, float a, float b) {
  const float u = lam * a, v = om * b;       // no contraction in this file
  return u + v;
}

__global__ __launch_bounds__(kThreads) void blend_mix_kernel(const float* __restrict__ x, const int64_t* __restrict__ perm, float lam,
                                                             float* __restrict__ out, int B, int64_t S) {
  const float om = 1.0f - lam;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* xa = x + (int64_t)b * S;
    const float* xb = x + source_of(perm, b, B) * S;
    float* o = out + (int64_t)b * S;
    const int ph = phase4(o);
    const int64_t units = (ph + S + 3) >> 2;
    for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
      const int64_t e0 = 4 * u - ph;
      if (e0 >= 0 && e0 + 4 <= S) {
        const float4 a = ld4_any(xa + e0), c = ld4_any(xb + e0);
        *reinterpret_cast<float4*>(o + e0) =
            make_float4(mix1(lam, om, a.x, c.x), mix1(lam, om, a.y, c.y), mix1(lam, om, a.z, c.z), mix1(lam, om, a.w, c.w));
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t e = e0 + k;
          if (e >= 0 && e < S) o[e] = mix1(lam, om, xa[e], xb[e]);
        }
      }
    }
  }
}

// The runs of one sample's box: `nrows` runs of L floats; run q starts (q / rps) * slab_stride + (q % rps) * row_stride floats after
// the box origin (off0 floats into the sample).  rps = rows per outer slab.
struct BoxRuns {
  int64_t S, off0, slab_stride, row_stride, L;
  uint32_t nrows, rps, U;      // U = units per run = (L + 6) / 4: L floats at any phase 0..3 of the 16-byte grid
};

// PACK: scratch[b] <- box of x[perm[b]];  !PACK: box of x[b] <- scratch[b].  A scratch run has a pitch of 4 * U floats and starts at
// the phase of the run of x[b] it is meant for, so the second pass moves aligned 16-byte units on both sides.  Samples with
// perm[b] == b are skipped in both passes.
template <bool PACK>
__global__ __launch_bounds__(kThreads) void blend_box_kernel(float* x, const int64_t* __restrict__ perm, float* scratch, int B, BoxRuns g) {
  const uint32_t total = g.nrows * g.U;
  const uint32_t stride = gridDim.x * kThreads;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t p = source_of(perm, b, B);
    if (p == b) continue;
    float* xd = x + (int64_t)b * g.S + g.off0;
    const float* xs = x + p * g.S + g.off0;
    float* sc = scratch + (int64_t)b * g.nrows * g.U * 4;
    for (uint32_t t = blockIdx.x * kThreads + threadIdx.x; t < total; t += stride) {
      const uint32_t q = t / g.U, u = t - q * g.U;
      const uint32_t slab = q / g.rps, r = q - slab * g.rps;
      const int64_t roff = (int64_t)slab * g.slab_stride + (int64_t)r * g.row_stride;
      float* drow = xd + roff;
      const int ph = phase4(drow);
      float* srow = sc + (int64_t)q * g.U * 4 + ph;
      const int64_t e0 = 4 * (int64_t)u - ph;
      if (e0 >= g.L) continue;
      const float* src = PACK ? xs + roff : srow;
      float* dst = PACK ? srow : drow;
      if (e0 >= 0 && e0 + 4 <= g.L) {
        *reinterpret_cast<float4*>(dst + e0) = ld4_any(src + e0);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t e = e0 + k;
          if (e >= 0 && e < g.L) dst[e] = src[e];
        }
      }
    }
  }
}

dim3 blend_grid(int64_t units_per_sample, int B) {
  const int gy = B < 65535 ? B : 65535;
  return dim3((unsigned)bdv_ew_grid(units_per_sample, gy), (unsigned)gy);      // kThreads is the helper's 256
}

inline int64_t box_units(int64_t L) { return (L + 6) / 4; }

}  // namespace

extern "C" int bdv_blend_mix_f32(const float* x, const int64_t* perm, float lam, float* out, int B, int64_t sample_elems, void* stream) {
  BDV_REQUIRE(x && perm && out, "bdv_blend_mix_f32: null pointer");
  BDV_REQUIRE(B > 0 && sample_elems > 0, "bdv_blend_mix_f32: B %d, sample_elems %lld", B, (long long)sample_elems);
  BDV_REQUIRE(sample_elems <= (INT64_MAX >> 3) / B, "bdv_blend_mix_f32: batch too large");
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "bdv_blend_mix_f32: alignment");
  const int64_t n = (int64_t)B * sample_elems;
  BDV_REQUIRE(out + n <= x || x + n <= out, "bdv_blend_mix_f32: out must not alias x");
  hipLaunchKernelGGL(blend_mix_kernel, blend_grid((sample_elems + 6) / 4, B), dim3(kThreads), 0, (hipStream_t)stream, x, perm, lam, out, B,
                     sample_elems);
  BDV_LAUNCH_CHECK("bdv_blend_mix_f32");
  return BDV_OK;
}

extern "C" size_t bdv_blend_box_scratch_bytes(int B, int outer, int inner, int r1, int c1, int r2, int c2) {
  if (B <= 0 || outer <= 0 || inner <= 0 || r1 < 0 || c1 < 0 || r2 <= r1 || c2 <= c1) return 0;
  return (size_t)B * (size_t)outer * (size_t)(r2 - r1) * (size_t)box_units((int64_t)(c2 - c1) * inner) * 16;
}

extern "C" int bdv_blend_box_f32(float* x, const int64_t* perm, int B, int outer, int H, int W, int inner, int r1, int c1, int r2, int c2,
                                 void* scratch, size_t scratch_bytes, void* stream) {
  BDV_REQUIRE(x && perm, "bdv_blend_box_f32: null pointer");
  BDV_REQUIRE(B > 0 && outer > 0 && H > 0 && W > 0, "bdv_blend_box_f32: B %d outer %d H %d W %d", B, outer, H, W);
  BDV_REQUIRE(inner == 1 || inner == 4, "bdv_blend_box_f32: inner %d (1 = planar, 4 = NHWC4)", inner);
  BDV_REQUIRE(0 <= r1 && r1 <= r2 && r2 <= H && 0 <= c1 && c1 <= c2 && c2 <= W, "bdv_blend_box_f32: box rows %d:%d cols %d:%d outside %d x %d",
              r1, r2, c1, c2, H, W);
  BDV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "bdv_blend_box_f32: alignment");
  if (r1 == r2 || c1 == c2) return BDV_OK;      // empty box: nothing to copy, no launch
  BoxRuns g;
  const int64_t plane = (int64_t)H * W * inner;
  g.S = (int64_t)outer * plane;
  BDV_REQUIRE(g.S <= (INT64_MAX >> 3) / B, "bdv_blend_box_f32: batch too large");
  // full-width rows are contiguous: merge them into one run per outer slab, and a full frame into one run per sample
  int64_t nrows;
  if (c1 == 0 && c2 == W && r1 == 0 && r2 == H) {
    nrows = 1, g.rps = 1, g.L = g.S, g.off0 = 0, g.slab_stride = 0, g.row_stride = 0;
  } else if (c1 == 0 && c2 == W) {
    nrows = outer, g.rps = 1, g.L = (int64_t)(r2 - r1) * W * inner, g.off0 = (int64_t)r1 * W * inner, g.slab_stride = plane, g.row_stride = 0;
  } else {
    nrows = (int64_t)outer * (r2 - r1), g.rps = (uint32_t)(r2 - r1), g.L = (int64_t)(c2 - c1) * inner;
    g.off0 = ((int64_t)r1 * W + c1) * inner, g.slab_stride = plane, g.row_stride = (int64_t)W * inner;
  }
  const int64_t U = box_units(g.L);
  BDV_REQUIRE(nrows * U < ((int64_t)1 << 31), "bdv_blend_box_f32: box too large");
  g.nrows = (uint32_t)nrows, g.U = (uint32_t)U;
  const size_t need = (size_t)B * (size_t)nrows * (size_t)U * 16;      // never more than the row-by-row bound below
  BDV_REQUIRE(scratch != nullptr, "bdv_blend_box_f32: null scratch");
  BDV_REQUIRE(bdv_aligned16(scratch), "bdv_blend_box_f32: scratch alignment");
  const size_t bound = bdv_blend_box_scratch_bytes(B, outer, inner, r1, c1, r2, c2);
  BDV_REQUIRE(scratch_bytes >= bound && bound >= need, "bdv_blend_box_f32: scratch %zu bytes, need %zu", scratch_bytes, bound);
  const dim3 grid = blend_grid(nrows * U, B);
  hipLaunchKernelGGL(blend_box_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, perm, (float*)scratch, B, g);
  BDV_LAUNCH_CHECK("bdv_blend_box_f32(pack)");
  hipLaunchKernelGGL(blend_box_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, perm, (float*)scratch, B, g);
  BDV_LAUNCH_CHECK("bdv_blend_box_f32(unpack)");
  return BDV_OK;
}
