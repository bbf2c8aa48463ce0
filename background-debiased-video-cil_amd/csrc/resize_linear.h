// OpenCV's INTER_LINEAR on 8-bit images: the box setup, one output pixel, and the walk over and store of a thread's four pixels,
// shared by bdv_resize_linear_u8 (augment.hip), bdv_resize_linear_ragged_u8 (ragged.hip) and the ActorCutMix composite
// (actor_cut_mix.hip).  UPSTREAM mmaction2 Resize -> mmcv.imresize(interpolation='bilinear') ->
// cv2.resize(..., INTER_LINEAR); the arithmetic restates OpenCV's published fixed-point algorithm (imgproc/resize.cpp) --
// PARITY UNPINNED, see oracle/resize_oracle.py.  Every file that includes this header is built with -ffp-contract=off: the
// float / double operations below must not be contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

struct ResizeAxis {
  int s0, s1;     // source taps (already clamped into the box)
  int a0, a1;     // 11-bit weights
};

__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// x axis: a tap left of / beyond the last column collapses onto the edge with weight 1 (cv::resize clamps fx there)
__device__ __forceinline__ ResizeAxis resize_axis_x(int d, double scale, int ssize) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.f;
    s = ssize - 1;
  }
  ResizeAxis r;
  r.s0 = s;
  r.s1 = s + 1 < ssize ? s + 1 : ssize - 1;
  r.a0 = sat_short(__float2int_rn((1.f - f) * 2048.f));
  r.a1 = sat_short(__float2int_rn(f * 2048.f));
  return r;
}

// y axis: the weights keep the unclamped fraction, only the row indices are clipped (resizeGeneric_Invoker)
__device__ __forceinline__ ResizeAxis resize_axis_y(int d, double scale, int ssize) {
  float f = (float)((d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= s;
  ResizeAxis r;
  r.s0 = s < 0 ? 0 : s >= ssize ? ssize - 1 : s;
  r.s1 = s + 1 < 0 ? 0 : s + 1 >= ssize ? ssize - 1 : s + 1;
  r.a0 = sat_short(__float2int_rn((1.f - f) * 2048.f));
  r.a1 = sat_short(__float2int_rn(f * 2048.f));
  return r;
}

struct ResizeBox {
  const uint8_t* base;   // first pixel of the box
  size_t pitch;
  int bw, bh, mode;      // mode 0: resample, 1: copy (same size), 2: 2x2 box mean (exact 2x shrink)
  double scale_x, scale_y;
};

// source column of box column c: FLIP reads the box mirrored (column c of np.flip(box, 1) is column bw - 1 - c), so the taps
// and weights are those of the mirrored image -- cv::resize's x-axis edge handling is not symmetric, flipping the output would
// not give the same pixels
template <bool FLIP>
__device__ __forceinline__ int resize_col(const ResizeBox& b, int c) { return FLIP ? b.bw - 1 - c : c; }

// one output pixel of a box -> packed 0x00BBGGRR; FLIP: of the horizontally mirrored box
template <bool FLIP = false>
__device__ __forceinline__ unsigned resize_pixel(const ResizeBox& b, int dx, int dy) {
  unsigned out = 0;
  if (b.mode == 1) {   // same size: cv::resize copies
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= (unsigned)b.base[dy * b.pitch + resize_col<FLIP>(b, dx) * 3 + c] << (8 * c);
    return out;
  }
  if (b.mode == 2) {   // exact 2x shrink: INTER_LINEAR is replaced by the fast INTER_AREA (2x2 mean, rounded)
    const uint8_t* r0 = b.base + (size_t)(2 * dy) * b.pitch;
    const int c0 = resize_col<FLIP>(b, 2 * dx) * 3, c1 = resize_col<FLIP>(b, 2 * dx + 1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= (unsigned)((r0[c0 + c] + r0[c1 + c] + r0[b.pitch + c0 + c] + r0[b.pitch + c1 + c] + 2) >> 2) << (8 * c);
    return out;
  }
  const ResizeAxis ax = resize_axis_x(dx, b.scale_x, b.bw), ay = resize_axis_y(dy, b.scale_y, b.bh);
  const uint8_t* r0 = b.base + (size_t)ay.s0 * b.pitch;
  const uint8_t* r1 = b.base + (size_t)ay.s1 * b.pitch;
  const int x0 = resize_col<FLIP>(b, ax.s0) * 3, x1 = resize_col<FLIP>(b, ax.s1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = r0[x0 + c] * ax.a0 + r0[x1 + c] * ax.a1;
    const int h1 = r1[x0 + c] * ax.a0 + r1[x1 + c] * ax.a1;
    const int v = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
    out |= (unsigned)(v & 255) << (8 * c);
  }
  return out;
}

// The path cv::resize takes for a bw x bh box (first pixel at base, rows `pitch` bytes apart) resized to Wd x Hd: a copy for the same
// size, the 2x2 mean for an exact 2x shrink, else the fixed-point resample with cv::resize's scales 1 / (dsize / ssize) in double
__device__ __forceinline__ ResizeBox resize_box(const uint8_t* base, size_t pitch, int bw, int bh, int Hd, int Wd) {
  ResizeBox b;
  b.base = base;
  b.pitch = pitch;
  b.bw = bw;
  b.bh = bh;
  b.mode = (bw == Wd && bh == Hd) ? 1 : (bw == 2 * Wd && bh == 2 * Hd) ? 2 : 0;
  b.scale_x = 1.0 / ((double)Wd / bw);
  b.scale_y = 1.0 / ((double)Hd / bh);
  return b;
}

// A thread's group of four consecutive output pixels from pixel p0 of a frame of npix pixels, Wd wide: (dx, dy) of the current pixel
// and cnt, the number of pixels that exist (the last group of a frame may be short).  One integer division per group, none per pixel.
struct ResizeGroup {
  int dx, dy, cnt;
  __device__ __forceinline__ void next(int Wd) {
    if (++dx == Wd) {
      dx = 0;
      ++dy;
    }
  }
};

__device__ __forceinline__ ResizeGroup resize_group(unsigned p0, unsigned npix, int Wd) {
  ResizeGroup g;
  g.dy = (int)(p0 / (unsigned)Wd);
  g.dx = (int)(p0 - (unsigned)g.dy * (unsigned)Wd);
  g.cnt = npix - p0 < 4u ? (int)(npix - p0) : 4;
  return g;
}

// cnt packed pixels to out: three aligned dwords for a whole group when `dwords` (out is 4-byte aligned: the frame starts aligned and
// is a whole number of dwords), else byte by byte
__device__ __forceinline__ void resize_store4(uint8_t* out, const unsigned (&px)[4], int cnt, bool dwords) {
  if (cnt == 4 && dwords) {
    unsigned* o = reinterpret_cast<unsigned*>(out);
    o[0] = px[0] | (px[1] << 24);
    o[1] = (px[1] >> 8) | (px[2] << 16);
    o[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    for (int k = 0; k < cnt; ++k) {
      out[3 * k] = (uint8_t)px[k];
      out[3 * k + 1] = (uint8_t)(px[k] >> 8);
      out[3 * k + 2] = (uint8_t)(px[k] >> 16);
    }
  }
}

}  // namespace
