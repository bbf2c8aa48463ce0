// Grad-CAM arithmetic on the device (UPSTREAM mmaction2 GradCAM._calculate_localization_map, mmaction/utils/gradcam_utils.py, for a
// 2D recognizer -- restated from memory, PARITY UNPINNED: mmaction2 is not vendored):
//   channel weights = mean over (y, x) of the gradient          (the existing bdv_avgpool_fwd, not a kernel of this file)
//   m = relu(sum_c wgt[n, c] * A[n, y, x, c])                   gradcam_map_kernel
//   u = F.interpolate(m, (H, W), 'bilinear', align_corners=False) per frame; per clip min / max over all T*H*W values of u
//                                                               gradcam_minmax_kernel
//   v = (u - min) / (max - min + 1e-20), the colormap overlay and the box sums   gradcam_render_kernel + gradcam_sums_kernel
// u is never stored: the minmax and the render kernel recompute it with the same device function (no contraction in this file, so
// the two agree bit for bit and the clip's v holds an exact 0).  No float atomics anywhere: the extremes go through integer
// atomics on the bits of non-negative floats (the integer order is the float order there, so the result does not depend on the
// order of arrival), the box sums through per-row partials in fp64 and one finalize, both in a fixed order.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// ---- m = relu(A . wgt) --------------------------------------------------------------------------------------------------------
// One wave per output pixel, 4 pixels per 256-thread block.  Lane l takes the channel groups l, l + 64, ... (16 bytes each), so
// every load instruction of a wave reads 1 KiB of consecutive bytes of A (and of wgt[n, :], which the pixels of a frame share
// through the caches); C/4 may be smaller than 64, the lanes past it add nothing.  Products are accumulated with fmaf in channel
// order inside a lane, then the 64 lane sums are combined by the xor butterfly of wave_sum: one fixed tree, the same bits each run.
__global__ __launch_bounds__(256) void gradcam_map_kernel(const float4* __restrict__ A, const float4* __restrict__ wgt,
                                                          float* __restrict__ m, int64_t npix, int HW, int CV) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
  if (p >= npix) return;                                               // whole waves leave: the shuffles below see 64 lanes
  const int64_t n = p / HW;
  const float4* a = A + p * CV;
  const float4* w = wgt + n * CV;
  float acc = 0.f;
  for (int c = lane; c < CV; c += 64) {
    const float4 av = a[c], wv = w[c];
    acc = fmaf(wv.x, av.x, acc);
    acc = fmaf(wv.y, av.y, acc);
    acc = fmaf(wv.z, av.z, acc);
    acc = fmaf(wv.w, av.w, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) m[p] = acc > 0.f ? acc : 0.f;                         // (-0 and NaN become +0: the later bit-order atomics need it)
}

// ---- the upsampled value at one output pixel -----------------------------------------------------------------------------------
// ATen's upsample_bilinear2d with align_corners=False, indices and fractions as bg_resize_crop_kernel (pool_frontend.hip) restates
// them: source index scale * (dst + 0.5) - 0.5 clamped at 0, the second tap clamped to the last row / column,
// columns combined before rows.  The source coordinate is computed in fp64 (two operations per axis and pixel) and only the
// fraction is rounded to fp32: in fp32 the coordinate alone would carry up to an ulp of in (2^-21 for in = 7), as much as the whole
// budget of 8 * 2^-24 * max|m| against an fp64 reference.  The two taps are combined as a + l * (b - a) and not as a * (1 - l) + b * l: on a constant map
// the difference is exactly 0 and u is exactly the constant, so a constant clip normalises to zeros whatever its value (with the
// two-weight form u wobbles by an ulp and the normalised map of a constant clip is noise in {0, 1}).  Each form is within
// 3 * 2^-24 * max|m| per axis of the exact value.
struct UpAxis {
  int i0, i1;
  float l;          // weight of i1
};

__device__ __forceinline__ UpAxis up_axis(int d, double scale, int in) {
  double f = scale * ((double)d + 0.5) - 0.5;
  f = f < 0.0 ? 0.0 : f;
  int i0 = (int)f;
  i0 = i0 > in - 1 ? in - 1 : i0;
  UpAxis a;
  a.i0 = i0;
  a.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  a.l = fminf(fmaxf((float)(f - (double)i0), 0.f), 1.f);
  return a;
}

__device__ __forceinline__ float up_value(const float* __restrict__ frame, int w, const UpAxis& ay, const UpAxis& ax) {
  const float* r0 = frame + (size_t)ay.i0 * w;
  const float* r1 = frame + (size_t)ay.i1 * w;
  const float t0 = r0[ax.i0] + ax.l * (r0[ax.i1] - r0[ax.i0]);
  const float t1 = r1[ax.i0] + ax.l * (r1[ax.i1] - r1[ax.i0]);
  const float u = t0 + ay.l * (t1 - t0);
  return u > 0.f ? u : 0.f;                                            // the map is non-negative; keeps the bit order total
}

// ---- per clip min / max of u -----------------------------------------------------------------------------------------------------
// grid (row groups of a clip, B): a block walks output rows (t, y) of its clip, its threads the pixels of a row; the extremes are
// reduced in the wave, then in the block, and each block issues one integer atomic per extreme: at most 128 blocks per clip, so
// the two words of a clip see at most 128 atomics each.  mm[0][b] = min (preset to 0x7F7F7F7F by the launcher), mm[1][b] = max
// (preset 0).
__global__ __launch_bounds__(256) void gradcam_minmax_kernel(const float* __restrict__ m, unsigned* __restrict__ mm, int B, int T, int h,
                                                             int w, int H, int W) {
  __shared__ unsigned red[8];
  const int b = blockIdx.y;
  const double sy = (double)h / (double)H, sx = (double)w / (double)W;
  const int rows = T * H;
  unsigned lo = 0x7F7F7F7Fu, hi = 0u;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int t = row / H, y = row - t * H;
    const UpAxis ay = up_axis(y, sy, h);
    const float* frame = m + ((int64_t)b * T + t) * h * w;
    for (int x = threadIdx.x; x < W; x += 256) {
      const unsigned bits = __float_as_uint(up_value(frame, w, ay, up_axis(x, sx, w)));
      lo = bits < lo ? bits : lo;
      hi = bits > hi ? bits : hi;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = lo;
    red[4 + (threadIdx.x >> 6)] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      lo = red[k] < lo ? red[k] : lo;
      hi = red[4 + k] > hi ? red[4 + k] : hi;
    }
    atomicMin(mm + b, lo);
    atomicMax(mm + B + b, hi);
  }
}

// ---- v, overlay, box sums ----------------------------------------------------------------------------------------------------------
struct RenderArgs {
  const float* m;          // (B*T, h, w)
  const float* mm;         // (2, B)
  float* v;                // (B, T, H, W) | null
  const float4* frames;    // (B*T, H, W, 4) normalised frames | null
  const float* lut;        // (256, 3)
  uint8_t* overlay;        // (B, T, H, W, 3) | null
  const int32_t* off;      // (B*T + 1) | null: no sums
  const float* boxes;      // (nbox, 4) x0 y0 x1 y1 in output-pixel coordinates
  double* partial;         // (B*T*H, 2)
  int T, h, w, H, W;
  float alpha, mean[3], std[3];
};

// The block sums below: butterfly inside each wave, then the four wave sums left to right (SumOrder::Sequential); sh may still be
// read from the previous call (REUSE).
// one block per output row (b, t, y)
__global__ __launch_bounds__(256) void gradcam_render_kernel(const RenderArgs a) {
  __shared__ double sh[4];
  const int64_t row = blockIdx.x;
  const int y = (int)(row % a.H);
  const int64_t f = row / a.H;          // frame b*T + t
  const int b = (int)(f / a.T);
  const int B = (int)(gridDim.x / ((int64_t)a.T * a.H));
  const float mn = a.mm[b], mx = a.mm[B + b];
  const float den = (mx - mn) + 1e-20f;
  const double sy = (double)a.h / (double)a.H, sx = (double)a.w / (double)a.W;
  const UpAxis ay = up_axis(y, sy, a.h);
  const float* frame = a.m + f * a.h * a.w;
  int b0 = 0, b1 = 0;
  if (a.off) {
    b0 = a.off[f];
    b1 = a.off[f + 1];
  }
  const float cy = (float)y + 0.5f;
  const float na = 1.f - a.alpha;
  double sv = 0.0, si = 0.0;
  for (int x = threadIdx.x; x < a.W; x += 256) {
    const float u = up_value(frame, a.w, ay, up_axis(x, sx, a.w));
    const float v = (u - mn) / den;
    const int64_t o = row * a.W + x;
    if (a.v) a.v[o] = v;
    if (a.overlay) {
      int idx = v > 0.f ? (int)floorf(256.f * v) : 0;       // matplotlib's lookup: int(v * N), the top value in the last bin
      idx = idx > 255 ? 255 : idx;
      const float4 px = a.frames[o];
      const float in[3] = {px.x, px.y, px.z};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float img01 = fmaf(in[c], a.std[c], a.mean[c]) / 255.f;
        float q = fmaf(a.alpha, a.lut[idx * 3 + c], na * img01);
        q = fminf(fmaxf(q, 0.f), 1.f);
        a.overlay[o * 3 + c] = (uint8_t)rintf(255.f * q);
      }
    }
    if (a.off) {
      const float cx = (float)x + 0.5f;
      bool in = false;
      for (int k = b0; k < b1; ++k) {
        const float* q = a.boxes + 4 * (size_t)k;
        in |= q[0] <= cx && cx < q[2] && q[1] <= cy && cy < q[3];
      }
      sv += (double)v;
      si += in ? (double)v : 0.0;
    }
  }
  if (a.off) {
    sv = block_sum<SumOrder::Sequential, true>(sv, sh);
    si = block_sum<SumOrder::Sequential, true>(si, sh);
    if (threadIdx.x == 0) {
      a.partial[2 * row] = sv;
      a.partial[2 * row + 1] = si;
    }
  }
}

// one block per clip: its T*H row partials, thread-strided in row order, then the fixed tree
__global__ __launch_bounds__(256) void gradcam_sums_kernel(const double* __restrict__ partial, float* __restrict__ sums, int rows) {
  __shared__ double sh[4];
  const double* p = partial + 2 * (int64_t)blockIdx.x * rows;
  double sv = 0.0, si = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    sv += p[2 * r];
    si += p[2 * r + 1];
  }
  sv = block_sum<SumOrder::Sequential, true>(sv, sh);
  si = block_sum<SumOrder::Sequential, true>(si, sh);
  if (threadIdx.x == 0) {
    sums[2 * blockIdx.x] = (float)sv;
    sums[2 * blockIdx.x + 1] = (float)si;
  }
}

bool map_shape_ok(int B, int T, int h, int w, int H, int W) {
  return B > 0 && T > 0 && h > 0 && w > 0 && H > 0 && W > 0 && B <= 65535 && (long long)h * w < (1ll << 30) &&
         (long long)H * W < (1ll << 30) && (long long)B * T * H < (1ll << 31) - 1;
}

}  // namespace

extern "C" int bdv_gradcam_map(const float* act, const float* wgt, float* map, int N, int HW, int C, void* stream) {
  BDV_REQUIRE(act && wgt && map, "bdv_gradcam_map: null pointer");
  BDV_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "bdv_gradcam_map: bad shape N=%d HW=%d C=%d (C must be a multiple of 4)", N, HW, C);
  BDV_REQUIRE(bdv_aligned16(act) && bdv_aligned16(wgt), "bdv_gradcam_map: act and wgt must be 16-byte aligned");
  const int64_t npix = (int64_t)N * HW;
  BDV_REQUIRE((npix + 3) / 4 < (1ll << 31) - 1, "bdv_gradcam_map: %lld pixels exceed one grid dimension", (long long)npix);
  hipLaunchKernelGGL(gradcam_map_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)act,
                     (const float4*)wgt, map, npix, HW, C / 4);
  BDV_LAUNCH_CHECK("bdv_gradcam_map");
  return BDV_OK;
}

extern "C" int bdv_gradcam_minmax(const float* map, int B, int T, int h, int w, int H, int W, float* minmax, void* stream) {
  BDV_REQUIRE(map && minmax, "bdv_gradcam_minmax: null pointer");
  BDV_REQUIRE(map_shape_ok(B, T, h, w, H, W), "bdv_gradcam_minmax: bad shape B=%d T=%d %dx%d -> %dx%d", B, T, h, w, H, W);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(minmax, 0x7F, (size_t)B * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(minmax + B, 0, (size_t)B * sizeof(float), st);
  if (e != hipSuccess) {
    bdv_set_error("bdv_gradcam_minmax: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  const int rows = T * H;
  hipLaunchKernelGGL(gradcam_minmax_kernel, dim3((unsigned)(rows > 128 ? 128 : rows), (unsigned)B), dim3(256), 0, st, map,
                     (unsigned*)minmax, B, T, h, w, H, W);
  BDV_LAUNCH_CHECK("bdv_gradcam_minmax");
  return BDV_OK;
}

extern "C" size_t bdv_gradcam_workspace_bytes(int B, int T, int H) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return (size_t)B * T * H * 2 * sizeof(double);
}

extern "C" int bdv_gradcam_render(const float* map, const float* minmax, int B, int T, int h, int w, int H, int W, float* v_out,
                                  const float* frames_nhwc4, const float* lut, float alpha, const float mean[3], const float std[3],
                                  uint8_t* overlay, const int32_t* box_off, const int32_t* box_off_host, const float* boxes,
                                  const float* boxes_host, int nbox, float* sums, void* workspace, size_t workspace_bytes, void* stream) {
  BDV_REQUIRE(map && minmax, "bdv_gradcam_render: null pointer");
  BDV_REQUIRE(map_shape_ok(B, T, h, w, H, W), "bdv_gradcam_render: bad shape B=%d T=%d %dx%d -> %dx%d", B, T, h, w, H, W);
  BDV_REQUIRE(v_out || overlay || sums, "bdv_gradcam_render: no output requested");
  RenderArgs a;
  a.m = map;
  a.mm = minmax;
  a.v = v_out;
  a.frames = nullptr;
  a.lut = nullptr;
  a.overlay = overlay;
  a.off = nullptr;
  a.boxes = nullptr;
  a.partial = nullptr;
  a.T = T;
  a.h = h;
  a.w = w;
  a.H = H;
  a.W = W;
  a.alpha = 0.f;
  for (int c = 0; c < 3; ++c) a.mean[c] = 0.f, a.std[c] = 1.f;
  if (overlay) {
    BDV_REQUIRE(frames_nhwc4 && lut && mean && std, "bdv_gradcam_render: the overlay needs frames, lut, mean and std");
    BDV_REQUIRE(bdv_aligned16(frames_nhwc4), "bdv_gradcam_render: frames must be 16-byte aligned");
    BDV_REQUIRE(alpha >= 0.f && alpha <= 1.f, "bdv_gradcam_render: alpha %g outside [0, 1]", (double)alpha);
    a.frames = (const float4*)frames_nhwc4;
    a.lut = lut;
    a.alpha = alpha;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean[c], a.std[c] = std[c];
  }
  const long long F = (long long)B * T;
  if (sums) {
    // the offsets and boxes are read by the kernel on the device; every index is checked here, on the host copy, before the launch
    BDV_REQUIRE(box_off && box_off_host && nbox >= 0 && (nbox == 0 || (boxes && boxes_host)),
                "bdv_gradcam_render: the box sums need the offsets and boxes on the device and on the host");
    BDV_REQUIRE(box_off_host[0] == 0, "bdv_gradcam_render: box offsets must start at 0");
    for (long long f = 0; f < F; ++f)
      BDV_REQUIRE(box_off_host[f + 1] >= box_off_host[f], "bdv_gradcam_render: box offsets decrease at frame %lld (%d after %d)", f,
                  box_off_host[f + 1], box_off_host[f]);
    BDV_REQUIRE(box_off_host[F] == nbox, "bdv_gradcam_render: the offsets end at %d, the table has %d boxes", box_off_host[F], nbox);
    for (long long i = 0; i < 4ll * nbox; ++i)
      BDV_REQUIRE(boxes_host[i] == boxes_host[i], "bdv_gradcam_render: box %lld holds a NaN", i / 4);
    BDV_REQUIRE(workspace && workspace_bytes >= bdv_gradcam_workspace_bytes(B, T, H) && (((uintptr_t)workspace) & 7) == 0,
                "bdv_gradcam_render: workspace of %zu bytes, %zu needed (8-byte aligned)", workspace_bytes,
                bdv_gradcam_workspace_bytes(B, T, H));
    a.off = box_off;
    a.boxes = nbox > 0 ? boxes : map;      // never read without a box; any valid pointer
    a.partial = (double*)workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gradcam_render_kernel, dim3((unsigned)(F * H)), dim3(256), 0, st, a);
  BDV_LAUNCH_CHECK("bdv_gradcam_render");
  if (sums) {
    hipLaunchKernelGGL(gradcam_sums_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)workspace, sums, T * H);
    BDV_LAUNCH_CHECK("bdv_gradcam_render (sums)");
  }
  return BDV_OK;
}
