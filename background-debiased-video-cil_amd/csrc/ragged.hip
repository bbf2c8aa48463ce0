// Frame stages for batches whose clips differ in size (the HMDB51 and sth-sthv2 configs: frames 240 high, the width differs from
// video to video).  The clips lie in one packed byte buffer (decode.py: RaggedClips); a per-clip descriptor table says where each
// clip starts and how large its frames are, so that one launch serves the whole batch:
//   bdv_resize_linear_ragged_u8   Resize(-1, S) into a second packed buffer, and MultiScaleCrop + Resize(input_size) into the
//                                 uniform (B, T, S, S, 3) tensor: per output pixel exactly bdv_resize_linear_u8 (resize_linear.h)
//   bdv_crop_normalize_ragged_u8  CenterCrop / ThreeCrop / FiveCrop / TenCrop + Normalize of the val / test pipelines: per output
//                                 value exactly bdv_crop_normalize_u8, the crop offsets depending on each clip's resized size
// Both tables are given on the device (read by the kernel) and on the host (validated before the launch: an out-of-range entry
// would read or write outside the buffers).
#include <algorithm>
#include <utility>
#include <vector>

#include "bdvcil_hip.h"
#include "common.h"
#include "loader_pieces.h"
#include "resize_linear.h"

namespace {

// columns of a clip's row in the resize table
enum { RG_SRC = 0, RG_HS, RG_WS, RG_X0, RG_Y0, RG_BW, RG_BH, RG_DST, RG_HD, RG_WD, RG_COLS };
static_assert(RG_COLS == BDV_RAGGED_RESIZE_COLS, "table width of include/bdvcil_hip.h");

// grid (pixel groups of the LARGEST destination frame of the table, frame over all clips): the body of resize_linear_u8_kernel
// (augment.hip) with the frame's geometry read from its clip's row; blocks beyond their clip's frame exit
__global__ __launch_bounds__(256) void resize_linear_ragged_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                                       uint8_t* __restrict__ dst, int T) {
  const unsigned clip = blockIdx.y / (unsigned)T, t = blockIdx.y - clip * (unsigned)T;
  const int64_t* q = table + (size_t)RG_COLS * clip;
  const int Hs = (int)q[RG_HS], Ws = (int)q[RG_WS], Hd = (int)q[RG_HD], Wd = (int)q[RG_WD];
  const unsigned npix = (unsigned)Hd * (unsigned)Wd;
  const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (p0 >= npix) return;
  const size_t pitch = (size_t)Ws * 3;
  const ResizeBox b = resize_box(src + q[RG_SRC] + ((size_t)t * Hs + (size_t)q[RG_Y0]) * pitch + (size_t)q[RG_X0] * 3, pitch, (int)q[RG_BW],
                                 (int)q[RG_BH], Hd, Wd);
  ResizeGroup g = resize_group(p0, npix, Wd);
  unsigned px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k, g.next(Wd)) px[k] = k < g.cnt ? resize_pixel(b, g.dx, g.dy) : 0u;
  // a clip starts 16-byte aligned; with npix a multiple of 4 every frame of it is a whole number of dwords
  resize_store4(dst + q[RG_DST] + ((size_t)t * npix + p0) * 3, px, g.cnt, (npix & 3u) == 0u);
}

// crop_normalize_kernel (pool_frontend.hip) with the clip's (byte offset, H, W) and its crop table read from memory: one thread =
// one output pixel of one (b, crop), looping over T
__global__ __launch_bounds__(256) void crop_normalize_ragged_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ clips,
                                                                     const int32_t* __restrict__ crops, int ncrops, ClipNorm np,
                                                                     float4* __restrict__ out_nhwc4, float* __restrict__ out_nchw,
                                                                     int B, int T, int ch, int cw) {
#pragma clang fp contract(off)
  const int chw = ch * cw;
  const int64_t total = (int64_t)B * ncrops * chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int p = (int)(i % chw);
    const int bc = (int)(i / chw);
    const int b = bc / ncrops, k = bc - b * ncrops;
    const int oy = p / cw, ox = p - oy * cw;
    const int64_t* d = clips + 3 * (size_t)b;
    const int H = (int)d[1], W = (int)d[2];
    const int32_t* c3 = crops + 3 * (size_t)bc;
    const int sy = c3[1] + oy, sx = c3[0] + (c3[2] ? cw - 1 - ox : ox);
    for (int t = 0; t < T; ++t) {
      const uint8_t* q = src + d[0] + (((int64_t)t * H + sy) * W + sx) * 3;
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = normalize_u8(q[c], np.mean[c], np.inv_std[c]);
      const int64_t f = ((int64_t)b * ncrops + k) * T + t;
      if (out_nhwc4 != nullptr) out_nhwc4[f * chw + p] = make_float4(v[0], v[1], v[2], 0.f);
      if (out_nchw != nullptr) {
        float* o = out_nchw + f * 3 * chw + p;
        o[0] = v[0];
        o[chw] = v[1];
        o[2 * (int64_t)chw] = v[2];
      }
    }
  }
}

bool frame_dims_ok(int64_t h, int64_t w) { return h > 0 && w > 0 && h < (1 << 15) && w < (1 << 15); }

}  // namespace

extern "C" int bdv_resize_linear_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* table, const int64_t* table_host,
                                           int nclips, int T, uint8_t* dst, int64_t dst_bytes, void* stream) {
  const char* me = "bdv_resize_linear_ragged_u8";
  BDV_REQUIRE(src && dst && table && table_host, "%s: null pointer (the table is needed on the device AND on the host: it is validated here)", me);
  BDV_REQUIRE(nclips > 0 && T > 0 && src_bytes > 0 && dst_bytes > 0 && (int64_t)nclips * T <= 65535,
              "%s: bad shape: %d clips of %d frames (at most 65535 frames per call), buffers of %lld and %lld bytes", me, nclips, T,
              (long long)src_bytes, (long long)dst_bytes);
  BDV_REQUIRE(src + src_bytes <= dst || dst + dst_bytes <= src, "%s: the source and destination buffers overlap", me);
  BDV_REQUIRE(bdv_aligned16(src) && bdv_aligned16(dst), "%s: the buffers must be 16-byte aligned", me);
  std::vector<std::pair<int64_t, int64_t>> ranges((size_t)nclips);   // destination (start, clip): sorted below to find overlaps
  int64_t max_pix = 0;
  for (int i = 0; i < nclips; ++i) {
    const int64_t* q = table_host + (size_t)RG_COLS * i;
    BDV_REQUIRE(frame_dims_ok(q[RG_HS], q[RG_WS]) && frame_dims_ok(q[RG_HD], q[RG_WD]),
                "%s: clip %d: bad frame size %lld x %lld -> %lld x %lld", me, i, (long long)q[RG_WS], (long long)q[RG_HS],
                (long long)q[RG_WD], (long long)q[RG_HD]);
    BDV_REQUIRE(q[RG_BW] > 0 && q[RG_BH] > 0 && q[RG_X0] >= 0 && q[RG_Y0] >= 0 && q[RG_X0] + q[RG_BW] <= q[RG_WS] &&
                    q[RG_Y0] + q[RG_BH] <= q[RG_HS],
                "%s: clip %d: box (x %lld, y %lld, w %lld, h %lld) leaves the %lld x %lld frame", me, i, (long long)q[RG_X0],
                (long long)q[RG_Y0], (long long)q[RG_BW], (long long)q[RG_BH], (long long)q[RG_WS], (long long)q[RG_HS]);
    const int64_t sb = (int64_t)T * q[RG_HS] * q[RG_WS] * 3, db = (int64_t)T * q[RG_HD] * q[RG_WD] * 3;
    BDV_REQUIRE((q[RG_SRC] & 15) == 0 && (q[RG_DST] & 15) == 0,
                "%s: clip %d: starts at source byte %lld / destination byte %lld, not both 16-byte aligned", me, i, (long long)q[RG_SRC],
                (long long)q[RG_DST]);
    BDV_REQUIRE(q[RG_SRC] >= 0 && q[RG_SRC] <= src_bytes - sb, "%s: clip %d: source bytes [%lld, %lld) lie outside the buffer of %lld bytes",
                me, i, (long long)q[RG_SRC], (long long)(q[RG_SRC] + sb), (long long)src_bytes);
    BDV_REQUIRE(q[RG_DST] >= 0 && q[RG_DST] <= dst_bytes - db,
                "%s: clip %d: destination bytes [%lld, %lld) lie outside the buffer of %lld bytes", me, i, (long long)q[RG_DST],
                (long long)(q[RG_DST] + db), (long long)dst_bytes);
    ranges[(size_t)i] = {q[RG_DST], (int64_t)i};
    max_pix = std::max(max_pix, q[RG_HD] * q[RG_WD]);
  }
  std::sort(ranges.begin(), ranges.end());
  for (int i = 0; i + 1 < nclips; ++i) {
    const int64_t a = ranges[(size_t)i].second, b = ranges[(size_t)i + 1].second;
    const int64_t* q = table_host + (size_t)RG_COLS * a;
    BDV_REQUIRE(q[RG_DST] + (int64_t)T * q[RG_HD] * q[RG_WD] * 3 <= ranges[(size_t)i + 1].first,
                "%s: clip %lld: its destination bytes overlap those of clip %lld", me, (long long)std::max(a, b), (long long)std::min(a, b));
  }
  const unsigned groups = (unsigned)((max_pix + 3) / 4);   // four pixels per thread
  hipLaunchKernelGGL(resize_linear_ragged_u8_kernel, dim3((groups + 255u) / 256u, (unsigned)(nclips * T)), dim3(256), 0, (hipStream_t)stream,
                     src, table, dst, T);
  BDV_LAUNCH_CHECK("bdv_resize_linear_ragged_u8");
  return BDV_OK;
}

extern "C" int bdv_crop_normalize_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* clips, const int64_t* clips_host,
                                            const int32_t* crops, const int32_t* crops_host, int ncrops, int crop_h, int crop_w,
                                            const float mean[3], const float inv_std[3], float* out_nhwc4, float* out_nchw, int B, int T,
                                            void* stream) {
  const char* me = "bdv_crop_normalize_ragged_u8";
  BDV_REQUIRE(src && clips && clips_host && crops && crops_host && mean && inv_std,
              "%s: null pointer (the tables are needed on the device AND on the host: they are validated here)", me);
  BDV_REQUIRE(out_nhwc4 || out_nchw, "%s: no output requested", me);
  BDV_REQUIRE(ncrops > 0 && ncrops <= BDV_MAX_CROPS, "%s: %d crops (1..%d supported)", me, ncrops, BDV_MAX_CROPS);
  BDV_REQUIRE(B > 0 && T > 0 && crop_h > 0 && crop_w > 0 && src_bytes > 0 && (int64_t)crop_h * crop_w < (1ll << 31) / (int64_t)ncrops,
              "%s: bad shape: %d clips of %d frames, crop %dx%d", me, B, T, crop_h, crop_w);
  BDV_REQUIRE(out_nhwc4 == nullptr || bdv_aligned16(out_nhwc4), "%s: alignment", me);
  for (int b = 0; b < B; ++b) {
    const int64_t* d = clips_host + 3 * (size_t)b;
    BDV_REQUIRE(frame_dims_ok(d[1], d[2]) && crop_h <= d[1] && crop_w <= d[2], "%s: clip %d: bad shape %dx%d crop of %lldx%lld", me, b,
                crop_h, crop_w, (long long)d[1], (long long)d[2]);
    const int64_t sb = (int64_t)T * d[1] * d[2] * 3;
    BDV_REQUIRE(d[0] >= 0 && d[0] <= src_bytes - sb, "%s: clip %d: source bytes [%lld, %lld) lie outside the buffer of %lld bytes", me, b,
                (long long)d[0], (long long)(d[0] + sb), (long long)src_bytes);
    for (int k = 0; k < ncrops; ++k) {
      const int32_t* c = crops_host + 3 * ((size_t)b * ncrops + k);
      BDV_REQUIRE(c[0] >= 0 && c[1] >= 0 && c[0] + crop_w <= d[2] && c[1] + crop_h <= d[1],
                  "%s: clip %d: crop %d at (%d, %d) leaves the %lldx%lld frame", me, b, k, c[0], c[1], (long long)d[1], (long long)d[2]);
    }
  }
  hipLaunchKernelGGL(crop_normalize_ragged_kernel, dim3(bdv_ew_grid((int64_t)B * ncrops * crop_h * crop_w)), dim3(256), 0, (hipStream_t)stream,
                     src, clips, crops, ncrops, clip_norm(mean, inv_std), (float4*)out_nhwc4, out_nchw, B, T, crop_h, crop_w);
  BDV_LAUNCH_CHECK("bdv_crop_normalize_ragged_u8");
  return BDV_OK;
}
