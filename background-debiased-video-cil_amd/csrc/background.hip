// Background extraction: the reference's bg_extraction_tmf (libs/loader/comix_loader.py:148-164) -- per-pixel
// np.median over a video's frames, .astype(uint8), cv2.imwrite as a baseline JPEG with libjpeg-turbo's defaults (quality 95, 4:2:0).
//
//   bdv_temporal_median_u8   (device) ragged batch of frame stacks -> one median frame per video; exactly np.median(...).astype(uint8)
//   bdv_jpeg_forward_u8      (device) RGB -> quantised coefficients: colour conversion, edge replication, h2v2 downsampling, ISLOW
//                            forward DCT and quantisation as libjpeg-turbo does them; the layout bdv_jpeg_entropy_decode produces
//   bdv_jpeg_entropy_encode  (host)   coefficients -> the whole file, byte for byte what libjpeg-turbo writes with its defaults
//
// The Huffman stage is serial per image, so it runs on host threads (the mirror image of the decoder's split in jpeg.hip).
#include <string.h>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "common.h"

namespace {

// ---- temporal median ------------------------------------------------------------------------------------------------------------
// One lane owns 4 consecutive bytes of the frame (aligned dword loads over the F frames when a frame is a whole number of dwords).
// Pass 1 counts the high nibbles, pass 2 the low nibbles of the values whose high nibble is that of the lower middle order
// statistic, so the stack is read twice.  Counters are u16, two positions packed per dword, in LDS at (slot * 256 + lane): a lane
// only touches its own 32 dwords, which all sit in bank (lane % 64) -- no conflicts, no barriers.  For an even count whose two
// middle values have different high nibbles (15 / 16, 127 / 128), the upper one is the smallest value above the lower one's
// nibble bucket, kept as a running minimum in pass 2.
//
// The person-masked median (bdv_temporal_masked_median_u8) is the same scheme with a sample count per byte position: a frame's
// sample is left out of both passes where one of the frame's boxes contains the pixel.  A lane's 4 bytes span pixels a = p0 / 3 and
// a + 1 (the first 3 - p0 % 3 bytes are a's), so a frame costs two containment tests per box; the box rows of a frame are the same
// for the whole wave and come through scalar loads.  Hole fallback: the lanes that own a byte with fewer than min_visible samples
// run the unmasked two passes as well, in the same launch and in the same LDS column, and take those bytes from them -- the
// select against bdv_temporal_median_u8's statistic, narrowed to the waves that hold a hole (no second histogram set, so LDS
// stays at 32 KB per block; no second launch over the whole batch, no flag read back on the host).
constexpr int kMedThreads = 256;

template <bool kAligned>
__device__ __forceinline__ unsigned load4(const unsigned char* __restrict__ p, unsigned nbytes) {
  if constexpr (kAligned) {
    return *reinterpret_cast<const unsigned*>(p);
  } else {
    unsigned v = 0;
    for (unsigned k = 0; k < nbytes; ++k) v |= (unsigned)p[k] << (8 * k);
    return v;
  }
}

// What a lane needs to tell which of its bytes a frame's boxes cover.  box_first is indexed by the frame's number in the batch.
struct LaneMask {
  const int* __restrict__ box_first;
  const int4* __restrict__ boxes;
  int xa, ya, xb, yb;            // pixels a and a + 1
  unsigned bytes_a;              // bit k set: byte k belongs to pixel a
};

// bit k set: byte k of the lane is visible (outside every box) in batch frame fg
__device__ __forceinline__ unsigned visible_bytes(const LaneMask& m, long long fg) {
  const int b0 = __builtin_amdgcn_readfirstlane(m.box_first[fg]), b1 = __builtin_amdgcn_readfirstlane(m.box_first[fg + 1]);
  bool in_a = false, in_b = false;
  for (int b = b0; b < b1; ++b) {
    const int4 r = m.boxes[b];
    in_a |= m.xa >= r.x && m.xa < r.z && m.ya >= r.y && m.ya < r.w;
    in_b |= m.xb >= r.x && m.xb < r.z && m.yb >= r.y && m.yb < r.w;
  }
  return (in_a ? 0u : m.bytes_a) | (in_b ? 0u : ~m.bytes_a & 15u);
}

// The median of each of the lane's 4 byte positions over frames src, src + P, ... (F of them), packed into a dword.  kMasked: only
// over the samples visible_bytes() keeps; n[k] returns their number per byte, and a byte with none gives an arbitrary value.
// h: the lane's LDS column (32 dwords, stride kMedThreads).
template <bool kAligned, bool kMasked>
__device__ __forceinline__ unsigned median4(const unsigned char* __restrict__ src, unsigned P, unsigned nb, int F, unsigned* h,
                                            const LaneMask& m, long long f0, int (&n)[4]) {
#pragma unroll
  for (int s = 0; s < 32; ++s) h[s * kMedThreads] = 0u;

  // pass 1: high nibbles.  Four frames' loads are issued before their counts, to keep several loads in flight per lane.
  int na = 0, nb2 = 0;             // masked: visible samples of pixel a (byte 0 is always its) and of pixel a + 1 (byte 3)
  auto count_hi = [&](unsigned w, int f) {
    unsigned vis = 15u;
    if constexpr (kMasked) {
      vis = visible_bytes(m, f0 + f);
      na += (int)(vis & 1u);
      nb2 += (int)(vis >> 3);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      atomicAdd(h + ((k >> 1) * 16 + ((w >> (8 * k + 4)) & 15u)) * kMedThreads, ((vis >> k) & 1u) << (16 * (k & 1)));
  };
  int f = 0;
  for (; f + 4 <= F; f += 4) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = load4<kAligned>(src + (size_t)(f + j) * P, nb);
#pragma unroll
    for (int j = 0; j < 4; ++j) count_hi(w[j], f + j);
  }
  for (; f < F; ++f) count_hi(load4<kAligned>(src + (size_t)f * P, nb), f);
  unsigned bucket[4], rank[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    n[k] = kMasked ? ((m.bytes_a >> k) & 1u ? na : nb2) : F;
    const int k1 = (n[k] - 1) >> 1;        // rank of the lower middle value (the middle one for an odd count)
    int below = 0, b = 0;
    for (; b < 15; ++b) {
      const int c = (int)((h[((k >> 1) * 16 + b) * kMedThreads] >> (16 * (k & 1))) & 0xffffu);
      if (below + c > k1) break;
      below += c;
    }
    bucket[k] = (unsigned)b;
    rank[k] = (unsigned)(k1 - below);
  }
#pragma unroll
  for (int s = 0; s < 32; ++s) h[s * kMedThreads] = 0u;

  // pass 2: low nibbles inside the chosen bucket, and the smallest value above it
  unsigned above[4] = {256u, 256u, 256u, 256u};
  auto count_lo = [&](unsigned w, int f) {
    unsigned vis = 15u;
    if constexpr (kMasked) vis = visible_bytes(m, f0 + f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned x = (w >> (8 * k)) & 255u, hi = x >> 4, on = (vis >> k) & 1u;
      if (hi > bucket[k] && on) above[k] = x < above[k] ? x : above[k];
      atomicAdd(h + ((k >> 1) * 16 + (x & 15u)) * kMedThreads, hi == bucket[k] ? on << (16 * (k & 1)) : 0u);
    }
  };
  for (f = 0; f + 4 <= F; f += 4) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = load4<kAligned>(src + (size_t)(f + j) * P, nb);
#pragma unroll
    for (int j = 0; j < 4; ++j) count_lo(w[j], f + j);
  }
  for (; f < F; ++f) count_lo(load4<kAligned>(src + (size_t)f * P, nb), f);
  unsigned res = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned below = 0, lo = 0, c = 0;
    for (; lo < 15; ++lo) {
      c = (h[((k >> 1) * 16 + lo) * kMedThreads] >> (16 * (k & 1))) & 0xffffu;
      if (below + c > rank[k]) break;
      below += c;
    }
    if (lo == 15) c = (h[((k >> 1) * 16 + 15) * kMedThreads] >> (16 * (k & 1))) & 0xffffu;
    const unsigned a = (bucket[k] << 4) | lo;
    unsigned med = a;
    if ((n[k] & 1) == 0) {
      unsigned b;
      if (below + c > rank[k] + 1) {           // the upper middle value has the same low nibble
        b = a;
      } else {                                 // the next non-empty low nibble of the bucket, else the smallest value above it
        b = above[k];
        for (unsigned l = lo + 1; l < 16; ++l)
          if ((h[((k >> 1) * 16 + l) * kMedThreads] >> (16 * (k & 1))) & 0xffffu) {
            b = (bucket[k] << 4) | l;
            break;
          }
      }
      med = (a + b) >> 1;                      // numpy: the float64 mean of the two, truncated by astype(uint8)
    }
    res |= (med & 255u) << (8 * k);
  }
  return res;
}

template <bool kAligned>
__device__ __forceinline__ void store4(unsigned char* __restrict__ dst, unsigned res, unsigned nb) {
  if constexpr (kAligned) {
    *reinterpret_cast<unsigned*>(dst) = res;
  } else {
    for (unsigned k = 0; k < nb; ++k) dst[k] = (unsigned char)(res >> (8 * k));
  }
}

template <bool kAligned>
__global__ __launch_bounds__(kMedThreads) void temporal_median_kernel(const unsigned char* __restrict__ frames,
                                                                      const long long* __restrict__ first,
                                                                      const int* __restrict__ counts, unsigned P,
                                                                      unsigned char* __restrict__ out) {
  __shared__ unsigned hist[32 * kMedThreads];
  const unsigned tid = threadIdx.x;
  const unsigned p0 = (blockIdx.x * kMedThreads + tid) * 4u;
  if (p0 >= P) return;
  const unsigned nb = P - p0 < 4u ? P - p0 : 4u;
  const int v = blockIdx.y;
  int n[4];
  const unsigned res = median4<kAligned, false>(frames + (size_t)first[v] * P + p0, P, nb, counts[v], hist + tid, LaneMask{}, 0, n);
  store4<kAligned>(out + (size_t)v * P + p0, res, nb);
}

template <bool kAligned>
__global__ __launch_bounds__(kMedThreads) void temporal_masked_median_kernel(const unsigned char* __restrict__ frames,
                                                                             const long long* __restrict__ first,
                                                                             const int* __restrict__ counts, unsigned P, int W,
                                                                             const int* __restrict__ box_first,
                                                                             const int4* __restrict__ boxes, int min_visible,
                                                                             unsigned char* __restrict__ out,
                                                                             unsigned short* __restrict__ visible) {
  __shared__ unsigned hist[32 * kMedThreads];
  const unsigned tid = threadIdx.x;
  const unsigned p0 = (blockIdx.x * kMedThreads + tid) * 4u;
  if (p0 >= P) return;
  const unsigned nb = P - p0 < 4u ? P - p0 : 4u;
  const int v = blockIdx.y;
  const int F = counts[v];
  const long long f0 = first[v];
  const unsigned char* src = frames + (size_t)f0 * P + p0;
  const unsigned pa = p0 / 3u, na_bytes = 3u - (p0 - pa * 3u);      // pixel a holds the lane's first 1..3 bytes
  LaneMask m;
  m.box_first = box_first;
  m.boxes = boxes;
  m.ya = (int)(pa / (unsigned)W);
  m.xa = (int)(pa - (unsigned)m.ya * (unsigned)W);
  m.yb = (int)((pa + 1u) / (unsigned)W);                            // row H past the last pixel: inside no box
  m.xb = (int)(pa + 1u - (unsigned)m.yb * (unsigned)W);
  m.bytes_a = (1u << na_bytes) - 1u;
  int n[4], nall[4];
  unsigned res = median4<kAligned, true>(src, P, nb, F, hist + tid, m, f0, n);
  unsigned holes = 0;                                                // 0xff in the bytes with fewer than min_visible samples
#pragma unroll
  for (int k = 0; k < 4; ++k) holes |= ((unsigned)k < nb && n[k] < min_visible ? 255u : 0u) << (8 * k);
  if (holes) res = (res & ~holes) | (median4<kAligned, false>(src, P, nb, F, hist + tid, m, f0, nall) & holes);
  store4<kAligned>(out + (size_t)v * P + p0, res, nb);
  // a pixel's count is written by the lane that holds its first byte
  const size_t npix = P / 3u;
  if (na_bytes == 3u) visible[(size_t)v * npix + pa] = (unsigned short)n[0];
  if (p0 + na_bytes < P) visible[(size_t)v * npix + pa + 1u] = (unsigned short)n[3];
}

// ---- JPEG forward stage ---------------------------------------------------------------------------------------------------------
const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU T.81 Annex K tables in natural order (libjpeg's jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl)
const unsigned short kStdQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jpeg_set_quality: the percentage scaling of jpeg_quality_scaling, then jpeg_add_quant_table's rounding (quality 25..100 keeps
// every entry in 1..255, so force_baseline never clips)
void quality_tables(int quality, unsigned short (&qt)[2][64]) {
  const long scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      long q = (kStdQuant[t][i] * scale + 50) / 100;
      qt[t][i] = (unsigned short)(q <= 0 ? 1 : q > 32767 ? 32767 : q);
    }
}

struct FwdGeom {
  int W, H;
  int bw[3], bh[3];              // block grids (MCU-padded), as bdv_jpeg_info
  int bwr, bhr;                  // luma blocks holding image samples: ceil(W / 8) x ceil(H / 8); the rest are dummy blocks
  int ch;                        // chroma rows holding samples: ceil(H / 2)
  long long coef_off[3], coef_count;
  int block_first[3], blocks_total;
  // libjpeg-turbo's quantiser (jcdctmgr.c compute_reciprocal with 16-bit DCTELEM, the SIMD build): per table and coefficient
  // q = ((|x| + corr) * recip) >> shift, sign restored; divisor = qt << 3 (the ISLOW DCT's outputs are scaled up by 8)
  unsigned short recip[2][64], corr[2][64];
  unsigned char shift[2][64];
};

void make_divisors(const unsigned short (&qt)[2][64], FwdGeom& g) {
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const unsigned d = (unsigned)qt[t][i] << 3;      // >= 8: never a power-of-two special case below 2
      int b = 31 - __builtin_clz(d);
      int r = 16 + b;
      unsigned fq = (unsigned)((1ull << r) / d), fr = (unsigned)((1ull << r) % d);
      unsigned c = d / 2;
      if (fr == 0) {
        fq >>= 1;
        --r;
      } else if (fr <= d / 2u) {
        ++c;
      } else {
        ++fq;
      }
      g.recip[t][i] = (unsigned short)fq;
      g.corr[t][i] = (unsigned short)c;
      g.shift[t][i] = (unsigned char)r;
    }
}

__host__ __device__ __forceinline__ int luma_at(const unsigned char* __restrict__ img, const FwdGeom& g, int x, int y) {
  x = x < g.W ? x : g.W - 1;
  y = y < g.H ? y : g.H - 1;
  const unsigned char* p = img + ((size_t)y * g.W + x) * 3;
  return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
}

// jccolor.c rgb_ycc_convert, 16 fraction bits; c = 1: Cb, 2: Cr
__host__ __device__ __forceinline__ int chroma_px(const unsigned char* __restrict__ img, const FwdGeom& g, int x, int y, int c) {
  const unsigned char* p = img + ((size_t)y * g.W + x) * 3;
  const int r = p[0], gg = p[1], b = p[2];
  return c == 1 ? (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16
                : (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jcsample.c h2v2_downsample over the edge-replicated plane (right columns to the block grid, rows to an even count), then the
// last downsampled row repeated to the block grid (jcprep.c expand_bottom_edge)
__host__ __device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ img, const FwdGeom& g, int j, int i, int c) {
  i = i < g.ch ? i : g.ch - 1;
  const int y0 = 2 * i, y1 = 2 * i + 1 < g.H ? 2 * i + 1 : g.H - 1;
  const int x0 = 2 * j < g.W ? 2 * j : g.W - 1, x1 = 2 * j + 1 < g.W ? 2 * j + 1 : g.W - 1;
  const int s = chroma_px(img, g, x0, y0, c) + chroma_px(img, g, x1, y0, c) + chroma_px(img, g, x0, y1, c) + chroma_px(img, g, x1, y1, c);
  return (s + 1 + (j & 1)) >> 2;
}

// jfdctint.c jpeg_fdct_islow: 13-bit constants, PASS1_BITS 2; rows then columns; outputs scaled up by 8
__host__ __device__ __forceinline__ void fdct_1d(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7, int pass) {
  const int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6;
  const int tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = pass == 1 ? 13 - 2 : 13 + 2, rnd = 1 << (sh - 1);
  if (pass == 1) {
    d0 = (tmp10 + tmp11) * 4;
    d4 = (tmp10 - tmp11) * 4;
  } else {
    d0 = (tmp10 + tmp11 + 2) >> 2;
    d4 = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d2 = (z1 + tmp13 * 6270 + rnd) >> sh;
  d6 = (z1 - tmp12 * 15137 + rnd) >> sh;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d7 = (t4 + z1 + z3 + rnd) >> sh;
  d5 = (t5 + z2 + z4 + rnd) >> sh;
  d3 = (t6 + z2 + z3 + rnd) >> sh;
  d1 = (t7 + z1 + z4 + rnd) >> sh;
}

__host__ __device__ __forceinline__ int quantize(int x, int t, int i, const FwdGeom& g) {
  const unsigned a = (unsigned)(x < 0 ? -x : x);
  const unsigned q = ((a + g.corr[t][i]) * (unsigned)g.recip[t][i]) >> g.shift[t][i];
  return x < 0 ? -(int)q : (int)q;
}

// the quantised coefficients of block (bx, by) of component c (which must hold image samples)
__host__ __device__ void forward_block(const unsigned char* __restrict__ img, const FwdGeom& g, int c, int bx, int by, int (&m)[8][8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      m[r][k] = (c == 0 ? luma_at(img, g, bx * 8 + k, by * 8 + r) : chroma_at(img, g, bx * 8 + k, by * 8 + r, c)) - 128;
    fdct_1d(m[r][0], m[r][1], m[r][2], m[r][3], m[r][4], m[r][5], m[r][6], m[r][7], 1);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) fdct_1d(m[0][k], m[1][k], m[2][k], m[3][k], m[4][k], m[5][k], m[6][k], m[7][k], 2);
  const int t = c == 0 ? 0 : 1;
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int k = 0; k < 8; ++k) m[r][k] = quantize(m[r][k], t, r * 8 + k, g);
}

// The stored coefficients of block (bx, by) of component c.  A luma block outside ceil(W/8) x ceil(H/8) is a dummy block
// (jccoefct.c compress_data): AC zero, DC that of the preceding block in MCU order -- the right neighbour copies its left block,
// a bottom dummy row copies the last block of the MCU's upper row, itself possibly a right dummy; both resolve to the real block
// (min(by, bhr - 1), min(2 * (bx / 2) + 1, bwr - 1)).
__host__ __device__ void block_coefs(const unsigned char* __restrict__ img, const FwdGeom& g, int c, int bx, int by, int (&m)[8][8]) {
  if (c == 0 && (bx >= g.bwr || by >= g.bhr)) {
    const int sx = 2 * (bx >> 1) + 1 < g.bwr - 1 ? 2 * (bx >> 1) + 1 : g.bwr - 1, sy = by < g.bhr - 1 ? by : g.bhr - 1;
    forward_block(img, g, 0, sx, sy, m);
    const int dc = m[0][0];
    for (int r = 0; r < 8; ++r)
      for (int k = 0; k < 8; ++k) m[r][k] = 0;
    m[0][0] = dc;
    return;
  }
  forward_block(img, g, c, bx, by, m);
}

// one thread per 8x8 block of the MCU-padded grids of all images; a block's 128 bytes leave as eight 16-byte stores
__global__ __launch_bounds__(256) void jpeg_forward_kernel(const unsigned char* __restrict__ rgb, short* __restrict__ coefs, FwdGeom g, int B) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)g.blocks_total * (unsigned)B) return;
  const int img = (int)(t / (unsigned)g.blocks_total), bi = (int)(t - (unsigned)img * (unsigned)g.blocks_total);
  const int c = bi >= g.block_first[2] ? 2 : bi >= g.block_first[1] ? 1 : 0;
  const int b = bi - g.block_first[c];
  const int by = b / g.bw[c], bx = b - by * g.bw[c];
  int m[8][8];
  block_coefs(rgb + (size_t)img * g.W * g.H * 3, g, c, bx, by, m);
  uint4* d4 = reinterpret_cast<uint4*>(coefs + (size_t)img * g.coef_count + g.coef_off[c] + (size_t)b * 64);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (unsigned)(unsigned short)m[r][2 * k] | ((unsigned)(unsigned short)m[r][2 * k + 1] << 16);
    d4[r] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

int encode_geometry(int width, int height, int quality, bdv_jpeg_info* info, const char* who) {
  BDV_REQUIRE(info != nullptr, "%s: null pointer", who);
  BDV_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "%s: bad image size %d x %d", who, width, height);
  BDV_REQUIRE(quality >= 25 && quality <= 100, "%s: quality %d outside 25..100", who, quality);
  memset(info, 0, sizeof(*info));
  info->width = width;
  info->height = height;
  info->ncomp = 3;
  const int mcux = (width + 15) / 16, mcuy = (height + 15) / 16;
  unsigned short qt[2][64];
  quality_tables(quality, qt);
  long long off = 0;
  for (int c = 0; c < 3; ++c) {
    info->h[c] = info->v[c] = c == 0 ? 2 : 1;
    info->blocks_w[c] = mcux * info->h[c];
    info->blocks_h[c] = mcuy * info->v[c];
    info->down_w[c] = c == 0 ? width : (width + 1) / 2;
    info->down_h[c] = c == 0 ? height : (height + 1) / 2;
    info->coef_offset[c] = off;
    off += (long long)info->blocks_w[c] * info->blocks_h[c] * 64;
    memcpy(info->qt[c], qt[c == 0 ? 0 : 1], sizeof(info->qt[c]));
  }
  info->coef_count = off;
  return BDV_OK;
}

void make_fwd_geom(const bdv_jpeg_info& info, int quality, FwdGeom& g) {
  memset(&g, 0, sizeof(g));
  g.W = info.width;
  g.H = info.height;
  g.bwr = (g.W + 7) / 8;
  g.bhr = (g.H + 7) / 8;
  g.ch = (g.H + 1) / 2;
  int nblk = 0;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = info.blocks_w[c];
    g.bh[c] = info.blocks_h[c];
    g.coef_off[c] = info.coef_offset[c];
    g.block_first[c] = nblk;
    nblk += g.bw[c] * g.bh[c];
  }
  g.blocks_total = nblk;
  g.coef_count = info.coef_count;
  unsigned short qt[2][64];
  quality_tables(quality, qt);
  make_divisors(qt, g);
}

// ---- entropy coding (jchuff.c with the standard tables of jstdhuff.c) ----------------------------------------------------------
const unsigned char kBitsDcLum[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char kBitsDcChr[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char kValDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kBitsAcLum[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const unsigned char kValAcLum[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const unsigned char kBitsAcChr[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char kValAcChr[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct EncTable {
  unsigned code[256];
  unsigned char len[256];
  void build(const unsigned char* bits, const unsigned char* vals) {   // jchuff.c jpeg_make_c_derived_tbl
    memset(len, 0, sizeof(len));
    unsigned c = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++k) {
        code[vals[k]] = c++;
        len[vals[k]] = (unsigned char)l;
      }
      c <<= 1;
    }
  }
};

struct EncTables {
  EncTable dc[2], ac[2];
  EncTables() {
    dc[0].build(kBitsDcLum, kValDc);
    dc[1].build(kBitsDcChr, kValDc);
    ac[0].build(kBitsAcLum, kValAcLum);
    ac[1].build(kBitsAcChr, kValAcChr);
  }
};
const EncTables& enc_tables() {
  static const EncTables t;   // thread-safe initialisation (C++11)
  return t;
}

struct BitWriter {
  std::vector<unsigned char>& out;
  uint64_t acc = 0;
  int n = 0;
  void put(unsigned bits, int k) {   // k <= 26
    acc = (acc << k) | (bits & ((1u << k) - 1));
    n += k;
    while (n >= 8) {
      const unsigned char b = (unsigned char)(acc >> (n - 8));
      out.push_back(b);
      if (b == 0xFF) out.push_back(0);
      n -= 8;
    }
  }
  void flush() {   // jchuff.c flush_bits: pad with 1-bits to a whole byte
    if (n) put(0x7F, 8 - n);
  }
};

inline int nbits_of(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

int encode_block(BitWriter& bw, const short* blk, int& last_dc, const EncTable& dct, const EncTable& act) {
  int diff = blk[0] - last_dc;
  last_dc = blk[0];
  int a = diff < 0 ? -diff : diff;
  int nb = nbits_of(a);
  if (nb > 11) return BDV_EINVAL;
  bw.put(dct.code[nb], dct.len[nb]);
  if (nb) bw.put((unsigned)(diff < 0 ? diff - 1 : diff), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kZigzag[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      bw.put(act.code[0xF0], act.len[0xF0]);
      run -= 16;
    }
    a = v < 0 ? -v : v;
    nb = nbits_of(a);
    if (nb > 10) return BDV_EINVAL;
    const int sym = (run << 4) + nb;
    bw.put(act.code[sym], act.len[sym]);
    bw.put((unsigned)(v < 0 ? v - 1 : v), nb);
    run = 0;
  }
  if (run > 0) bw.put(act.code[0], act.len[0]);
  return BDV_OK;
}

void put16(std::vector<unsigned char>& o, unsigned v) {
  o.push_back((unsigned char)(v >> 8));
  o.push_back((unsigned char)v);
}

void put_dht(std::vector<unsigned char>& o, int cls_id, const unsigned char* bits, const unsigned char* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  o.push_back(0xFF);
  o.push_back(0xC4);
  put16(o, 2 + 1 + 16 + n);
  o.push_back((unsigned char)cls_id);
  o.insert(o.end(), bits, bits + 16);
  o.insert(o.end(), vals, vals + n);
}

thread_local std::vector<unsigned char> g_stream;

int encode_stream(const short* coefs, int width, int height, int quality, std::vector<unsigned char>& o, const char* who) {
  bdv_jpeg_info info;
  if (int e = encode_geometry(width, height, quality, &info, who)) return e;
  o.clear();
  const unsigned char head[] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
  o.insert(o.end(), head, head + sizeof(head));
  for (int t = 0; t < 2; ++t) {
    o.push_back(0xFF);
    o.push_back(0xDB);
    put16(o, 67);
    o.push_back((unsigned char)t);
    for (int i = 0; i < 64; ++i) o.push_back((unsigned char)info.qt[t][kZigzag[i]]);
  }
  const unsigned char sof[] = {0xFF, 0xC0, 0x00, 0x11, 0x08, (unsigned char)(height >> 8), (unsigned char)height, (unsigned char)(width >> 8),
                               (unsigned char)width, 0x03, 0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01};
  o.insert(o.end(), sof, sof + sizeof(sof));
  put_dht(o, 0x00, kBitsDcLum, kValDc);
  put_dht(o, 0x10, kBitsAcLum, kValAcLum);
  put_dht(o, 0x01, kBitsDcChr, kValDc);
  put_dht(o, 0x11, kBitsAcChr, kValAcChr);
  const unsigned char sos[] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00};
  o.insert(o.end(), sos, sos + sizeof(sos));
  const EncTables& T = enc_tables();
  BitWriter bw{o};
  int dc[3] = {0, 0, 0};
  const int mcux = info.blocks_w[1], mcuy = info.blocks_h[1];
  for (int my = 0; my < mcuy; ++my)
    for (int mx = 0; mx < mcux; ++mx) {
      for (int yy = 0; yy < 2; ++yy)
        for (int xx = 0; xx < 2; ++xx) {
          const short* blk = coefs + info.coef_offset[0] + ((size_t)(2 * my + yy) * info.blocks_w[0] + 2 * mx + xx) * 64;
          BDV_REQUIRE(encode_block(bw, blk, dc[0], T.dc[0], T.ac[0]) == BDV_OK, "%s: coefficient out of the baseline range in luma block (%d, %d)",
                      who, 2 * my + yy, 2 * mx + xx);
        }
      for (int c = 1; c < 3; ++c) {
        const short* blk = coefs + info.coef_offset[c] + ((size_t)my * info.blocks_w[c] + mx) * 64;
        BDV_REQUIRE(encode_block(bw, blk, dc[c], T.dc[1], T.ac[1]) == BDV_OK, "%s: coefficient out of the baseline range in chroma block (%d, %d)",
                    who, my, mx);
      }
    }
  bw.flush();
  o.push_back(0xFF);
  o.push_back(0xD9);
  return BDV_OK;
}

}  // namespace

extern "C" int bdv_temporal_median_u8(const uint8_t* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                                      const int64_t* first_host, const int32_t* counts_host, int V, int H, int W, uint8_t* out, void* stream) {
  BDV_REQUIRE(frames && first && counts && first_host && counts_host && out, "bdv_temporal_median_u8: null pointer");
  BDV_REQUIRE(V > 0 && V <= 65535 && H > 0 && W > 0, "bdv_temporal_median_u8: bad batch (V=%d, %d x %d)", V, H, W);
  BDV_REQUIRE((long long)H * W * 3 < (1ll << 31) - 1024, "bdv_temporal_median_u8: frame too large");
  if (int rc = bdv_check_video_runs("bdv_temporal_median_u8", first_host, counts_host, V, total_frames)) return rc;
  const unsigned P = (unsigned)H * (unsigned)W * 3u;
  const bool aligned = (P & 3u) == 0 && (((uintptr_t)frames) & 3) == 0 && (((uintptr_t)out) & 3) == 0;
  const unsigned groups = (P + 3u) / 4u;
  dim3 grid((groups + kMedThreads - 1) / kMedThreads, (unsigned)V);
  hipStream_t s = (hipStream_t)stream;
  if (aligned)
    hipLaunchKernelGGL(temporal_median_kernel<true>, grid, dim3(kMedThreads), 0, s, frames, (const long long*)first, counts, P, out);
  else
    hipLaunchKernelGGL(temporal_median_kernel<false>, grid, dim3(kMedThreads), 0, s, frames, (const long long*)first, counts, P, out);
  BDV_LAUNCH_CHECK("bdv_temporal_median_u8");
  return BDV_OK;
}

extern "C" int bdv_temporal_masked_median_u8(const uint8_t* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                                             const int64_t* first_host, const int32_t* counts_host, int V, int H, int W,
                                             const int32_t* box_first, const int32_t* boxes, const int32_t* box_first_host,
                                             const int32_t* boxes_host, int64_t num_boxes, int min_visible, uint8_t* out,
                                             uint16_t* visible, void* stream) {
  const char* who = "bdv_temporal_masked_median_u8";
  BDV_REQUIRE(frames && first && counts && first_host && counts_host && out && visible && box_first && box_first_host, "%s: null pointer", who);
  BDV_REQUIRE(V > 0 && V <= 65535 && H > 0 && W > 0, "%s: bad batch (V=%d, %d x %d)", who, V, H, W);
  BDV_REQUIRE((long long)H * W * 3 < (1ll << 31) - 1024, "%s: frame too large", who);
  BDV_REQUIRE(min_visible >= 1, "%s: min_visible %d (at least 1)", who, min_visible);
  BDV_REQUIRE(num_boxes >= 0 && num_boxes < (1ll << 31) && (num_boxes == 0 || (boxes && boxes_host)), "%s: bad box table (%lld rows)", who,
              (long long)num_boxes);
  BDV_REQUIRE(num_boxes == 0 || bdv_aligned16(boxes), "%s: boxes must be 16-byte aligned", who);
  if (int rc = bdv_check_video_runs(who, first_host, counts_host, V, total_frames)) return rc;
  BDV_REQUIRE(box_first_host[0] >= 0 && box_first_host[total_frames] <= num_boxes, "%s: box_first spans rows %d..%d of %lld", who,
              box_first_host[0], box_first_host[total_frames], (long long)num_boxes);
  for (int64_t f = 0; f < total_frames; ++f)
    BDV_REQUIRE(box_first_host[f] <= box_first_host[f + 1], "%s: box_first decreases at frame %lld (%d > %d)", who, (long long)f,
                box_first_host[f], box_first_host[f + 1]);
  for (int64_t b = box_first_host[0]; b < box_first_host[total_frames]; ++b) {
    const int32_t* r = boxes_host + 4 * b;
    BDV_REQUIRE(0 <= r[0] && r[0] <= r[2] && r[2] <= W && 0 <= r[1] && r[1] <= r[3] && r[3] <= H,
                "%s: box %lld (%d, %d, %d, %d) is not inside the %d x %d frame", who, (long long)b, r[0], r[1], r[2], r[3], W, H);
  }
  const unsigned P = (unsigned)H * (unsigned)W * 3u;
  const bool aligned = (P & 3u) == 0 && (((uintptr_t)frames) & 3) == 0 && (((uintptr_t)out) & 3) == 0;
  const unsigned groups = (P + 3u) / 4u;
  dim3 grid((groups + kMedThreads - 1) / kMedThreads, (unsigned)V);
  hipStream_t s = (hipStream_t)stream;
  if (aligned)
    hipLaunchKernelGGL(temporal_masked_median_kernel<true>, grid, dim3(kMedThreads), 0, s, frames, (const long long*)first, counts, P, W,
                       box_first, (const int4*)boxes, min_visible, out, visible);
  else
    hipLaunchKernelGGL(temporal_masked_median_kernel<false>, grid, dim3(kMedThreads), 0, s, frames, (const long long*)first, counts, P, W,
                       box_first, (const int4*)boxes, min_visible, out, visible);
  BDV_LAUNCH_CHECK(who);
  return BDV_OK;
}

extern "C" int bdv_jpeg_encode_info(int width, int height, int quality, bdv_jpeg_info* info) {
  return encode_geometry(width, height, quality, info, "bdv_jpeg_encode_info");
}

extern "C" int bdv_jpeg_forward_u8(const uint8_t* rgb, int B, int height, int width, int quality, short* coefs, void* stream) {
  bdv_jpeg_info info;
  if (int e = encode_geometry(width, height, quality, &info, "bdv_jpeg_forward_u8")) return e;
  BDV_REQUIRE(rgb && coefs && B > 0, "bdv_jpeg_forward_u8: null pointer / empty batch");
  BDV_REQUIRE(bdv_aligned16(coefs), "bdv_jpeg_forward_u8: coefs must be 16-byte aligned");
  FwdGeom g;
  make_fwd_geom(info, quality, g);
  const int nblk = g.blocks_total;
  BDV_REQUIRE((long long)nblk * B < (1ll << 31), "bdv_jpeg_forward_u8: batch too large for one launch");
  const unsigned nb = (unsigned)(((long long)nblk * B + 255) / 256);
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, rgb, coefs, g, B);
  BDV_LAUNCH_CHECK("bdv_jpeg_forward_u8");
  return BDV_OK;
}

extern "C" size_t bdv_jpeg_encode_bound(int width, int height) {
  bdv_jpeg_info info;
  if (encode_geometry(width, height, 95, &info, "bdv_jpeg_encode_bound") != BDV_OK) return 0;
  // headers: 623 bytes; a block: at most 11 + 11 + 63 * (16 + 10) bits, every byte of it possibly stuffed
  return 1024 + (size_t)(info.coef_count / 64) * 2 * ((22 + 63 * 26 + 7) / 8);
}

extern "C" int bdv_jpeg_entropy_encode(const short* coefs, int width, int height, int quality, unsigned char* out, size_t capacity, size_t* size) {
  BDV_REQUIRE(coefs && out && size, "bdv_jpeg_entropy_encode: null pointer");
  if (int e = encode_stream(coefs, width, height, quality, g_stream, "bdv_jpeg_entropy_encode")) return e;
  *size = g_stream.size();
  BDV_REQUIRE(g_stream.size() <= capacity, "bdv_jpeg_entropy_encode: %zu-byte output buffer, %zu needed", capacity, g_stream.size());
  memcpy(out, g_stream.data(), g_stream.size());
  return BDV_OK;
}

extern "C" int bdv_jpeg_entropy_encode_batch(const short* coefs, int n, int width, int height, int quality, unsigned char* out, size_t stride,
                                             size_t* sizes, int threads) {
  BDV_REQUIRE(coefs && out && sizes && n > 0, "bdv_jpeg_entropy_encode_batch: null pointer / empty batch");
  BDV_REQUIRE(threads >= 1 && threads <= 256, "bdv_jpeg_entropy_encode_batch: %d threads (1..256)", threads);
  bdv_jpeg_info info;
  if (int e = encode_geometry(width, height, quality, &info, "bdv_jpeg_entropy_encode_batch")) return e;
  std::atomic<int> next(0), failed(0);
  std::mutex mu;
  std::string first_error;
  int first_code = BDV_OK;
  auto worker = [&]() {
    for (int i = next.fetch_add(1); i < n && !failed.load(); i = next.fetch_add(1)) {
      const int e = bdv_jpeg_entropy_encode(coefs + (size_t)i * info.coef_count, width, height, quality, out + (size_t)i * stride, stride, sizes + i);
      if (e != BDV_OK) {
        std::lock_guard<std::mutex> lock(mu);
        if (!failed.exchange(1)) {
          first_code = e;
          first_error = "image " + std::to_string(i) + ": " + bdv_last_error();
        }
      }
    }
  };
  const int nt = threads < n ? threads : n;
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
  if (failed.load()) {
    bdv_set_error("bdv_jpeg_entropy_encode_batch: %s", first_error.c_str());
    return first_code;
  }
  return BDV_OK;
}
