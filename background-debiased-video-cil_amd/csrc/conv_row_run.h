// Index map of the "row run" activation path of the plane conv kernels (conv_mfma.hip).
//
// A 3x3 stride-1 tile of BM consecutive flat pixels m0 .. m0 + BM - 1 reads, through the three taps of ONE filter row, the
// BM + 2 consecutive flat pixels m0 - 1 .. m0 + BM of one (shifted) image row sequence: the "run".  Run entry j is pixel
// m0 - 1 + j; output pixel i reads the entries i, i + 1, i + 2 (column offsets -1, 0, +1).  The run is kept in LDS once per filter
// row; a tap is a row offset of -1 / 0 / +1 around the centre row of the output pixel.  An entry whose column offset leaves the
// image (w = 0 reading -1, w = W - 1 reading +1) must read zeros: between two entries that belong to different image rows one
// all-zero SEPARATOR row is reserved in the LDS image.  It is the right pad of one image row and the left pad of the next.
//
// With c0 = column of entry 0, entry j starts a new image row iff (c0 + j) % W == 0 and j > 0, so
//   lds_row(j)  = j + (c0 + j) / W                         (entries stay in order, one row skipped per image-row start)
//   separators  = the rows no entry maps to: sep_row(k), k = 1 .. num_sep, in front of the k-th image-row start
//   rows in use = lds_row(BM + 1) + 1 = BM + 2 + num_sep  <=  rows_bound(BM, W)
// Plain integer functions, checked exhaustively on the host (tests/test_conv_row_run_cpu.py).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BDV_RR_HD __host__ __device__
#else
#define BDV_RR_HD
#endif

namespace rowrun {

// column of run entry 0 (pixel m0 - 1; m0 = 0 gives the column W - 1 of the non-existent pixel -1)
BDV_RR_HD constexpr int col0(int m0, int W) { return (m0 + W - 1) % W; }
// LDS row of run entry j, 0 <= j <= BM + 1
BDV_RR_HD constexpr int lds_row(int j, int c0, int W) { return j + (c0 + j) / W; }
// image-row starts inside the run after entry 0 = separator rows of the image
BDV_RR_HD constexpr int num_sep(int bm, int c0, int W) { return (c0 + bm + 1) / W; }
// LDS row of separator k (1 .. num_sep): the row in front of entry k * W - c0
BDV_RR_HD constexpr int sep_row(int k, int c0, int W) { return k * (W + 1) - c0 - 1; }
// rows the image can need for any tile start: BM + 2 entries + at most 1 + BM / W separators (c0 <= W - 1)
BDV_RR_HD constexpr int rows_bound(int bm, int W) { return bm + 3 + bm / W; }
// the geometry test of the kernels: the image of any tile fits `cap` LDS rows
BDV_RR_HD constexpr bool fits(int bm, int W, int cap) { return rows_bound(bm, W) <= cap; }

}  // namespace rowrun
