// Exhaustive host check of the row-run index map (csrc/conv_row_run.h), compiled and run by tests/test_conv_row_run_cpu.py.
// For BM in {64, 128, 256}, every image width W = 1 .. 300 and every column c0 of the run's first entry (= every tile start
// modulo W):
//   * lds_row is strictly increasing (injective, entries stay in order) and starts at 0;
//   * the separator rows are exactly the rows no entry maps to, one in front of every image-row start, never hit by data;
//   * the rows in use are BM + 2 + num_sep <= rows_bound(BM, W), and the bound is reached for some c0;
//   * an output pixel's centre row - 1 / + 1 is its left / right neighbour's row when that neighbour lies in the same image row,
//     and a separator when the pixel sits at w = 0 / w = W - 1;
//   * col0 agrees with the column of pixel m0 - 1 for the tile starts m0 = BM * t.
// Prints "ok <number of (BM, W, c0) cases>" and exits 0, or the first violation and exits 1.
#include <cstdio>
#include <vector>

#include "conv_row_run.h"

#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAIL %s: ", #cond);                          \
      std::printf(__VA_ARGS__);                                 \
      std::printf("\n");                                        \
      return 1;                                                 \
    }                                                           \
  } while (0)

int main() {
  long cases = 0;
  const int bms[3] = {64, 128, 256};
  for (int bm : bms) {
    for (int W = 1; W <= 300; ++W) {
      int max_rows = 0;
      for (int c0 = 0; c0 < W; ++c0, ++cases) {
        const int nsep = rowrun::num_sep(bm, c0, W);
        const int rows = rowrun::lds_row(bm + 1, c0, W) + 1;
        CHECK(rows == bm + 2 + nsep, "bm %d W %d c0 %d: rows %d nsep %d", bm, W, c0, rows, nsep);
        CHECK(rows <= rowrun::rows_bound(bm, W), "bm %d W %d c0 %d: rows %d > bound %d", bm, W, c0, rows, rowrun::rows_bound(bm, W));
        max_rows = rows > max_rows ? rows : max_rows;
        std::vector<int> owner(rows, -1);   // run entry of an LDS row, -1 = no entry, -2 = separator
        CHECK(rowrun::lds_row(0, c0, W) == 0, "bm %d W %d c0 %d: entry 0 at row %d", bm, W, c0, rowrun::lds_row(0, c0, W));
        for (int j = 0; j <= bm + 1; ++j) {
          const int r = rowrun::lds_row(j, c0, W);
          CHECK(r >= 0 && r < rows, "bm %d W %d c0 %d j %d: row %d of %d", bm, W, c0, j, r, rows);
          CHECK(j == 0 || r > rowrun::lds_row(j - 1, c0, W), "bm %d W %d c0 %d j %d: not increasing", bm, W, c0, j);
          CHECK(owner[r] == -1, "bm %d W %d c0 %d j %d: row %d taken", bm, W, c0, j, r);
          owner[r] = j;
        }
        for (int k = 1; k <= nsep; ++k) {
          const int r = rowrun::sep_row(k, c0, W);
          CHECK(r >= 0 && r < rows, "bm %d W %d c0 %d sep %d: row %d of %d", bm, W, c0, k, r, rows);
          CHECK(owner[r] == -1, "bm %d W %d c0 %d sep %d: row %d holds entry %d or a separator", bm, W, c0, k, r, owner[r]);
          owner[r] = -2;
          // the entry behind the separator starts an image row
          CHECK(r + 1 < rows && owner[r + 1] >= 0 && (c0 + owner[r + 1]) % W == 0, "bm %d W %d c0 %d sep %d: row %d not in front of a row start",
                bm, W, c0, k, r);
        }
        for (int r = 0; r < rows; ++r) CHECK(owner[r] != -1, "bm %d W %d c0 %d: row %d is neither entry nor separator", bm, W, c0, r);
        for (int i = 0; i < bm; ++i) {   // output pixel i = run entry i + 1
          const int w = (c0 + i + 1) % W, c = rowrun::lds_row(i + 1, c0, W);
          CHECK(owner[c] == i + 1, "centre");
          CHECK(owner[c - 1] == (w > 0 ? i : -2), "bm %d W %d c0 %d pixel %d (w %d): left row holds %d", bm, W, c0, i, w, owner[c - 1]);
          CHECK(owner[c + 1] == (w < W - 1 ? i + 2 : -2), "bm %d W %d c0 %d pixel %d (w %d): right row holds %d", bm, W, c0, i, w, owner[c + 1]);
        }
      }
      CHECK(max_rows == rowrun::rows_bound(bm, W), "bm %d W %d: bound %d never reached (max %d)", bm, W, rowrun::rows_bound(bm, W), max_rows);
      for (int t = 0; t < W; ++t) {
        const long m0 = (long)bm * t;
        CHECK(rowrun::col0((int)m0, W) == (int)(((m0 - 1) % W + W) % W), "col0(%ld, %d)", m0, W);
      }
    }
  }
  // the fallback bound of the 256x64 tile with 256 + 96 image rows, the last of them not for data: W >= 3 takes the path
  for (int W = 1; W <= 300; ++W)
    CHECK(rowrun::fits(256, W, 256 + 95) == (W >= 3), "fits(256, %d, 351) = %d", W, (int)rowrun::fits(256, W, 256 + 95));
  std::printf("ok %ld\n", cases);
  return 0;
}
