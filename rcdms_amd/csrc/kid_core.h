// kid_core.h — the lane-free arithmetic of the kernel distance (include/rcdm.h, "Kernel distance"): the unbiased squared maximum
// mean discrepancy under a polynomial kernel over subsets of stored feature rows (KID; Binkowski et al., Demystifying MMD GANs,
// 2018).  Plain C++: kid.hip runs it on the device and tools/kid_host.cpp runs the same functions on one CPU thread;
// tests/kid_oracle.py restates them in numpy.
//   kernel      k(x, y) = (gamma <x, y> + c)^p, p an integer in 1 .. 8.
//   one subset  index lists ia[0..m) into the rows of X and ib[0..m) into the rows of Y, m >= 2:
//                 Sxx = sum over POSITIONS i != j of k(x_ia[i], x_ia[j]), Syy the same over Y, Sxy = sum over all i, j of
//                 k(x_ia[i], y_ib[j]);  mmd2 = (Sxx / (m (m - 1)) + Syy / (m (m - 1))) - 2 (Sxy / (m m)), in that order in float64,
//                 m (m - 1) and m m formed in int64 and converted once.  The diagonal mask goes by position, not by row number:
//                 a list with a repeated row is well defined.
//   KID         the mean of mmd2 over the subsets and their population standard deviation (ddof = 0), taken on the host.
//   arithmetic  float32 / float16 features are widened exactly, so every product of the dot is exact in float64; the dot is
//               summed in float64; t = fl(fl(gamma dot) + c) with no contraction; k = ((t t) t) ..., left to right.
//   reduction   every block (xx, yy, xy) of a subset is cut into TILE x TILE tiles, tile (ti, tj) holding positions
//               i = TILE ti + row, j = TILE tj + col.  One workgroup of THREADS threads owns a tile; thread t holds the REGS
//               elements element(t, 0 .. REGS - 1) (the float64 matrix pipe's C/D map of a 2 x 2 arrangement of 16 x 16 results
//               per wave, four waves per tile).
//                 1. a thread adds its elements in register order e = 0 .. REGS - 1 from +0.0; elements outside the subset
//                    (i >= m or j >= m) and the masked diagonal of a symmetric block are SKIPPED — a padded row that enters
//                    the matrix pipe as 0.0 has k = c^p != 0, so zero operands mask nothing;
//                 2. the THREADS thread sums go through the binary tree part[t] += part[t + s], s = THREADS / 2 .. 1;
//                 3. a symmetric block is computed from its upper-triangle tiles only: tile (ti, tj) with tj > ti counts
//                    twice (weight 2, exact), the diagonal tiles once, tiles with tj < ti are not computed and their
//                    partial is +0.0 (tile_weight);
//                 4. the tiles(m)^2 tile partials of one (subset, block), in the order ti tiles(m) + tj, go through fr's fixed
//                    sum (frechet_core.h: 256 strided partial sums, then the same tree) in a second launch, which also forms
//                    mmd2.
//               No atomics anywhere: the same input gives the same bits.  The order INSIDE a dot product is the only freedom:
//               k ascending on the CPU, the matrix pipe's own on the device.
//   chain(m)    the longest chain of additions of steps 1 - 4, the D of the error bound
//               |mmd2^ - mmd2| <= 2^-53 (p (d + 2) + D + 4) s  (tests/kid_oracle.py, `bound`).
// No expression here may be contracted into an FMA.
#pragma once
#include <stdint.h>

#include "frechet_core.h"

namespace kid {

constexpr int MAX_DIM = fr::MAX_DIM;      // d
constexpr int MAX_M = 65536;              // rows of one subset
constexpr int MAX_SUBSETS = 65535;
constexpr int MAX_DEGREE = 8;
constexpr int TILE = 64;
constexpr int THREADS = 256;
constexpr int REGS = 16;
constexpr int XX = 0, YY = 1, XY = 2;     // the blocks, and their places in out[subset][0 .. 2]

FR_HD int tiles(int m) { return (m + TILE - 1) / TILE; }

// element e = 0 .. REGS - 1 of thread t = 0 .. THREADS - 1: its row and column inside the tile.  Wave w = t / 64 owns the 32 x 32
// quarter at ((w >> 1) 32, (w & 1) 32); e = (u, v, r) = (e >> 3, (e >> 2) & 1, e & 3) is result r of the 16 x 16 product (u, v),
// row (lane >> 4) + 4 r and column lane & 15 of it.
FR_HD void element(int t, int e, int* row, int* col) {
  const int w = t >> 6, lane = t & 63;
  *row = (w >> 1) * 32 + (e >> 3) * 16 + (lane >> 4) + 4 * (e & 3);
  *col = (w & 1) * 32 + ((e >> 2) & 1) * 16 + (lane & 15);
}

// 0: tile (ti, tj) of the block is not computed; otherwise what its sum counts for
FR_HD int tile_weight(int block, int ti, int tj) { return block == XY || tj == ti ? 1 : tj > ti ? 2 : 0; }

// true: positions (i, j) of the block add nothing
FR_HD bool skipped(int block, int i, int j, int m) { return i >= m || j >= m || (block != XY && i == j); }

FR_HD double kernel_value(double dot, double gamma, double coef0, int degree) {
  FR_NO_CONTRACT
  const double t = gamma * dot + coef0;
  double k = t;
  for (int e = 1; e < degree; ++e) k = k * t;
  return k;
}

FR_HD double mmd2(double sxx, double syy, double sxy, int m) {
  FR_NO_CONTRACT
  const double off = (double)((int64_t)m * (m - 1)), all = (double)((int64_t)m * m);
  return (sxx / off + syy / off) - 2.0 * (sxy / all);
}

// the longest chain of additions behind one of the three sums: REGS in a thread, 8 levels of the tile's tree, the strided
// partial sums of fr's fixed sum over tiles(m)^2 values and the 8 levels of its tree
FR_HD int64_t chain(int m) {
  const int64_t t = tiles(m), n = t * t;
  return REGS + 8 + (n + fr::LANES - 1) / fr::LANES + 8;
}

}  // namespace kid
