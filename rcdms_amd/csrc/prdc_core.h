// prdc_core.h — the lane-free arithmetic of the k-nearest-neighbour manifold figures (include/rcdm.h, "Manifold figures"):
// improved precision and recall (Kynkaanniemi et al., 2019) and density and coverage (Naeem et al., 2020) over stored feature
// rows.  Plain C++: prdc.hip runs it on the device and tools/prdc_host.cpp runs the same functions on one CPU thread;
// tests/prdc_oracle.py restates them in numpy.
//   inputs      real rows X (nx x d) and generated rows Y (ny x d), float32 or float16, widened exactly; k = nearest_k in
//               1 .. MAX_K; nx, ny >= k + 1.
//   distance    D2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>) in float64, no contraction (dist2).  |a|^2 is summed from the
//               exact products through fr's fixed sum (256 strided partial sums, then the tree); the dot is summed in float64,
//               k ascending on the CPU, the matrix pipe's own order on the device.  Every comparison is made on SQUARED
//               distances: there is no square root anywhere.
//   radius      rX2[i] = the k-th smallest of { D2(X_i, X_j) : j != i }, with multiplicity.  The exclusion goes by POSITION, as
//               KID's diagonal mask does: a repeated row is its twin's neighbour at distance 0.  rY2 the same over Y.
//   balls       closed (<=) in all four figures (in_ball):
//                 fake_count[j] = #{ i : D2(X_i, Y_j) <= rX2[i] }
//                 real_hit[i]   = 1 if some j has D2(X_i, Y_j) <= rY2[j], else 0
//                 real_min2[i]  = min_j D2(X_i, Y_j)
//   figures     precision = #{ j : fake_count[j] > 0 } / ny          recall   = sum_i real_hit[i] / nx
//               density   = sum_j fake_count[j] / (k ny)              coverage = #{ i : real_min2[i] <= rX2[i] } / nx
//               The four numerators are int64 (PRECISION, RECALL, DENSITY, COVERAGE of out[4]); the divisions are the caller's,
//               once, in float64.
//   k-list      LIST = MAX_K sorted values; list_init puts -inf into the first LIST - k places and +inf into the rest, so that
//               after any number of list_insert calls list[LIST - 1] is the k-th smallest value seen (+inf while fewer than k
//               were seen) and every index is a compile-time constant: the list lives in registers on the device.
//   reduction   the set is cut into TILE x TILE tiles of kid's geometry (kid::element: the float64 matrix pipe's C/D map, four
//               waves per tile).  Positions outside the set and the position-diagonal of the radius sweep are set to +inf (counts:
//               skipped) in the epilogue — a padded row enters the matrix pipe as the zero vector, which is a real point near
//               a centred cloud: zero operands mask nothing.  The tile columns are dealt to `chunks` column chunks
//               (chunk_tiles); every chunk keeps k candidates per row, a second launch merges them.  Counts, ors and minima
//               are folded per tile and then over the tiles: integer sums, ors and minima, so any order gives the same bits.
//   bound       |D2^ - D2| <= dist2_bound = 2^-53 (d + 2) (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|), to first order, for ANY
//               evaluation inside the rules:  each norm is d exact non-negative products in some order, (d - 1) u |.|^2; their
//               sum one rounding; the dot (d - 1) u sum |a_k b_k|, its doubling exact; the difference one rounding on a value of
//               at most |a|^2 + |b|^2 + 2 sum |a_k b_k|; the clamp at 0 moves towards the true value, which is >= 0.  An order
//               statistic moves by no more than the largest error of its inputs, so a radius is within the largest bound of
//               its row.
// No expression here may be contracted into an FMA.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kid_core.h"

namespace prdc {

constexpr int MAX_K = 16;
constexpr int MAX_N = 65536;              // rows of one set
constexpr int MAX_DIM = fr::MAX_DIM;      // d
constexpr int MAX_CHUNKS = 1024;          // column chunks a caller may force
constexpr int TILE = kid::TILE;
constexpr int THREADS = kid::THREADS;
constexpr int REGS = kid::REGS;
constexpr int LIST = MAX_K;
constexpr int TILE_LD = TILE + 1;         // doubles per row of the LDS tile of the radius sweep: a thread's row walk hits every bank once
constexpr int SEGMENTS = THREADS / TILE;  // threads that share one row of the tile in the radius sweep, SEG_COLS columns each
constexpr int SEG_COLS = TILE / SEGMENTS;
constexpr int FILL_CUS = 256;             // the chunk count the library chooses fills this many compute units,
constexpr int FILL_WGS = 8;               // each with this many workgroups: a unit holds three at once (profiles/prdc.txt)
constexpr int PRECISION = 0, RECALL = 1, DENSITY = 2, COVERAGE = 3;      // the places of the numerators in out[4]

FR_HD int tiles(int n) { return kid::tiles(n); }

// the column chunks the library chooses for `strips` row strips over `col_tiles` tile columns
FR_HD int default_chunks(int strips, int col_tiles) {
  const int want = (FILL_CUS * FILL_WGS + strips - 1) / strips;
  return want < 1 ? 1 : want > col_tiles ? col_tiles : want;
}

// tile columns [*t0, *t1) of chunk c out of `chunks`; empty for a chunk beyond the tiles
FR_HD void chunk_tiles(int col_tiles, int chunks, int c, int* t0, int* t1) {
  const int per = (col_tiles + chunks - 1) / chunks;
  const int a = c * per, b = a + per;
  *t0 = a < col_tiles ? a : col_tiles;
  *t1 = b < col_tiles ? b : col_tiles;
}

FR_HD double dist2(double na, double nb, double dot) {
  FR_NO_CONTRACT
  const double t = (na + nb) - 2.0 * dot;
  return t > 0.0 ? t : 0.0;
}

// the closed ball: the comparison of fake_count (r2 = rX2[i]), of real_hit (r2 = rY2[j]) and of coverage (d2 = real_min2[i])
FR_HD bool in_ball(double d2, double r2) { return d2 <= r2; }

FR_HD double dist2_bound(double na, double nb, double absdot, int d) {
  FR_NO_CONTRACT
  return 0x1p-53 * ((double)(d + 2) * ((na + nb) + 2.0 * absdot));
}

FR_HD void list_init(double (&list)[LIST], int k) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int p = 0; p < LIST; ++p) list[p] = p < LIST - k ? -INFINITY : INFINITY;
}

// keeps the LIST smallest of the list and v, ascending
FR_HD void list_insert(double (&list)[LIST], double v) {
  if (!(v < list[LIST - 1])) return;
#if defined(__clang__)
#pragma unroll
#endif
  for (int p = LIST - 1; p > 0; --p) list[p] = v < list[p - 1] ? list[p - 1] : (v < list[p] ? v : list[p]);
  list[0] = v < list[0] ? v : list[0];
}

FR_HD double list_kth(const double (&list)[LIST]) { return list[LIST - 1]; }

}  // namespace prdc
