// frechet_core.h — the lane-free arithmetic of the Fréchet distance (include/rcdm.h, "Fréchet distance"): the round-robin
// pairing of a one-sided (Hestenes) Jacobi sweep, the plane rotation with its two rules, the numerical-rank rule of the factor
// step and the fixed-order sum every reduction uses.  Plain C++: frechet.hip runs it on the device, one workgroup per pair,
// and tools/frechet_host.cpp runs the same functions on one CPU thread; tests/frechet_oracle.py restates them in numpy.
//   vectors     "column j" of the matrix under rotation is ROW j of the buffer (contiguous).  `rows` is even: an odd
//               dimension gets one zero row, which rule 2 never lets rotate.
//   pairing     round r = 0 .. rows - 2 of a chess tournament (circle method): player rows - 1 sits still, the others turn.
//               Every pair meets exactly once per sweep, and the rows / 2 pairs of a round are disjoint.
//   rotation    alpha = |wp|^2, beta = |wq|^2, gamma = wp . wq;  zeta = (beta - alpha) / (2 gamma),
//               t = sgn(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t;  wp' = c wp - s wq, wq' = s wp + c wq.
//   rule 1      a pair rotates only if |gamma| > 2^-50 sqrt(alpha) sqrt(beta): it is orthogonal to working precision otherwise.
//   rule 2      a pair rotates only if alpha and beta both exceed (dim 2^-52)^2 x the largest squared norm at the start of the
//               sweep: a vector that is rounding noise of a rank-deficient matrix has no direction worth a rotation, and
//               without this rule such pairs can rotate for ever.
//   rule 3      factor step: a vector with lambda = |w| <= dim 2^-52 lambda_max is set to zero (the numerical rank).
//   sums        LANES partial sums, lane t adding elements t, t + LANES, ... in ascending order from +0.0, then a binary tree
//               (part[t] += part[t + s], s = LANES / 2 .. 1).  The same order on the device (threads and LDS) and on the host.
//   Cholesky    the second way to a factor (rcdm_cholesky_pivoted_f64): a diagonally pivoted, right-looking factorisation in panels of
//               nb columns with an implicit permutation (a done mask and a pivot list; no row or column moves), so that the
//               columns come out as those of P L in the original row order.
//     pivot     step j takes the largest remaining diagonal; the lowest index wins a tie; a NaN never wins (chol_better).
//     cut       the factorisation stops when that diagonal is not above (d 2^-52) x the largest diagonal of the input (taken as
//               at least 0): zero, negative and NaN diagonals stop it the same way (chol_threshold, chol_go).  The rank is the
//               number of steps taken.
//     column    inside a panel the work matrix is left alone: with k over the panel's earlier columns,
//               f[i][j] = (work[p][i] - sum_k f[i][k] f[p][k]) / sqrt(pivot) and the next diagonal of row i is
//               work[i][i] - sum_k f[i][k]^2, the sums in the fixed order above (panel_sum: at most nb <= LANES terms, one per
//               lane, so only the tree's last log2 nb levels add anything but +0.0).
//     update    after a full panel, work -= P P^T for the panel's columns P, accumulated from +0.0 with k ascending on the CPU
//               and on the float64 matrix pipe on the device (whose order inside a k-step of four is its own).
// No expression here may be contracted into an FMA: the model in numpy has none, and the three agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FR_HD __host__ __device__ inline
#else
#define FR_HD inline
#endif
#if defined(__clang__)
#define FR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FR_NO_CONTRACT
#endif

namespace fr {

constexpr int LANES = 256;
constexpr int MAX_DIM = 4096;
constexpr int MAX_SWEEPS = 30;
constexpr double EPS = 0x1p-52;
constexpr double RULE1 = 0x1p-50;

// pair i = 0 .. rows / 2 - 1 of round `round` = 0 .. rows - 2; p < q
FR_HD void pair(int rows, int round, int i, int* p, int* q) {
  const int m = rows - 1;
  int a, b;
  if (i == 0) {
    a = round;
    b = m;
  } else {
    a = (round + i) % m;
    b = (round - i + m) % m;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// one element of the two vectors into the three running sums
FR_HD void accumulate(double a, double b, double& aa, double& bb, double& ab) {
  FR_NO_CONTRACT
  aa += a * a;
  bb += b * b;
  ab += a * b;
}

FR_HD double rule2_threshold(int dim, double max_norm2) {
  FR_NO_CONTRACT
  const double t = (double)dim * EPS;
  return (t * t) * max_norm2;
}

// true: the pair rotates by (c, s)
FR_HD bool rotation(double alpha, double beta, double gamma, double threshold2, double* c, double* s) {
  FR_NO_CONTRACT
  if (!(alpha > threshold2 && beta > threshold2)) return false;                 // rule 2
  if (!(fabs(gamma) > RULE1 * (sqrt(alpha) * sqrt(beta)))) return false;        // rule 1
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  *c = 1.0 / sqrt(1.0 + t * t);
  *s = *c * t;
  return true;
}

FR_HD void rotate(double c, double s, double& a, double& b) {
  FR_NO_CONTRACT
  const double na = c * a - s * b, nb = s * a + c * b;
  a = na;
  b = nb;
}

// rule 3
FR_HD bool keep_column(double lambda, double lambda_max, int dim) {
  FR_NO_CONTRACT
  return lambda > ((double)dim * EPS) * lambda_max;
}

FR_HD double factor_entry(double w, double lambda) { return w / sqrt(lambda); }

// ---- pivoted Cholesky ----
constexpr int CHOL_NB = 16;          // the panel width every caller gets with nb = 0 (profiles/frechet.txt has the measurement)

FR_HD bool chol_nb_ok(int nb) { return nb == 16 || nb == 32 || nb == 64 || nb == 128; }

// true: diagonal v of row i replaces the best so far (bv of row bi; bi < 0: none yet)
FR_HD bool chol_better(double v, int i, double bv, int bi) { return bi < 0 ? v > -INFINITY : (v > bv || (v == bv && i < bi)); }

FR_HD double chol_threshold(int d, double max_diag) {
  FR_NO_CONTRACT
  return ((double)d * EPS) * max_diag;
}

// false: the factorisation stops before this step
FR_HD bool chol_go(double pivot, int index, double threshold) { return index >= 0 && pivot > threshold; }

// fr's fixed-order sum of elem(0 .. cnt - 1), cnt <= NB <= LANES: lane t holds +0.0 + elem(t), the tree's levels above NB / 2 add +0.0
template <int NB, typename E>
FR_HD double panel_sum(int cnt, E elem) {
  FR_NO_CONTRACT
  constexpr int H = NB / 2;
  double v[H];
#if defined(__clang__)
#pragma unroll
#endif
  for (int t = 0; t < H; ++t) {
    const double lo = t < cnt ? elem(t) : 0.0, hi = t + H < cnt ? elem(t + H) : 0.0;
    v[t] = (0.0 + lo) + (0.0 + hi);
  }
#if defined(__clang__)
#pragma unroll
#endif
  for (int s = H / 2; s > 0; s >>= 1) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < H / 2; ++t)
      if (t < s) v[t] += v[t + s];
  }
  return v[0];
}

FR_HD double chol_entry(double work, double dot, double ljj) {
  FR_NO_CONTRACT
  return (work - dot) / ljj;
}

FR_HD double chol_diag(double work, double squares) {
  FR_NO_CONTRACT
  return work - squares;
}

// the binary tree over the LANES partial sums, in place
inline double tree_sum(double* part) {
  for (int s = LANES / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) part[t] += part[t + s];
  return part[0];
}

}  // namespace fr
