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

// the binary tree over the LANES partial sums, in place
inline double tree_sum(double* part) {
  for (int s = LANES / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) part[t] += part[t + s];
  return part[0];
}

}  // namespace fr
