// ssim_core.h — the lane-free arithmetic of rcdm_frame_metrics (include/rcdm.h, "Frame metrics"): the window sums of one
// pixel of one pass, and the SSIM map value made from them.  Plain C++: metrics.hip runs it on the device, one thread per
// (row, byte column) of a tile, and tools/ssim_host.cpp runs the same functions on the CPU over whole images.
//   definition  scikit-image's structural_similarity(a, b, channel_axis=-1, data_range=255), K1 = 0.01, K2 = 0.03, per channel:
//                 ux = F(x), uy = F(y), uxx = F(x x), uyy = F(y y), uxy = F(x y)      F: the window mean (box) or the
//                 vx = cn (uxx - ux ux), vy = cn (uyy - uy uy), vxy = cn (uxy - ux uy)    Gaussian-weighted mean
//                 S  = (2 ux uy + C1)(2 vxy + C2) / ((ux ux + uy uy + C1)(vx + vy + C2))
//               cn = NP / (NP - 1) with NP = win^2 (use_sample_covariance) or 1; the image figure is the mean of S over the
//               pixels whose window lies inside the image.
//   box         the five sums are integers below 2^24; the variances are NP sxx - sx^2 in integers (below 2^31 for win <= 13):
//               nothing cancels in floating point.
//   Gaussian    two separable passes in double over the exact integer products (x x, y y, x y <= 65025), taps in index order.
//   exact 1.0   for x == y the sums of x and y, and so the three second moments, are the same bits; the numerator and the
//               denominator are then the same operations on the same bits — as long as neither side is contracted into an
//               FMA the other side does not get.  map_value is compiled with contraction off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSIM_HD __host__ __device__ inline
#else
#define SSIM_HD inline
#endif

namespace ssim {

constexpr int UNIFORM_WIN = 7;
constexpr int GAUSS_WIN = 11;
constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double C2 = (0.03 * 255.0) * (0.03 * 255.0);

// skimage's cov_norm for a window of win x win pixels
SSIM_HD double cov_norm(int win, int sample_covariance) {
  const double np = (double)(win * win);
  return sample_covariance ? np / (np - 1.0) : 1.0;
}

// First pass, box: the five sums over WIN pixels of one row.  a, b: the first pixel's byte of this channel; step: bytes
// between pixels.  s = (sum x, sum y, sum x x, sum y y, sum x y).
template <int WIN>
SSIM_HD void row_sums_box(const uint8_t* a, const uint8_t* b, int step, int32_t s[5]) {
  int32_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
  for (int i = 0; i < WIN; ++i) {
    const int32_t x = a[i * step], y = b[i * step];
    sx += x;
    sy += y;
    sxx += x * x;
    syy += y * y;
    sxy += x * y;
  }
  s[0] = sx, s[1] = sy, s[2] = sxx, s[3] = syy, s[4] = sxy;
}

// First pass, weighted: the same five quantities, each product an exact integer, weighted by w[0..WIN) in tap order.
template <int WIN>
SSIM_HD void row_sums_weighted(const uint8_t* a, const uint8_t* b, int step, const double* w, double s[5]) {
  double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
  for (int i = 0; i < WIN; ++i) {
    const int32_t x = a[i * step], y = b[i * step];
    const double k = w[i];
    sx += k * (double)x;
    sy += k * (double)y;
    sxx += k * (double)(x * x);
    syy += k * (double)(y * y);
    sxy += k * (double)(x * y);
  }
  s[0] = sx, s[1] = sy, s[2] = sxx, s[3] = syy, s[4] = sxy;
}

// Second pass: quantity q of WIN consecutive rows of first-pass results, h[i * stride] being row i.
template <int WIN>
SSIM_HD int32_t col_sum_box(const int32_t* h, int stride) {
  int32_t s = 0;
  for (int i = 0; i < WIN; ++i) s += h[i * stride];
  return s;
}
template <int WIN>
SSIM_HD double col_sum_weighted(const double* h, int stride, const double* w) {
  double s = 0.0;
  for (int i = 0; i < WIN; ++i) s += w[i] * h[i * stride];
  return s;
}

// S from the five means and the two (co)variance terms; every product and sum is rounded on its own
SSIM_HD double map_value(double ux, double uy, double vx, double vy, double vxy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double pxy = ux * uy, pxx = ux * ux, pyy = uy * uy;
  const double a1 = 2.0 * pxy + C1;
  const double a2 = 2.0 * vxy + C2;
  const double b1 = (pxx + pyy) + C1;
  const double b2 = (vx + vy) + C2;
  const double num = a1 * a2, den = b1 * b2;
  return num / den;
}

// box window: s = the five integer sums over the NP = win^2 pixels
SSIM_HD double map_value_box(const int32_t s[5], int win, double cn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int32_t np = win * win;              // win <= 13: np * np * 255^2 < 2^31, every term below fits int32
  const int32_t sx = s[0], sy = s[1];
  const double inv = 1.0 / (double)np, inv2 = 1.0 / (double)(np * np);   // constants once win is: no division per map value
  const double vx = cn * ((double)(np * s[2] - sx * sx) * inv2);
  const double vy = cn * ((double)(np * s[3] - sy * sy) * inv2);
  const double vxy = cn * ((double)(np * s[4] - sx * sy) * inv2);
  return map_value((double)sx * inv, (double)sy * inv, vx, vy, vxy);
}

// weighted window: u = the five weighted means
SSIM_HD double map_value_weighted(const double u[5], double cn) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double mxx = u[0] * u[0], myy = u[1] * u[1], mxy = u[0] * u[1];
  const double vx = cn * (u[2] - mxx);
  const double vy = cn * (u[3] - myy);
  const double vxy = cn * (u[4] - mxy);
  return map_value(u[0], u[1], vx, vy, vxy);
}

}  // namespace ssim
