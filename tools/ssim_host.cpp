// The arithmetic of rcdm_frame_metrics (rcdms_amd/csrc/ssim_core.h) on one CPU thread: the same window sums and the same map
// value as the kernels of metrics.hip, over whole images instead of tiles.  It is how the SSIM arithmetic is checked against
// the float64 restatement (tests/ssim_oracle.py) before a GPU runs it, and it builds with sanitizers as it stands (host code
// with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/ssim_host.cpp -o ssim_host
//   ssim_host [--gaussian] [--population] H W a.raw b.raw
// a.raw, b.raw: H * W * 3 bytes each, uint8 HWC RGB, dense.  Prints one line:
//   `<ssim R> <ssim G> <ssim B> <sse R> <sse G> <sse B> <sad R> <sad G> <sad B>`   (the means with 17 significant digits)
// --gaussian: the 11-tap sigma 1.5 window instead of the 7 x 7 box; --population: use_sample_covariance=False.
// Exit status 2: bad arguments, an unreadable file, or an image smaller than the window.  Every buffer is allocated at its
// exact size, so that a read or write one element outside it is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ssim_core.h"

namespace {

bool read_raw(const char* path, size_t bytes, std::vector<uint8_t>& out) {
  out.assign(bytes, 0);
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  const size_t got = fread(out.data(), 1, bytes, fp);
  const bool at_end = fgetc(fp) == EOF;
  fclose(fp);
  return got == bytes && at_end;
}

// mean SSIM of channel c: first pass over every row, second pass down the columns, map values added in row-major order
template <int WIN, bool BOX>
double channel_mean(const uint8_t* a, const uint8_t* b, int H, int W, int c, const double* w, double cn) {
  const int mh = H - WIN + 1, mw = W - WIN + 1;
  std::vector<int32_t> hi(BOX ? (size_t)5 * H * mw : 0);
  std::vector<double> hd(BOX ? 0 : (size_t)5 * H * mw);
  for (int r = 0; r < H; ++r)
    for (int x = 0; x < mw; ++x) {
      const size_t at = ((size_t)r * W + x) * 3 + c;
      if (BOX) {
        int32_t s[5];
        ssim::row_sums_box<WIN>(a + at, b + at, 3, s);
        for (int q = 0; q < 5; ++q) hi[((size_t)q * H + r) * mw + x] = s[q];
      } else {
        double s[5];
        ssim::row_sums_weighted<WIN>(a + at, b + at, 3, w, s);
        for (int q = 0; q < 5; ++q) hd[((size_t)q * H + r) * mw + x] = s[q];
      }
    }
  double sum = 0.0;
  for (int y = 0; y < mh; ++y)
    for (int x = 0; x < mw; ++x) {
      if (BOX) {
        int32_t s[5];
        for (int q = 0; q < 5; ++q) s[q] = ssim::col_sum_box<WIN>(&hi[((size_t)q * H + y) * mw + x], mw);
        sum += ssim::map_value_box(s, WIN, cn);
      } else {
        double s[5];
        for (int q = 0; q < 5; ++q) s[q] = ssim::col_sum_weighted<WIN>(&hd[((size_t)q * H + y) * mw + x], mw, w);
        sum += ssim::map_value_weighted(s, cn);
      }
    }
  return sum / ((double)mh * (double)mw);
}

}  // namespace

int main(int argc, char** argv) {
  bool gaussian = false, sample = true;
  std::vector<const char*> pos;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--gaussian")) gaussian = true;
    else if (!strcmp(argv[i], "--population")) sample = false;
    else pos.push_back(argv[i]);
  }
  if (pos.size() != 4) {
    fprintf(stderr, "usage: ssim_host [--gaussian] [--population] H W a.raw b.raw\n");
    return 2;
  }
  const int H = atoi(pos[0]), W = atoi(pos[1]);
  const int win = gaussian ? ssim::GAUSS_WIN : ssim::UNIFORM_WIN;
  if (H < win || W < win || H > 8192 || W > 8192) {
    fprintf(stderr, "ssim_host: %d x %d: sides are %d..8192 with this window\n", H, W, win);
    return 2;
  }
  std::vector<uint8_t> a, b;
  if (!read_raw(pos[2], (size_t)H * W * 3, a) || !read_raw(pos[3], (size_t)H * W * 3, b)) {
    fprintf(stderr, "ssim_host: each file must hold exactly %d * %d * 3 bytes\n", H, W);
    return 2;
  }
  double w[ssim::GAUSS_WIN], total = 0.0;
  for (int i = 0; i < ssim::GAUSS_WIN; ++i) {
    const double t = (double)(i - ssim::GAUSS_WIN / 2);
    w[i] = exp(-(t * t) / (2.0 * 1.5 * 1.5));
    total += w[i];
  }
  for (int i = 0; i < ssim::GAUSS_WIN; ++i) w[i] /= total;
  const double cn = ssim::cov_norm(win, sample ? 1 : 0);
  double mean[3];
  int64_t sse[3] = {0, 0, 0}, sad[3] = {0, 0, 0};
  for (int c = 0; c < 3; ++c) {
    mean[c] = gaussian ? channel_mean<ssim::GAUSS_WIN, false>(a.data(), b.data(), H, W, c, w, cn)
                       : channel_mean<ssim::UNIFORM_WIN, true>(a.data(), b.data(), H, W, c, w, cn);
    for (size_t p = 0; p < (size_t)H * W; ++p) {
      const int d = (int)a[p * 3 + c] - (int)b[p * 3 + c];
      sse[c] += d * d;
      sad[c] += d < 0 ? -d : d;
    }
  }
  printf("%.17g %.17g %.17g %lld %lld %lld %lld %lld %lld\n", mean[0], mean[1], mean[2], (long long)sse[0], (long long)sse[1],
         (long long)sse[2], (long long)sad[0], (long long)sad[1], (long long)sad[2]);
  return 0;
}
