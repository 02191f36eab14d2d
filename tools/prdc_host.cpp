// The arithmetic of the manifold figures (rcdms_amd/csrc/prdc_core.h) on one CPU thread: the same distance, masks, tile geometry,
// column chunks, k-lists and folds as prdc.hip, with loops where the device has workgroups and the dot product summed with k
// ascending.  It is how the core is checked against the numpy model (tests/prdc_oracle.py: the same bits) before a GPU runs it,
// and it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/prdc_host.cpp -o prdc_host
//   prdc_host nx ny d k col_chunks x.raw y.raw
// x.raw / y.raw hold nx * d / ny * d float64 values (the features, widened), dense.  col_chunks: 1 .. 1024, or 0 for the
// library's choice.  Prints six lines, every float with 17 significant digits:
//   counts <precision> <recall> <density> <coverage>      (the int64 numerators)
//   radii2_real <nx values>      radii2_fake <ny values>      fake_count <ny values>      real_hit <nx values>      real_min2 <nx values>
// Exit status 2: bad arguments or an unreadable file.  Every buffer is allocated at its exact size, so that a read or write one
// element outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prdc_core.h"

namespace {

struct KList {
  double v[prdc::LIST];
};

bool read_raw(const char* path, size_t count, std::vector<double>& out) {
  out.assign(count, 0.0);
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  const size_t got = fread(out.data(), sizeof(double), count, fp);
  const bool at_end = fgetc(fp) == EOF;
  fclose(fp);
  return got == count && at_end;
}

double dot(const double* a, const double* b, int d) {
  FR_NO_CONTRACT
  double s = 0.0;
  for (int k = 0; k < d; ++k) s += a[k] * b[k];
  return s;
}

// |row|^2 through fr's fixed sum
std::vector<double> norms2(const std::vector<double>& x, int n, int d) {
  FR_NO_CONTRACT
  std::vector<double> out((size_t)n), part(fr::LANES);
  for (int i = 0; i < n; ++i) {
    const double* row = &x[(size_t)i * d];
    for (int t = 0; t < fr::LANES; ++t) {
      double s = 0.0;
      for (int k = t; k < d; k += fr::LANES) s += row[k] * row[k];
      part[t] = s;
    }
    out[(size_t)i] = fr::tree_sum(part.data());
  }
  return out;
}

// rcdm_knn_radii2: grid (row strips, column chunks), then the merge
std::vector<double> radii2(const std::vector<double>& x, int n, int d, int k, int col_chunks) {
  const std::vector<double> nn = norms2(x, n, d);
  const int T = prdc::tiles(n), chunks = col_chunks ? col_chunks : prdc::default_chunks(T, T);
  std::vector<double> cand((size_t)chunks * n * k), tile((size_t)prdc::TILE * prdc::TILE_LD);
  std::vector<KList> lists((size_t)prdc::THREADS);          // a thread's register list
  for (int ti = 0; ti < T; ++ti)
    for (int c = 0; c < chunks; ++c) {
      int t0, t1;
      prdc::chunk_tiles(T, chunks, c, &t0, &t1);
      for (int t = 0; t < prdc::THREADS; ++t) prdc::list_init(lists[(size_t)t].v, k);
      for (int tj = t0; tj < t1; ++tj) {
        for (int t = 0; t < prdc::THREADS; ++t)
          for (int e = 0; e < prdc::REGS; ++e) {
            int row, col;
            kid::element(t, e, &row, &col);
            const int i = ti * prdc::TILE + row, j = tj * prdc::TILE + col;
            double v = INFINITY;
            if (i < n && j < n && i != j) v = prdc::dist2(nn[(size_t)i], nn[(size_t)j], dot(&x[(size_t)i * d], &x[(size_t)j * d], d));
            tile[(size_t)row * prdc::TILE_LD + col] = v;
          }
        for (int t = 0; t < prdc::THREADS; ++t) {
          const int srow = t / prdc::SEGMENTS, seg = t - srow * prdc::SEGMENTS;
          double(&list)[prdc::LIST] = lists[(size_t)t].v;
          for (int q = 0; q < prdc::SEG_COLS; ++q) prdc::list_insert(list, tile[(size_t)srow * prdc::TILE_LD + seg * prdc::SEG_COLS + q]);
        }
      }
      for (int srow = 0; srow < prdc::TILE; ++srow) {
        const int t = srow * prdc::SEGMENTS;
        double(&list)[prdc::LIST] = lists[(size_t)t].v;
        for (int s = 1; s < prdc::SEGMENTS; ++s)
          for (int p = prdc::LIST - k; p < prdc::LIST; ++p) prdc::list_insert(list, lists[(size_t)(t + s)].v[p]);
        const int i = ti * prdc::TILE + srow;
        if (i < n)
          for (int q = 0; q < k; ++q) cand[((size_t)c * n + i) * k + q] = list[prdc::LIST - k + q];
      }
    }
  std::vector<double> r2((size_t)n);
  for (int i = 0; i < n; ++i) {
    double list[prdc::LIST];
    prdc::list_init(list, k);
    for (int c = 0; c < chunks; ++c)
      for (int q = 0; q < k; ++q) prdc::list_insert(list, cand[((size_t)c * n + i) * k + q]);
    r2[(size_t)i] = prdc::list_kth(list);
  }
  return r2;
}

template <typename T>
void print_line(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (const T& e : v) printf(" %.17g", (double)e);
  printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: prdc_host nx ny d k col_chunks x.raw y.raw\n");
    return 2;
  }
  const int nx = atoi(argv[1]), ny = atoi(argv[2]), d = atoi(argv[3]), k = atoi(argv[4]), col_chunks = atoi(argv[5]);
  if (d < 1 || d > prdc::MAX_DIM || k < 1 || k > prdc::MAX_K || nx < k + 1 || ny < k + 1 || nx > prdc::MAX_N || ny > prdc::MAX_N ||
      col_chunks < 0 || col_chunks > prdc::MAX_CHUNKS) {
    fprintf(stderr, "prdc_host: d is 1..%d, k 1..%d, nx and ny k + 1..%d, col_chunks 0..%d\n", prdc::MAX_DIM, prdc::MAX_K,
            prdc::MAX_N, prdc::MAX_CHUNKS);
    return 2;
  }
  std::vector<double> x, y;
  if (!read_raw(argv[6], (size_t)nx * d, x) || !read_raw(argv[7], (size_t)ny * d, y)) {
    fprintf(stderr, "prdc_host: the feature files must hold exactly %d * %d and %d * %d float64 values\n", nx, d, ny, d);
    return 2;
  }
  const std::vector<double> rx2 = radii2(x, nx, d, k, col_chunks), ry2 = radii2(y, ny, d, k, col_chunks);

  // rcdm_prdc_counts: the sweep over (row strips, column chunks), the fold, the four numerators
  const std::vector<double> nnx = norms2(x, nx, d), nny = norms2(y, ny, d);
  const int TX = prdc::tiles(nx), TY = prdc::tiles(ny), chunks = col_chunks ? col_chunks : prdc::default_chunks(TX, TY);
  std::vector<uint8_t> colcnt((size_t)TX * ny, 0);
  std::vector<double> rowmin((size_t)chunks * nx, INFINITY);
  std::vector<int32_t> rowhit((size_t)chunks * nx, 0);
  for (int ti = 0; ti < TX; ++ti)
    for (int c = 0; c < chunks; ++c) {
      int t0, t1;
      prdc::chunk_tiles(TY, chunks, c, &t0, &t1);
      for (int tj = t0; tj < t1; ++tj) {
        int cnt[prdc::TILE] = {0};
        for (int t = 0; t < prdc::THREADS; ++t)
          for (int e = 0; e < prdc::REGS; ++e) {
            int row, col;
            kid::element(t, e, &row, &col);
            const int i = ti * prdc::TILE + row, j = tj * prdc::TILE + col;
            if (i >= nx || j >= ny) continue;
            const double d2 = prdc::dist2(nnx[(size_t)i], nny[(size_t)j], dot(&x[(size_t)i * d], &y[(size_t)j * d], d));
            cnt[col] += prdc::in_ball(d2, rx2[(size_t)i]) ? 1 : 0;
            rowhit[(size_t)c * nx + i] |= prdc::in_ball(d2, ry2[(size_t)j]) ? 1 : 0;
            double& m = rowmin[(size_t)c * nx + i];
            m = d2 < m ? d2 : m;
          }
        for (int col = 0; col < prdc::TILE; ++col)
          if (tj * prdc::TILE + col < ny) colcnt[(size_t)ti * ny + tj * prdc::TILE + col] = (uint8_t)cnt[col];
      }
    }
  std::vector<int32_t> fake_count((size_t)ny), real_hit((size_t)nx);
  std::vector<double> real_min2((size_t)nx);
  int64_t out[4] = {0, 0, 0, 0};
  for (int j = 0; j < ny; ++j) {
    int s = 0;
    for (int ti = 0; ti < TX; ++ti) s += colcnt[(size_t)ti * ny + j];
    fake_count[(size_t)j] = s;
    out[prdc::PRECISION] += s > 0 ? 1 : 0;
    out[prdc::DENSITY] += s;
  }
  for (int i = 0; i < nx; ++i) {
    double m = INFINITY;
    int h = 0;
    for (int c = 0; c < chunks; ++c) {
      const double w = rowmin[(size_t)c * nx + i];
      m = w < m ? w : m;
      h |= rowhit[(size_t)c * nx + i];
    }
    real_hit[(size_t)i] = h;
    real_min2[(size_t)i] = m;
    out[prdc::RECALL] += h;
    out[prdc::COVERAGE] += prdc::in_ball(m, rx2[(size_t)i]) ? 1 : 0;
  }
  printf("counts %lld %lld %lld %lld\n", (long long)out[0], (long long)out[1], (long long)out[2], (long long)out[3]);
  print_line("radii2_real", rx2);
  print_line("radii2_fake", ry2);
  print_line("fake_count", fake_count);
  print_line("real_hit", real_hit);
  print_line("real_min2", real_min2);
  return 0;
}
