// The arithmetic of the kernel distance (rcdms_amd/csrc/kid_core.h) on one CPU thread: the same kernel value, masks, tile
// order, tile weights and fixed-order sums as kid.hip, with loops where the device has workgroups and the dot product summed
// with k ascending.  It is how the core is checked against the numpy model (tests/kid_oracle.py: the same bits) before a GPU
// runs it, and it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/kid_host.cpp -o kid_host
//   kid_host nx ny d subsets m degree gamma coef0 x.raw y.raw [ia.raw ib.raw]
// x.raw / y.raw hold nx * d / ny * d float64 values (the features, widened), dense; ia.raw / ib.raw subsets * m int32 values
// (left out: rows 0 .. m - 1 in every subset).  gamma and coef0 are read with strtod: pass 17 significant digits or a hex float.
// Prints one line per subset: `<Sxx> <Syy> <Sxy> <mmd2>` (17 significant digits).
// Exit status 2: bad arguments, an unreadable file or an index outside its set.  Every buffer is allocated at its exact size,
// so that a read or write one element outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kid_core.h"

namespace {

template <typename T>
bool read_raw(const char* path, size_t count, std::vector<T>& out) {
  out.assign(count, T(0));
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  const size_t got = fread(out.data(), sizeof(T), count, fp);
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

// one block of one subset: rows a[ia[.]] against rows b[ib[.]]
double block_sum(int block, const double* a, const int32_t* ia, const double* b, const int32_t* ib, int m, int d, double gamma,
                 double coef0, int degree) {
  const int T = kid::tiles(m);
  std::vector<double> partials((size_t)T * T, 0.0), part(kid::THREADS);
  for (int ti = 0; ti < T; ++ti)
    for (int tj = 0; tj < T; ++tj) {
      const int weight = kid::tile_weight(block, ti, tj);
      if (weight == 0) continue;
      for (int t = 0; t < kid::THREADS; ++t) {
        double s = 0.0;
        for (int e = 0; e < kid::REGS; ++e) {
          int row, col;
          kid::element(t, e, &row, &col);
          const int i = ti * kid::TILE + row, j = tj * kid::TILE + col;
          if (kid::skipped(block, i, j, m)) continue;
          const int64_t ra = ia ? ia[i] : i, rb = ib ? ib[j] : j;
          s += kid::kernel_value(dot(a + (size_t)ra * d, b + (size_t)rb * d, d), gamma, coef0, degree);
        }
        part[t] = s;
      }
      static_assert(kid::THREADS == fr::LANES, "the tile's tree is fr's");
      const double sum = fr::tree_sum(part.data());
      partials[(size_t)ti * T + tj] = weight == 2 ? 2.0 * sum : sum;
    }
  std::vector<double> lanes(fr::LANES, 0.0);
  for (int t = 0; t < fr::LANES; ++t)
    for (size_t k = t; k < partials.size(); k += fr::LANES) lanes[t] += partials[k];
  return fr::tree_sum(lanes.data());
}

bool in_range(const std::vector<int32_t>& idx, int n) {
  for (int32_t v : idx)
    if (v < 0 || v >= n) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 11 && argc != 13) {
    fprintf(stderr, "usage: kid_host nx ny d subsets m degree gamma coef0 x.raw y.raw [ia.raw ib.raw]\n");
    return 2;
  }
  const int nx = atoi(argv[1]), ny = atoi(argv[2]), d = atoi(argv[3]), subsets = atoi(argv[4]), m = atoi(argv[5]), degree = atoi(argv[6]);
  const double gamma = strtod(argv[7], nullptr), coef0 = strtod(argv[8], nullptr);
  const bool lists = argc == 13;
  if (nx < 1 || ny < 1 || d < 1 || d > kid::MAX_DIM || subsets < 1 || subsets > kid::MAX_SUBSETS || m < 2 || m > kid::MAX_M ||
      degree < 1 || degree > kid::MAX_DEGREE || (!lists && (m > nx || m > ny))) {
    fprintf(stderr, "kid_host: d is 1..%d, m 2..%d (and no more than the rows there are without lists), subsets 1..%d, degree 1..%d\n",
            kid::MAX_DIM, kid::MAX_M, kid::MAX_SUBSETS, kid::MAX_DEGREE);
    return 2;
  }
  std::vector<double> x, y;
  if (!read_raw(argv[9], (size_t)nx * d, x) || !read_raw(argv[10], (size_t)ny * d, y)) {
    fprintf(stderr, "kid_host: the feature files must hold exactly %d * %d and %d * %d float64 values\n", nx, d, ny, d);
    return 2;
  }
  std::vector<int32_t> ia, ib;
  if (lists) {
    if (!read_raw(argv[11], (size_t)subsets * m, ia) || !read_raw(argv[12], (size_t)subsets * m, ib)) {
      fprintf(stderr, "kid_host: the index files must hold exactly %d * %d int32 values\n", subsets, m);
      return 2;
    }
    if (!in_range(ia, nx) || !in_range(ib, ny)) {
      fprintf(stderr, "kid_host: an index lies outside its set\n");
      return 2;
    }
  }
  for (int s = 0; s < subsets; ++s) {
    const int32_t* a = lists ? &ia[(size_t)s * m] : nullptr;
    const int32_t* b = lists ? &ib[(size_t)s * m] : nullptr;
    const double sxx = block_sum(kid::XX, x.data(), a, x.data(), a, m, d, gamma, coef0, degree);
    const double syy = block_sum(kid::YY, y.data(), b, y.data(), b, m, d, gamma, coef0, degree);
    const double sxy = block_sum(kid::XY, x.data(), a, y.data(), b, m, d, gamma, coef0, degree);
    printf("%.17g %.17g %.17g %.17g\n", sxx, syy, sxy, kid::mmd2(sxx, syy, sxy, m));
  }
  return 0;
}
