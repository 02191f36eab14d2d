// The rules of the scores from logits (rcdms_amd/csrc/scores_core.h) on one CPU thread: the same prediction rule, state layout,
// row statistics, split boundaries, chunking and fixed-order sums as scores.hip, with loops where the device has lanes and
// blocks.  It is how the core is checked against the numpy model (tests/scores_oracle.py) before a GPU runs it, and it builds
// with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/scores_host.cpp -o scores_host
//   scores_host labels n C logits.raw labels.raw [thresholds.raw]
//       logits.raw: n * C float32, dense; labels.raw: n * C bytes; thresholds.raw: C float32 (left out: all 0.0).
//       Prints the int64 state, one number per line: n, then tp fp fn per class, then H[t][e] row by row.
//   scores_host isc n C splits logits.raw [order.raw]
//       logits.raw: n * C float64 (the logits, widened), dense; order.raw: n int32 row numbers (left out: the given order).
//       Prints KL of every split, one per line (17 significant digits).
// Exit status 2: bad arguments, an unreadable file or an index outside the rows.  Every buffer is allocated at its exact size,
// so that a read or write one element outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scores_core.h"

#pragma clang fp contract(off)

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

int usage() {
  fprintf(stderr, "usage: scores_host labels n C logits.raw labels.raw [thresholds.raw]\n"
                  "       scores_host isc n C splits logits.raw [order.raw]\n");
  return 2;
}

int labels_main(int argc, char** argv) {
  if (argc != 6 && argc != 7) return usage();
  const int64_t n = atoll(argv[2]);
  const int C = atoi(argv[3]);
  if (n < 1 || n > sc::MAX_N || C < 1 || C > sc::MAX_LABEL_CLASSES) {
    fprintf(stderr, "scores_host: n is 1..2^30, C 1..%d\n", sc::MAX_LABEL_CLASSES);
    return 2;
  }
  std::vector<float> z, thr;
  std::vector<uint8_t> y;
  if (!read_raw(argv[4], (size_t)n * C, z) || !read_raw(argv[5], (size_t)n * C, y) || (argc == 7 && !read_raw(argv[6], (size_t)C, thr))) {
    fprintf(stderr, "scores_host: the files must hold exactly %lld * %d float32, as many bytes, and %d float32\n", (long long)n, C, C);
    return 2;
  }
  std::vector<int64_t> state((size_t)sc::label_state_len(C), 0);
  // block by block as the device goes, each block's counts added to the state: integer sums, any order gives the same
  for (int64_t b = 0; b < sc::label_blocks(n); ++b) {
    const int64_t r0 = b * sc::LABEL_ROWS, r1 = r0 + sc::LABEL_ROWS < n ? r0 + sc::LABEL_ROWS : n;
    state[0] += r1 - r0;
    for (int64_t r = r0; r < r1; ++r) {
      int t = 0, e = 0;
      for (int c = 0; c < C; ++c) {
        const bool p = sc::predicts(z[(size_t)r * C + c], thr.empty() ? 0.0f : thr[c]), l = sc::present(y[(size_t)r * C + c]);
        state[(size_t)sc::class_at(c, sc::TP)] += p && l;
        state[(size_t)sc::class_at(c, sc::FP)] += p && !l;
        state[(size_t)sc::class_at(c, sc::FN)] += !p && l;
        t += p && l;
        e += p != l;
      }
      state[(size_t)sc::hist_at(C, t, e)] += 1;
    }
  }
  for (int64_t v : state) printf("%lld\n", (long long)v);
  return 0;
}

// the sum over the classes of one row: WAVE strided partial sums, then the tree
template <typename F>
double row_sum(int C, F term) {
  double part[sc::WAVE];
  for (int l = 0; l < sc::WAVE; ++l) {
    double s = 0.0;
    for (int c = l; c < C; c += sc::WAVE) s += term(c);
    part[l] = s;
  }
  return sc::wave_tree(part);
}

int isc_main(int argc, char** argv) {
  if (argc != 6 && argc != 7) return usage();
  const int64_t n = atoll(argv[2]);
  const int C = atoi(argv[3]), splits = atoi(argv[4]);
  if (n < 1 || n > sc::MAX_N || C < sc::MIN_CLASSES || C > sc::MAX_CLASSES || splits < 1 || splits > sc::MAX_SPLITS || splits > n) {
    fprintf(stderr, "scores_host: n is 1..2^30, C %d..%d, splits 1..%d and no more than n\n", sc::MIN_CLASSES, sc::MAX_CLASSES, sc::MAX_SPLITS);
    return 2;
  }
  std::vector<double> z;
  std::vector<int32_t> order;
  if (!read_raw(argv[5], (size_t)n * C, z) || (argc == 7 && !read_raw(argv[6], (size_t)n, order))) {
    fprintf(stderr, "scores_host: the files must hold exactly %lld * %d float64 and %lld int32\n", (long long)n, C, (long long)n);
    return 2;
  }
  for (int32_t v : order)
    if (v < 0 || v >= n) {
      fprintf(stderr, "scores_host: an index lies outside the rows\n");
      return 2;
    }
  // launch 1: by position
  std::vector<double> m((size_t)n), logs((size_t)n), h((size_t)n);
  for (int64_t pos = 0; pos < n; ++pos) {
    const double* row = &z[(size_t)(order.empty() ? pos : order[(size_t)pos]) * C];
    double mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmax(mx, row[c]);
    const double ls = log(row_sum(C, [&](int c) { return sc::exp_shifted(row[c], mx); }));
    m[(size_t)pos] = mx;
    logs[(size_t)pos] = ls;
    h[(size_t)pos] = row_sum(C, [&](int c) {
      const double lp = sc::log_prob(row[c], mx, ls);
      return sc::plogp(exp(lp), lp);
    });
  }
  std::vector<double> P((size_t)C), part(fr::LANES);
  for (int k = 0; k < splits; ++k) {
    const int64_t b0 = sc::split_begin(n, splits, k), b1 = sc::split_begin(n, splits, k + 1);
    const double nk = (double)(b1 - b0);
    // launch 2 and the first half of launch 3: chunk sums, then the chunks in order
    double H = 0.0;
    for (int c = 0; c < C; ++c) P[(size_t)c] = 0.0;
    for (int64_t j = 0; j < sc::chunks(b1 - b0); ++j) {
      const int64_t p0 = b0 + j * sc::CHUNK, p1 = p0 + sc::CHUNK < b1 ? p0 + sc::CHUNK : b1;
      double Hc = 0.0;
      for (int64_t pos = p0; pos < p1; ++pos) Hc += h[(size_t)pos];
      H += Hc;
      for (int c = 0; c < C; ++c) {
        double Pc = 0.0;
        for (int64_t pos = p0; pos < p1; ++pos) {
          const double* row = &z[(size_t)(order.empty() ? pos : order[(size_t)pos]) * C];
          Pc += sc::prob(row[c], m[(size_t)pos], logs[(size_t)pos]);
        }
        P[(size_t)c] += Pc;
      }
    }
    for (int t = 0; t < fr::LANES; ++t) {
      double g = 0.0;
      for (int c = t; c < C; c += fr::LANES) g += sc::mean_term(P[(size_t)c], nk);
      part[(size_t)t] = g;
    }
    printf("%.17g\n", sc::kl(H, fr::tree_sum(part.data()), nk));
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  if (!strcmp(argv[1], "labels")) return labels_main(argc, argv);
  if (!strcmp(argv[1], "isc")) return isc_main(argc, argv);
  return usage();
}
