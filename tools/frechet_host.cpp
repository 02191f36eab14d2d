// The arithmetic of the Fréchet distance (rcdms_amd/csrc/frechet_core.h) on one CPU thread: the same pairing, rotation, rules
// and fixed-order sums as the kernels of frechet.hip, with loops where the device has workgroups.  It is how the core is checked
// against the numpy model (tests/frechet_oracle.py: the same rotation counts per sweep, the same bits) before a GPU runs it, and
// it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/frechet_host.cpp -o frechet_host
//   frechet_host d mu_a.raw cov_a.raw mu_b.raw cov_b.raw
//   frechet_host --pairs rows        the round-robin order of fr::pair alone: rows - 1 lines of rows / 2 pairs `p:q`
//   frechet_host --cholesky d mu_a.raw cov_a.raw mu_b.raw cov_b.raw
//                                    the distance with both factors from the pivoted Cholesky steps of the core (panels of
//                                    fr::CHOL_NB) and the sweeps over the rank_b (rounded up to even) x rank_a block alone; lines
//                                    2 and 3 are then the pivots of the two factorisations, in the order taken
//   frechet_host --cholesky-factor d nb cov.raw f.raw
//                                    one factorisation in panels of nb: prints the rank and the pivots, writes f (d x d float64)
// The files hold d and d * d float64 values, dense.  Prints four lines:
//   `<distance> <mean term> <trace a> <trace b> <sqrt trace> <rank a> <rank b>`      (17 significant digits)
//   the rotations of every sweep of the run over cov a, then of the run over cov b, then of the run over Fb^T Fa
// Exit status 2: bad arguments or an unreadable file; 3: a run did not stop within fr::MAX_SWEEPS sweeps.  Every buffer is
// allocated at its exact size, so that a read or write one element outside it is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frechet_core.h"

namespace {

bool read_raw(const char* path, size_t count, std::vector<double>& out) {
  out.assign(count, 0.0);
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  const size_t got = fread(out.data(), sizeof(double), count, fp);
  const bool at_end = fgetc(fp) == EOF;
  fclose(fp);
  return got == count && at_end;
}

// fr's sum of elem(0 .. len - 1)
template <typename F>
double fixed_sum(int len, F elem) {
  std::vector<double> part(fr::LANES, 0.0);
  for (int t = 0; t < fr::LANES; ++t)
    for (int k = t; k < len; k += fr::LANES) part[t] += elem(k);
  return fr::tree_sum(part.data());
}

double norm2(const double* p, int len) {
  return fixed_sum(len, [&](int k) {
    FR_NO_CONTRACT
    return p[k] * p[k];
  });
}

// sweeps over w[rows][len] until one rotates nothing; false after fr::MAX_SWEEPS
bool jacobi(std::vector<double>& w, int rows, int len, int dim, std::vector<int>& counts) {
  std::vector<double> aa(fr::LANES), bb(fr::LANES), ab(fr::LANES);
  for (int sweep = 0; sweep < fr::MAX_SWEEPS; ++sweep) {
    double mx = 0.0;
    for (int j = 0; j < rows; ++j) mx = fmax(mx, norm2(&w[(size_t)j * len], len));
    const double thr = fr::rule2_threshold(dim, mx);
    int count = 0;
    for (int round = 0; round < rows - 1; ++round)
      for (int i = 0; i < rows / 2; ++i) {
        int p, q;
        fr::pair(rows, round, i, &p, &q);
        double* wp = &w[(size_t)p * len];
        double* wq = &w[(size_t)q * len];
        for (int t = 0; t < fr::LANES; ++t) {
          aa[t] = bb[t] = ab[t] = 0.0;
          for (int k = t; k < len; k += fr::LANES) fr::accumulate(wp[k], wq[k], aa[t], bb[t], ab[t]);
        }
        const double alpha = fr::tree_sum(aa.data()), beta = fr::tree_sum(bb.data()), gamma = fr::tree_sum(ab.data());
        double c, s;
        if (!fr::rotation(alpha, beta, gamma, thr, &c, &s)) continue;
        for (int k = 0; k < len; ++k) fr::rotate(c, s, wp[k], wq[k]);
        ++count;
      }
    counts.push_back(count);
    if (count == 0) return true;
  }
  return false;
}

// cov (d x d) -> f (d x rows), the factor; false when the sweeps do not stop
bool factor(const std::vector<double>& cov, int d, int rows, std::vector<double>& f, int& rank, std::vector<int>& counts) {
  std::vector<double> w((size_t)rows * d, 0.0);
  for (size_t i = 0; i < (size_t)d * d; ++i) w[i] = cov[i];
  if (!jacobi(w, rows, d, d, counts)) return false;
  std::vector<double> lam(rows);
  double lmax = 0.0;
  for (int j = 0; j < rows; ++j) {
    lam[j] = sqrt(norm2(&w[(size_t)j * d], d));
    lmax = fmax(lmax, lam[j]);
  }
  f.assign((size_t)d * rows, 0.0);
  rank = 0;
  for (int j = 0; j < rows; ++j) {
    if (!fr::keep_column(lam[j], lmax, d)) continue;
    ++rank;
    for (int k = 0; k < d; ++k) f[(size_t)k * rows + j] = fr::factor_entry(w[(size_t)j * d + k], lam[j]);
  }
  return true;
}

// cov (d x d) -> f (d x ldf): columns of P L of the diagonally pivoted factorisation, the core's steps with loops where the
// device has threads; the trailing update is the k-ascending product from +0.0, then one subtraction
template <int NB>
void cholesky(const std::vector<double>& cov, int d, std::vector<double>& f, int ldf, int& rank, std::vector<int>& piv) {
  std::vector<double> work(cov), panel((size_t)NB * d), base(d), diag(d), acc((size_t)d * d);
  std::vector<char> done(d, 0);
  f.assign((size_t)d * ldf, 0.0);
  piv.clear();
  rank = 0;
  double thr = 0.0;
  for (int j0 = 0; j0 < d; j0 += NB) {
    const int j1 = j0 + NB < d ? j0 + NB : d;
    for (int i = 0; i < d; ++i) base[i] = diag[i] = work[(size_t)i * d + i];
    for (int j = j0; j < j1; ++j) {
      if (j == 0) {
        double mx = 0.0;
        for (int i = 0; i < d; ++i) mx = fmax(mx, diag[i]);
        thr = fr::chol_threshold(d, mx);
      }
      double bv = 0.0;
      int bi = -1;
      for (int i = 0; i < d; ++i)
        if (!done[i] && fr::chol_better(diag[i], i, bv, bi)) {
          bv = diag[i];
          bi = i;
        }
      if (!fr::chol_go(bv, bi, thr)) return;
      const int p = bi, cnt = j - j0;
      const double ljj = sqrt(bv);
      piv.push_back(p);
      done[p] = 1;
      rank = j + 1;
      const double* pivot = &panel[p];
      for (int i = 0; i < d; ++i) {
        double* mine = &panel[i];
        if (done[i]) {
          mine[(size_t)cnt * d] = i == p ? ljj : 0.0;
          if (i == p) f[(size_t)i * ldf + j] = ljj;
          continue;
        }
        const double dot = fr::panel_sum<NB>(cnt, [&](int k) {
          FR_NO_CONTRACT
          return mine[(size_t)k * d] * pivot[(size_t)k * d];
        });
        const double c = fr::chol_entry(work[(size_t)p * d + i], dot, ljj);
        const double squares = fr::panel_sum<NB>(cnt + 1, [&](int k) {
          FR_NO_CONTRACT
          const double x = k < cnt ? mine[(size_t)k * d] : c;
          return x * x;
        });
        mine[(size_t)cnt * d] = c;
        f[(size_t)i * ldf + j] = c;
        diag[i] = fr::chol_diag(base[i], squares);
      }
    }
    if (j1 == d) break;
    acc.assign((size_t)d * d, 0.0);
    for (int k = 0; k < NB; ++k)
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
          FR_NO_CONTRACT
          acc[(size_t)i * d + j] += panel[(size_t)k * d + i] * panel[(size_t)k * d + j];
        }
    for (size_t e = 0; e < (size_t)d * d; ++e) work[e] -= acc[e];
  }
}

bool cholesky_nb(int nb, const std::vector<double>& cov, int d, std::vector<double>& f, int ldf, int& rank, std::vector<int>& piv) {
  if (nb == 16) cholesky<16>(cov, d, f, ldf, rank, piv);
  else if (nb == 32) cholesky<32>(cov, d, f, ldf, rank, piv);
  else if (nb == 64) cholesky<64>(cov, d, f, ldf, rank, piv);
  else if (nb == 128) cholesky<128>(cov, d, f, ldf, rank, piv);
  else return false;
  return true;
}

void print_counts(const std::vector<int>& c) {
  for (size_t i = 0; i < c.size(); ++i) printf("%s%d", i ? " " : "", c[i]);
  printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "--pairs")) {          // fr::pair alone: one line per round, `p:q` per pair
    const int rows = atoi(argv[2]);
    if (rows < 2 || (rows & 1) || rows > fr::MAX_DIM) {
      fprintf(stderr, "frechet_host: rows is even, 2..%d\n", fr::MAX_DIM);
      return 2;
    }
    for (int round = 0; round < rows - 1; ++round) {
      for (int i = 0; i < rows / 2; ++i) {
        int p, q;
        fr::pair(rows, round, i, &p, &q);
        printf("%s%d:%d", i ? " " : "", p, q);
      }
      printf("\n");
    }
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "--cholesky-factor")) {
    const int d = atoi(argv[2]), nb = atoi(argv[3]);
    if (d < 1 || d > fr::MAX_DIM || !fr::chol_nb_ok(nb)) {
      fprintf(stderr, "frechet_host: d is 1..%d, nb 16, 32, 64 or 128\n", fr::MAX_DIM);
      return 2;
    }
    std::vector<double> cov, f;
    if (!read_raw(argv[4], (size_t)d * d, cov)) {
      fprintf(stderr, "frechet_host: the file must hold exactly %d * %d float64 values\n", d, d);
      return 2;
    }
    std::vector<int> piv;
    int rank = 0;
    cholesky_nb(nb, cov, d, f, d, rank, piv);
    FILE* fp = fopen(argv[5], "wb");
    if (!fp || fwrite(f.data(), sizeof(double), f.size(), fp) != f.size() || fclose(fp) != 0) {
      fprintf(stderr, "frechet_host: cannot write %s\n", argv[5]);
      return 2;
    }
    printf("%d\n", rank);
    print_counts(piv);
    return 0;
  }
  const bool chol = argc == 7 && !strcmp(argv[1], "--cholesky");
  if (chol) {
    --argc;
    ++argv;
  }
  if (argc != 6) {
    fprintf(stderr, "usage: frechet_host [--cholesky] d mu_a.raw cov_a.raw mu_b.raw cov_b.raw | frechet_host --pairs rows | "
                    "frechet_host --cholesky-factor d nb cov.raw f.raw\n");
    return 2;
  }
  const int d = atoi(argv[1]);
  if (d < 1 || d > fr::MAX_DIM) {
    fprintf(stderr, "frechet_host: d is 1..%d\n", fr::MAX_DIM);
    return 2;
  }
  std::vector<double> mu_a, cov_a, mu_b, cov_b;
  if (!read_raw(argv[2], d, mu_a) || !read_raw(argv[3], (size_t)d * d, cov_a) || !read_raw(argv[4], d, mu_b) ||
      !read_raw(argv[5], (size_t)d * d, cov_b)) {
    fprintf(stderr, "frechet_host: the files must hold exactly %d and %d * %d float64 values\n", d, d, d);
    return 2;
  }
  const int rows = d + (d & 1);
  std::vector<double> fa, fb;
  std::vector<int> ca, cb, cm;
  int rank_a = 0, rank_b = 0;
  int mrows = rows, mlen = rows;              // the block of fb^T fa under rotation
  if (chol) {
    cholesky_nb(fr::CHOL_NB, cov_a, d, fa, rows, rank_a, ca);
    cholesky_nb(fr::CHOL_NB, cov_b, d, fb, rows, rank_b, cb);
    mrows = rank_b + (rank_b & 1);
    mlen = rank_a;
  } else if (!factor(cov_a, d, rows, fa, rank_a, ca) || !factor(cov_b, d, rows, fb, rank_b, cb)) {
    return 3;
  }
  double sqrt_trace = 0.0;
  if (mrows > 0 && mlen > 0) {
    // m = fb^T fa, k ascending, one rounding per product and per sum
    std::vector<double> m((size_t)mrows * mlen, 0.0);
    for (int k = 0; k < d; ++k)
      for (int i = 0; i < mrows; ++i)
        for (int j = 0; j < mlen; ++j) {
          FR_NO_CONTRACT
          m[(size_t)i * mlen + j] += fb[(size_t)k * rows + i] * fa[(size_t)k * rows + j];
        }
    if (!jacobi(m, mrows, mlen, d, cm)) return 3;
    std::vector<double> sv(mrows);
    for (int j = 0; j < mrows; ++j) sv[j] = sqrt(norm2(&m[(size_t)j * mlen], mlen));
    sqrt_trace = fixed_sum(mrows, [&](int k) { return sv[k]; });
  }
  const double mean_term = fixed_sum(d, [&](int k) {
    FR_NO_CONTRACT
    const double df = mu_a[k] - mu_b[k];
    return df * df;
  });
  const double trace_a = fixed_sum(d, [&](int k) { return cov_a[(size_t)k * d + k]; });
  const double trace_b = fixed_sum(d, [&](int k) { return cov_b[(size_t)k * d + k]; });
  const double distance = ((mean_term + trace_a) + trace_b) - 2.0 * sqrt_trace;
  printf("%.17g %.17g %.17g %.17g %.17g %d %d\n", distance, mean_term, trace_a, trace_b, sqrt_trace, rank_a, rank_b);
  print_counts(ca);
  print_counts(cb);
  print_counts(cm);
  return 0;
}
