// scores_core.h — the lane-free rules of the figures taken from classifier logits (include/rcdm.h, "Scores from logits"): the
// multi-label counts behind Char-F1 / Frm-Acc and the Inception Score.  Plain C++: scores.hip runs it on the device and
// tools/scores_host.cpp runs the same functions on one CPU thread; tests/scores_oracle.py restates them in numpy.
//   label counts   C = 1 .. 64 classes.  A row predicts class c when logit > threshold[c], strictly, compared in float32 (a
//                  float16 logit widens exactly; a NaN logit predicts 0); a label byte counts as 1 when it is non-zero.
//                  deviation: the StoryGAN lineage rounds sigmoid(x) in float32, which gives 0 for 0 < x <~ 6e-8 where this
//                  rule gives 1.
//     state        int64[1 + 3 C + (C + 1)^2]: n; per class tp, fp, fn (class_at); H[t][e], the number of rows with t true
//                  positives and e = false positives + false negatives (hist_at; t + e <= C, the other bins stay 0).  Integer
//                  sums only: exact, the same bits in any order, two states merge by addition.  Every figure (frame accuracy,
//                  the four F1 averages, Hamming loss, the per-class figures) is a division on the host.
//     launch       a block of THREADS threads owns LABEL_ROWS consecutive rows, one row per lane and pass; the class counts
//                  come from wave ballots, the histogram from an owner scan (thread t alone increments the bins = t mod THREADS):
//                  no atomics.  A second launch adds the blocks' int32 partials into the state.
//   Inception Score  C = 2 .. 4096 classes, `splits` >= 1, N >= splits rows in the given order (or through an order list).
//     row          in float64: m = max z, s = sum_c exp(z_c - m), logs = log s, logp_c = (z_c - m) - logs, p_c = exp(logp_c),
//                  h = sum_c p_c logp_c.  Sums over the classes of a row: WAVE partial sums, lane l adding classes l, l + WAVE,
//                  ... in ascending order from +0.0, then the binary tree part[l] += part[l + s], s = WAVE / 2 .. 1 (wave_tree).
//     split k      positions [k N / splits, (k + 1) N / splits) (integer division), n_k of them, cut into chunks of CHUNK
//                  consecutive positions from the split's first.  P_c = sum of p_c, Hs = sum of h: inside a chunk in ascending
//                  position from +0.0, then the chunk sums in ascending order from +0.0.  p_c is recomputed from (m, logs), by
//                  the same expression: no N x C matrix of probabilities is stored.
//     KL_k         Hs / n_k - sum_c g(P_c / n_k), g(p) = p log p and g(0) = 0; the sum over classes through fr's fixed sum
//                  (frechet_core.h: 256 strided partial sums, then the tree).  The score of the split is exp(KL_k), the
//                  caller's to take, as are the mean and the spread over splits.
//                  This one-pass form equals the definition mean_rows KL(p_row || p_mean).
//   No order above depends on the launch geometry and there are no atomics: the same input gives the same bits.  Non-finite
//   logits give a non-finite score and are not looked for.  exp and log are the platform's (libm here, the device library
//   there): the two agree to within their own errors only, see `bound` in tests/scores_oracle.py.
// No expression here may be contracted into an FMA.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frechet_core.h"

namespace sc {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
// ---- label counts
constexpr int MAX_LABEL_CLASSES = 64;
constexpr int LABEL_ROWS = 256;           // rows of one block of the count launch: a multiple of THREADS (its partials are int32)
constexpr int TP = 0, FP = 1, FN = 2;
// ---- Inception Score
constexpr int MIN_CLASSES = 2;
constexpr int MAX_CLASSES = 4096;
constexpr int MAX_SPLITS = 65535;
constexpr int MAX_CHUNKS_PER_BLOCK = 64;
constexpr int CHUNK = 256;
constexpr int64_t MAX_N = (int64_t)1 << 30;

FR_HD int64_t label_state_len(int C) { return 1 + 3 * (int64_t)C + (int64_t)(C + 1) * (C + 1); }
FR_HD int64_t class_at(int c, int which) { return 1 + 3 * (int64_t)c + which; }
FR_HD int64_t hist_at(int C, int t, int e) { return 1 + 3 * (int64_t)C + (int64_t)t * (C + 1) + e; }
FR_HD int64_t label_blocks(int64_t n) { return (n + LABEL_ROWS - 1) / LABEL_ROWS; }

FR_HD bool predicts(float logit, float threshold) { return logit > threshold; }      // false for a NaN
FR_HD bool present(uint8_t label) { return label != 0; }

FR_HD int64_t split_begin(int64_t n, int splits, int k) { return (int64_t)k * n / splits; }
FR_HD int64_t chunks(int64_t rows) { return (rows + CHUNK - 1) / CHUNK; }
// the chunk slots every split gets in the workspace: the chunks of the longest split
FR_HD int64_t split_slots(int64_t n, int splits) { return chunks((n + splits - 1) / splits); }

FR_HD double exp_shifted(double z, double m) { return exp(z - m); }
FR_HD double log_prob(double z, double m, double logs) {
  FR_NO_CONTRACT
  return (z - m) - logs;
}
FR_HD double prob(double z, double m, double logs) { return exp(log_prob(z, m, logs)); }
FR_HD double plogp(double p, double logp) {
  FR_NO_CONTRACT
  const double v = p * logp;
  return v;
}
// g(P / n_k)
FR_HD double mean_term(double P, double nk) {
  FR_NO_CONTRACT
  const double p = P / nk;
  if (p == 0.0) return 0.0;
  const double v = p * log(p);
  return v;
}
FR_HD double kl(double hsum, double g, double nk) {
  FR_NO_CONTRACT
  const double mean_h = hsum / nk;
  return mean_h - g;
}

inline double wave_tree(double* part) {
  for (int s = WAVE / 2; s > 0; s >>= 1)
    for (int l = 0; l < s; ++l) part[l] += part[l + s];
  return part[0];
}

}  // namespace sc
