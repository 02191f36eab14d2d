// gn_plan.h — the launch geometry and the block reduction of the GroupNorm statistics pass, shared by norm.hip
// (gn_stats_kernel) and igemm.hip (splitk_reduce_gn_kernel: a split-K GEMM / conv whose reduce pass leaves the GroupNorm
// partial statistics of the rows it writes, so that the norm behind it needs no statistics launch of its own).
#pragma once
#include "common.h"

constexpr int GN_U = 8;  // 16-byte loads a thread of the stats / apply kernels keeps in flight

struct GnArgs {
  const f16* x;
  f16* y;
  const float* gamma;
  const float* beta;
  float* partial;  // [samples][groups][splits][3] = (count, mean, M2)
  float* stat;     // [samples][groups][2] = (mean, rstd)
  int samples, P, C, G, cg, CH, RPB, ldx, ldy, splits, rows_per_split;
  float eps;
  int silu;
};

// Geometry of the three-launch form for a descriptor (grid (splits, samples), CH * RPB threads: thread (rl, ch) owns 16-byte
// chunk ch of rows rl + k RPB of its split).  Defined in norm.hip.  gn_three_launch: whether rcdm_groupnorm_silu takes that
// form for this descriptor (not the single-launch kernel of the smallest tensors) — only then do partials exist.
int rcdm_gn_plan(const rcdm_groupnorm_desc* d, GnArgs& a);
bool rcdm_gn_three_launch(const GnArgs& a);

// ---- shifted moments ---------------------------------------------------------------------------------------------------
// Every GroupNorm statistic of the library is formed from SHIFTED sums: a thread accumulates S = sum(x - k) and
// Q = sum((x - k)^2) of each of its columns with the pivot k = the first value it read of that column (its own first row: no
// extra load, and the split-K reduce pass, which produces that row itself, owns the same pivot as the stand-alone statistics
// pass), so the sums are of the size of the column's spread whatever the group's offset is.  The raw form sum(x), sum(x^2),
// M2 = sum(x^2) - sum(x) mean loses (mean / std)^2 2^-24 of the variance: 1 % of rstd at mean / std = 200.  Partial moments
// are combined by the decomposition M2 = sum_i M2_i + sum_i n_i (mean_i - mean)^2 with mean = p + sum_i n_i d_i / n,
// d_i = mean_i - p, around the first part's mean p; the second term is sum n_i d_i^2 - (sum n_i d_i)^2 / n, a sum of the size
// of the means' spread because p is one of them.  One walk over the parts: the LDS reads of the raw-sum form.  Every product
// that feeds a sum is an explicit fma: the kernels that share these helpers must round alike (rcdm_*_gnstat is bit-identical
// to the separate launches).
__device__ __forceinline__ void gn_acc(float& S, float& Q, float f, float k, bool in) {
  const float d = in ? f - k : 0.f;
  S += d;
  Q = __builtin_fmaf(d, d, Q);
}

// (S, Q, k) of m values -> (mean, M2) of those values; m = 0: zeros (weight 0 in every combination)
__device__ __forceinline__ void gn_shifted_moments(float S, float Q, float k, float m, float& mean, float& m2) {
  const float inv = m > 0.f ? __builtin_amdgcn_rcpf(m) : 0.f;
  const float dm = S * inv;
  mean = __builtin_fmaf(S, inv, k);
  m2 = fmaxf(__builtin_fmaf(-dm, S, Q), 0.f);
}

// nrows = base * RPB + rem, 0 <= rem < RPB (nrows < 2^23, RPB >= 1), without the integer-division sequence: the float
// quotient is off by less than one, one correction step makes it exact.  Row-thread rl owns base + (rl < rem) of the rows
// rl, rl + RPB, ...
__device__ __forceinline__ void gn_divmod(int nrows, int RPB, int& base, int& rem) {
  base = (int)((float)nrows * __builtin_amdgcn_rcpf((float)RPB));
  rem = nrows - base * RPB;
  if (rem < 0) { --base; rem += RPB; }
  else if (rem >= RPB) { ++base; rem -= RPB; }
}

__device__ __forceinline__ float gn_rows_of(int rl, int nrows, int RPB) {
  int base, rem;
  gn_divmod(nrows, RPB, base, rem);
  return (float)(base + (rl < rem ? 1 : 0));
}

// The block's per-thread (mean, M2) pairs -> per-column pairs.  part: [thread (r, c)][16] = mean[8], M2[8] of the thread's
// rows of chunk c; cs: [CH][16] in the same layout; thread o of nthreads takes columns o, o + nthreads, ...  Row-thread 0 of a
// chunk owns at least one row (nrows >= 1), so its mean is a pivot from the data.
__device__ __forceinline__ void gn_column_moments(const float* part, float* cs, int CH, int RPB, int nrows, int t, int nthreads) {
  if (nrows <= 0) return;   // an empty split: the caller writes zeros
  int base, rem;
  gn_divmod(nrows, RPB, base, rem);
  const float inv_n = __builtin_amdgcn_rcpf((float)nrows);
  for (int o = t; o < CH * 8; o += nthreads) {
    const int c = o >> 3, e = o & 7;
    const float piv = part[c * 16 + e];
    float a = 0.f, b = 0.f, q = 0.f;   // one walk over the row-threads: sums of n_r d_r, n_r d_r^2 (d_r = mean_r - piv), M2_r
    for (int r = 0; r < RPB; ++r) {
      const float d = part[(r * CH + c) * 16 + e] - piv;
      const float wd = (float)(base + (r < rem ? 1 : 0)) * d;
      a += wd;
      b = __builtin_fmaf(wd, d, b);
      q += part[(r * CH + c) * 16 + 8 + e];
    }
    const float mean = __builtin_fmaf(a, inv_n, piv);
    q += fmaxf(__builtin_fmaf(-(a * inv_n), a, b), 0.f);
    cs[c * 16 + e] = mean;
    cs[c * 16 + 8 + e] = q;
  }
}

// (mean, M2) of the cg columns c0 .. c0 + cg - 1 of `nrows` values each -> the group's (mean, M2); mean_of(c) / m2_of(c) read a
// column's pair
template <class FM, class FQ>
__device__ __forceinline__ void gn_group_moments(FM mean_of, FQ m2_of, int c0, int cg, float nrows, float& mean, float& m2) {
  const float piv = mean_of(c0);
  float a = 0.f, b = 0.f, q = 0.f;   // one walk over the columns: sums of d_c, d_c^2 (d_c = mean_c - piv), M2_c
  for (int c = c0; c < c0 + cg; ++c) {
    const float d = mean_of(c) - piv;
    a += d;
    b = __builtin_fmaf(d, d, b);
    q += m2_of(c);
  }
  const float inv = __builtin_amdgcn_rcpf((float)cg);
  mean = __builtin_fmaf(a, inv, piv);
  m2 = __builtin_fmaf(nrows, fmaxf(__builtin_fmaf(-(a * inv), a, b), 0.f), q);
}

// Tail of a statistics block: per-thread shifted sums (S[e], Q[e] of the thread's 8 columns over its rows r_begin + rl + j RPB,
// pivot k[e]) -> the G group partials (count, mean, M2) of split `sp` of sample `s`.  part: dynamic LDS, (threads + CH) * 16
// floats.  Column moments first (CH * 8 columns, each over the RPB row-threads, spread over the whole block), then the G
// groups: the one-step form (G threads walking RPB * cg entries each) was a 120-read serial tail on 32 threads per block.
// (The [thread][16] layout puts a wave's ds accesses on two banks — SQ_LDS_BANK_CONFLICT several times SQ_ACTIVE_INST_LDS in
// the counters — but a conflict-free value-major layout measured the same kernel times and the same step time, round 5: the
// tail is not on the block's critical path, its one memory round trip is.)
__device__ __forceinline__ void gn_block_partials(const GnArgs& p, float* part, int t, const float (&S)[8], const float (&Q)[8],
                                                  const float (&k)[8], int s, int sp, int nrows) {
  const float m = gn_rows_of(t / p.CH, nrows, p.RPB);
#pragma unroll
  for (int e = 0; e < 8; ++e) gn_shifted_moments(S[e], Q[e], k[e], m, part[t * 16 + e], part[t * 16 + 8 + e]);
  __syncthreads();
  const float* col = part;  // one row-thread per chunk: the per-thread moments ARE the column moments
  if (p.RPB > 1) {
    float* cs = part + blockDim.x * 16;
    gn_column_moments(part, cs, p.CH, p.RPB, nrows, t, blockDim.x);
    col = cs;
    __syncthreads();
  }
  if (t < p.G) {
    float mean = 0.f, m2 = 0.f;
    if (nrows > 0)
      gn_group_moments([&](int c) { return col[(c >> 3) * 16 + (c & 7)]; }, [&](int c) { return col[(c >> 3) * 16 + 8 + (c & 7)]; },
                       t * p.cg, p.cg, (float)nrows, mean, m2);
    float* o = p.partial + (((size_t)s * p.G + t) * p.splits + sp) * 3;
    o[0] = (float)nrows * (float)p.cg;
    o[1] = mean;
    o[2] = m2;
  }
}
