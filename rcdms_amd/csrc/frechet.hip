// frechet.hip — running float64 feature statistics and the Fréchet distance between two sets of them, on the device
// (include/rcdm.h, "Fréchet distance").
//   rcdm_feature_stats_update    X (n x d, f32 or f16) -> sum += sum(x - k), outer += (X - k)^T (X - k), float64.  Two launches:
//                                a column-sum kernel and the TN product on v_mfma_f64_16x16x4_f64.
//   rcdm_gemm_tn_f64             C = A^T B in float64: the same TN kernel on double operands without a shift.
//   rcdm_feature_stats_finalize  mean, covariance (symmetric by construction) and its trace.
//   rcdm_frechet_mean_term       |mu_a - mu_b|^2.
//   rcdm_jacobi_sweep            one sweep of one-sided Jacobi over the rows of a buffer: rows - 1 rounds of rows / 2 disjoint plane
//                                rotations, one launch per round, one workgroup per pair.  No workgroup waits on another.
//   rcdm_jacobi_norm_sum         the row norms, their sum and their maximum.
//   rcdm_frechet_factor          rows w_j = lambda_j v_j of a finished sweep -> the factor F (columns w_j / sqrt(lambda_j)).
//   rcdm_cholesky_pivoted_f64    the other way to a factor: columns of P L of the diagonally pivoted Cholesky factorisation, blocked and
//                                right-looking.  Per column one single-workgroup launch (the pivot and the cut) and one launch of a
//                                thread per row (the column and the next diagonals, lazily against the panel); per panel one
//                                subtracting TN product.  No read-back: a stop flag in the workspace empties the later launches.
// TN product: a wave owns a 32 x 32 tile of C as 2 x 2 MFMA tiles, a workgroup of four waves 64 x 64.  Lane l holds A[k0 + (l >> 4)][i0 + (l & 15)]
// and B[k0 + (l >> 4)][j0 + (l & 15)] — the f32 16x16x4 operand maps, one double per lane — and the results
// C[i0 + (l >> 4) + 4 r][j0 + (l & 15)], r = 0..3: the f64 C/D map, which is NOT the f32 one.  The operands are read straight
// from global memory (a tile's 16 columns are one 64 / 128-byte segment per row) and widened exactly; rows beyond n and
// columns beyond d enter as 0.0 after the shift, so nothing outside [n][d] is read.  The k order of a tile is fixed and one lane
// alone adds its result to C: no atomics, the same input gives the same bits.
// Every sum elsewhere is fr's fixed-order sum (frechet_core.h): LANES strided partials, then a tree in LDS.
#include "common.h"
#include "frechet_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = fr::LANES;
constexpr int EPT = fr::MAX_DIM / NT;     // elements of one vector per thread: 16
typedef double f64x4 __attribute__((ext_vector_type(4)));

// fr's tree over the NT partials of one workgroup; every thread gets the sum.  red: NT doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();            // red may still be read from a previous sum
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// three sums through one tree: the same order as block_sum for each, a third of the barriers
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double (*red)[NT]) {
  const int tid = threadIdx.x;
  red[0][tid] = a;
  red[1][tid] = b;
  red[2][tid] = c;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
      red[2][tid] += red[2][tid + s];
    }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
  c = red[2][0];
}

__device__ __forceinline__ double block_max(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// ---- statistics ------------------------------------------------------------------------------------------------------------

// one thread per column: rows in ascending order
template <typename T>
__global__ __launch_bounds__(NT) void colsum_kernel(const T* __restrict__ x, int64_t ld, const float* __restrict__ shift, int n, int d,
                                                    double* __restrict__ sum) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= d) return;
  const double k = (double)shift[j];
  double s = 0.0;
#pragma unroll 8
  for (int r = 0; r < n; ++r) s += (double)x[(int64_t)r * ld + j] - k;
  sum[j] += s;
}

// ACC: 0 C = A^T B, 1 C += A^T B, -1 C -= A^T B (the product is summed from +0.0 first in all three)
template <typename T, bool SHIFT, int ACC>
__global__ __launch_bounds__(256) void tn_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
                                                 const float* __restrict__ shift, int m, int n, int k, double* __restrict__ C,
                                                 int64_t ldc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
  if (i0 >= m || j0 >= n) return;          // the whole wave; there is no barrier in this kernel
  const int li = lane & 15, lk = lane >> 4;
  int ia[2], jb[2];
  double ka[2], kb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    ia[u] = i0 + 16 * u + li;
    jb[u] = j0 + 16 * u + li;
    ka[u] = SHIFT && ia[u] < m ? (double)shift[ia[u]] : 0.0;
    kb[u] = SHIFT && jb[u] < n ? (double)shift[jb[u]] : 0.0;
  }
  f64x4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int k0 = 0; k0 < k; k0 += 4) {
    const int kk = k0 + lk;
    const bool row = kk < k;
    double a[2], b[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      a[u] = row && ia[u] < m ? (double)A[(int64_t)kk * lda + ia[u]] - ka[u] : 0.0;
      b[u] = row && jb[u] < n ? (double)B[(int64_t)kk * ldb + jb[u]] - kb[u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + 16 * u + lk + 4 * r, col = j0 + 16 * v + li;
        if (row < m && col < n) {
          double* c = C + (int64_t)row * ldc + col;
          *c = ACC > 0 ? *c + acc[u][v][r] : ACC < 0 ? *c - acc[u][v][r] : acc[u][v][r];
        }
      }
}

template <typename T, bool SHIFT, int ACC>
int launch_tn(const T* A, int64_t lda, const T* B, int64_t ldb, const float* shift, int m, int n, int k, double* C, int64_t ldc,
              hipStream_t st) {
  hipLaunchKernelGGL((tn_kernel<T, SHIFT, ACC>), dim3((n + 63) / 64, (m + 63) / 64), dim3(256), 0, st, A, lda, B, ldb, shift, m, n,
                     k, C, ldc);
  return rcdm_check_launch();
}

// mean = k + sum / n; cov[i][j] = (outer[lo][hi] - sum[lo] sum[hi] / n) / (n - 1) with lo <= hi: both triangles from the upper one
__global__ __launch_bounds__(NT) void finalize_kernel(const float* __restrict__ shift, const double* __restrict__ sum,
                                                      const double* __restrict__ outer, int d, double n, double* __restrict__ mean,
                                                      double* __restrict__ cov) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx < d) mean[idx] = (double)shift[idx] + sum[idx] / n;
  if (!cov || idx >= (int64_t)d * d) return;
  const int i = (int)(idx / d), j = (int)(idx - (int64_t)i * d);
  const int lo = min(i, j), hi = max(i, j);
  cov[idx] = (outer[(int64_t)lo * d + hi] - sum[lo] * sum[hi] / n) / (n - 1.0);
}

// out[0] = sum of the diagonal of a d x d matrix, one workgroup
__global__ __launch_bounds__(NT) void trace_kernel(const double* __restrict__ a, int d, double* __restrict__ out) {
  __shared__ double red[NT];
  double s = 0.0;
  for (int j = threadIdx.x; j < d; j += NT) s += a[(int64_t)j * d + j];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(NT) void mean_term_kernel(const double* __restrict__ a, const double* __restrict__ b, int d,
                                                       double* __restrict__ out) {
  __shared__ double red[NT];
  double s = 0.0;
  for (int j = threadIdx.x; j < d; j += NT) {
    const double df = a[j] - b[j];
    s += df * df;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- Jacobi ----------------------------------------------------------------------------------------------------------------

// workspace, doubles: [0] largest squared norm at the start of the sweep, [1] sum of the norms, [2] largest norm,
// [3] unused, [4 .. 4 + rows) the (squared) norms
constexpr int WS_HEAD = 4;

// one workgroup per row: out[row] = |w_row|^2, or its square root
__global__ __launch_bounds__(NT) void norms_kernel(const double* __restrict__ w, int64_t ld, int len, int root, double* __restrict__ out) {
  __shared__ double red[NT];
  const double* p = w + (int64_t)blockIdx.x * ld;
  double aa = 0.0, bb = 0.0, ab = 0.0;
  for (int k = threadIdx.x; k < len; k += NT) fr::accumulate(p[k], 0.0, aa, bb, ab);
  aa = block_sum(aa, red);
  if (threadIdx.x == 0) out[blockIdx.x] = root ? sqrt(aa) : aa;
}

// one workgroup: ws[0] = the largest of the rows squared norms, *count = 0
__global__ __launch_bounds__(NT) void sweep_begin_kernel(double* __restrict__ ws, int rows, int32_t* __restrict__ count) {
  __shared__ double red[NT];
  double mx = 0.0;
  for (int j = threadIdx.x; j < rows; j += NT) mx = fmax(mx, ws[WS_HEAD + j]);
  mx = block_max(mx, red);
  if (threadIdx.x == 0) {
    ws[0] = mx;
    *count = 0;
  }
}

// one workgroup: the sum (fixed order) and the maximum of the rows norms
__global__ __launch_bounds__(NT) void norm_sum_kernel(double* __restrict__ ws, int rows, double* __restrict__ out) {
  __shared__ double red[NT];
  double s = 0.0, mx = 0.0;
  for (int j = threadIdx.x; j < rows; j += NT) {
    s += ws[WS_HEAD + j];
    mx = fmax(mx, ws[WS_HEAD + j]);
  }
  s = block_sum(s, red);
  mx = block_max(mx, red);
  if (threadIdx.x == 0) {
    ws[1] = s;
    ws[2] = mx;
    if (out) {
      out[0] = s;
      out[1] = mx;
    }
  }
}

// pair blockIdx.x of round `round`: both vectors live in registers between the sums and the rotation
__global__ __launch_bounds__(NT) void jacobi_round_kernel(double* __restrict__ w, int64_t ld, int rows, int len, int dim, int round,
                                                          const double* __restrict__ ws, int32_t* __restrict__ count) {
  __shared__ double red[3][NT];
  const int tid = threadIdx.x;
  int p, q;
  fr::pair(rows, round, blockIdx.x, &p, &q);
  double* wp = w + (int64_t)p * ld;
  double* wq = w + (int64_t)q * ld;
  double a[EPT], b[EPT];
  double aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int k = tid + e * NT;
    a[e] = k < len ? wp[k] : 0.0;
    b[e] = k < len ? wq[k] : 0.0;
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) fr::accumulate(a[e], b[e], aa, bb, ab);     // a dead element adds +0.0: the sum is unchanged
  block_sum3(aa, bb, ab, red);
  double c, s;
  if (!fr::rotation(aa, bb, ab, fr::rule2_threshold(dim, ws[0]), &c, &s)) return;      // the whole workgroup: same values
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int k = tid + e * NT;
    if (k < len) {
      fr::rotate(c, s, a[e], b[e]);
      wp[k] = a[e];
      wq[k] = b[e];
    }
  }
  if (tid == 0) atomicAdd(count, 1);
}

// f[k][j] = w[j][k] / sqrt(lambda_j), or 0 for a row rule 3 drops; a 32 x 32 tile through LDS so that both sides are coalesced
__global__ __launch_bounds__(256) void factor_kernel(const double* __restrict__ w, int64_t ld, int rows, int len, int dim,
                                                     const double* __restrict__ ws, double* __restrict__ f, int64_t ldf) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
  const double lmax = ws[2];
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + r, k = k0 + tx;
    double v = 0.0;
    if (j < rows && k < len) {
      const double lam = ws[WS_HEAD + j];
      if (fr::keep_column(lam, lmax, dim)) v = fr::factor_entry(w[(int64_t)j * ld + k], lam);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, j = j0 + tx;
    if (k < len && j < rows) f[(int64_t)k * ldf + j] = tile[tx][r];
  }
}

__global__ __launch_bounds__(NT) void rank_kernel(const double* __restrict__ ws, int rows, int dim, int32_t* __restrict__ rank) {
  __shared__ int cnt[NT];
  int c = 0;
  for (int j = threadIdx.x; j < rows; j += NT) c += fr::keep_column(ws[WS_HEAD + j], ws[2], dim) ? 1 : 0;
  cnt[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < NT; ++i) t += cnt[i];
    *rank = t;
  }
}

// ---- pivoted Cholesky ------------------------------------------------------------------------------------------------------

// workspace, doubles: [0] the cut, [1] the pivot of the current step, [2] its square root, [3] 1.0 once the factorisation has
// stopped, [4 .. 8) unused; then work[d][d], the copy under factorisation; panel[nb][d], the current panel's columns, one per
// row (the TN product's operand layout); base[d], the diagonal of work at the panel's start; diag[d], the remaining diagonal;
// then int32: piv[d], the pivot of every step, and done[d].
constexpr int CH_HEAD = 8;
constexpr int CH_ROWS = 64;      // rows per workgroup of the column step: one wave

struct chol_ws {
  double *head, *work, *panel, *base, *diag;
  int32_t *piv, *done;
};

size_t chol_bytes(int d, int nb) {
  return ((size_t)CH_HEAD + (size_t)d * d + (size_t)nb * d + 2 * (size_t)d) * sizeof(double) + 2 * (size_t)(d + (d & 1)) * sizeof(int32_t);
}

chol_ws chol_carve(void* workspace, int d, int nb) {
  chol_ws w;
  w.head = (double*)workspace;
  w.work = w.head + CH_HEAD;
  w.panel = w.work + (size_t)d * d;
  w.base = w.panel + (size_t)nb * d;
  w.diag = w.base + d;
  w.piv = (int32_t*)(w.diag + d);
  w.done = w.piv + (d + (d & 1));
  return w;
}

// work = a (dense), f[d][d] = 0
__global__ __launch_bounds__(NT) void chol_begin_kernel(const double* __restrict__ a, int64_t ld, int d, double* __restrict__ work,
                                                        double* __restrict__ f, int64_t ldf) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)d * d) return;
  const int i = (int)(idx / d), j = (int)(idx - (int64_t)i * d);
  work[idx] = a[(int64_t)i * ld + j];
  f[(int64_t)i * ldf + j] = 0.0;
}

// one workgroup: the pivot of step j and the cut.  first: step j opens a panel, the remaining diagonal is that of work.
__global__ __launch_bounds__(NT) void chol_pivot_kernel(chol_ws w, int d, int j, int first, int32_t* __restrict__ rank) {
  __shared__ double red[NT];
  __shared__ int redi[NT];
  const int tid = threadIdx.x;
  if (j > 0 && w.head[3] != 0.0) return;           // the whole workgroup: stopped at an earlier step
  double mx = 0.0, bv = 0.0;
  int bi = -1;
  for (int i = tid; i < d; i += NT) {
    double v;
    if (first) {
      v = w.work[(int64_t)i * d + i];
      w.base[i] = v;
    } else {
      v = w.diag[i];
    }
    bool open = true;
    if (j == 0) {
      w.done[i] = 0;
      mx = fmax(mx, v);                            // a NaN diagonal is passed over
    } else {
      open = w.done[i] == 0;
    }
    if (open && fr::chol_better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
  if (j == 0) mx = block_max(mx, red);
  __syncthreads();
  red[tid] = bv;
  redi[tid] = bi;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s && redi[tid + s] >= 0 && fr::chol_better(red[tid + s], redi[tid + s], red[tid], redi[tid])) {
      red[tid] = red[tid + s];
      redi[tid] = redi[tid + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  bv = red[0];
  bi = redi[0];
  if (j == 0) w.head[0] = fr::chol_threshold(d, mx);
  if (!fr::chol_go(bv, bi, w.head[0])) {
    w.head[3] = 1.0;
    if (j == 0) *rank = 0;
    return;
  }
  w.piv[j] = bi;
  w.done[bi] = 1;
  w.head[1] = bv;
  w.head[2] = sqrt(bv);
  w.head[3] = 0.0;
  *rank = j + 1;
}

// one thread per row: column j of the factor (step j of the panel that began at step j0) and the row's next diagonal
template <int NB>
__global__ __launch_bounds__(CH_ROWS) void chol_column_kernel(chol_ws w, int d, int j, int j0, double* __restrict__ f, int64_t ldf) {
  if (w.head[3] != 0.0) return;
  const int i = blockIdx.x * CH_ROWS + threadIdx.x;
  if (i >= d) return;
  const int p = w.piv[j], cnt = j - j0;
  const double ljj = w.head[2];
  double* mine = w.panel + i;                       // element k of this row: mine[k * d]
  const double* pivot = w.panel + p;
  if (w.done[i]) {                                  // rows of earlier pivots are zero in this column; the pivot's own holds L_jj
    mine[(int64_t)cnt * d] = i == p ? ljj : 0.0;
    if (i == p) f[(int64_t)i * ldf + j] = ljj;
    return;
  }
  const double dot = fr::panel_sum<NB>(cnt, [&](int k) { return mine[(int64_t)k * d] * pivot[(int64_t)k * d]; });
  const double c = fr::chol_entry(w.work[(int64_t)p * d + i], dot, ljj);
  const double squares = fr::panel_sum<NB>(cnt + 1, [&](int k) {
    const double x = k < cnt ? mine[(int64_t)k * d] : c;
    return x * x;
  });
  mine[(int64_t)cnt * d] = c;
  f[(int64_t)i * ldf + j] = c;
  w.diag[i] = fr::chol_diag(w.base[i], squares);
}

template <int NB>
int chol_run(const rcdm_cholesky_desc* d, chol_ws w, double* f, int32_t* rank, hipStream_t st) {
  const int n = d->d;
  int rc;
  for (int j0 = 0; j0 < n; j0 += NB) {
    const int j1 = j0 + NB < n ? j0 + NB : n;
    for (int j = j0; j < j1; ++j) {
      hipLaunchKernelGGL(chol_pivot_kernel, dim3(1), dim3(NT), 0, st, w, n, j, j == j0 ? 1 : 0, rank);
      if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
      hipLaunchKernelGGL(chol_column_kernel<NB>, dim3((n + CH_ROWS - 1) / CH_ROWS), dim3(CH_ROWS), 0, st, w, n, j, j0, f, d->ldf);
      if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
    }
    // work -= panel^T panel over the whole matrix: rows and columns of earlier pivots are dead and cost nothing to carry
    if (j1 < n && (rc = launch_tn<double, false, -1>(w.panel, n, w.panel, n, nullptr, n, n, NB, w.work, n, st)) != RCDM_OK) return rc;
  }
  return RCDM_OK;
}

bool misaligned8(const void* p) { return ((uintptr_t)p & 7) != 0; }

int cholesky_check(const rcdm_cholesky_desc* d) {
  if (d->d < 1 || d->ld < d->d || d->ldf < d->d || (d->nb != 0 && !fr::chol_nb_ok(d->nb))) return RCDM_EINVAL;
  if (d->d > fr::MAX_DIM) return RCDM_ESHAPE;
  return RCDM_OK;
}

int stats_check(const rcdm_fstats_desc* d) {
  if (d->n < 1 || d->d < 1 || d->ld < d->d) return RCDM_EINVAL;
  if (d->dtype != RCDM_FSTATS_F32 && d->dtype != RCDM_FSTATS_F16) return RCDM_EINVAL;
  if (d->d > fr::MAX_DIM || d->n > (1 << 30)) return RCDM_ESHAPE;
  return RCDM_OK;
}

int jacobi_check(const rcdm_jacobi_desc* d) {
  if (d->rows < 2 || (d->rows & 1) || d->len < 1 || d->dim < 1 || d->ld < d->len) return RCDM_EINVAL;
  if (d->rows > fr::MAX_DIM || d->len > fr::MAX_DIM || d->dim > fr::MAX_DIM) return RCDM_ESHAPE;
  return RCDM_OK;
}

}  // namespace

extern "C" {

int rcdm_feature_stats_update(const rcdm_fstats_desc* d, const void* x, const float* shift, double* sum, double* outer,
                              void* stream) {
  if (!d || !x || !shift || !sum || !outer) return RCDM_EINVAL;
  const int rc = stats_check(d);
  if (rc != RCDM_OK) return rc;
  const int esz = d->dtype == RCDM_FSTATS_F16 ? 2 : 4;
  if (((uintptr_t)x & (esz - 1)) || ((uintptr_t)shift & 3) || misaligned8(sum) || misaligned8(outer)) return RCDM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 cg((d->d + NT - 1) / NT);
  if (d->dtype == RCDM_FSTATS_F16)
    hipLaunchKernelGGL(colsum_kernel<f16>, cg, dim3(NT), 0, st, (const f16*)x, d->ld, shift, d->n, d->d, sum);
  else
    hipLaunchKernelGGL(colsum_kernel<float>, cg, dim3(NT), 0, st, (const float*)x, d->ld, shift, d->n, d->d, sum);
  const int st1 = rcdm_check_launch();
  if (st1 != RCDM_OK) return st1;
  if (d->dtype == RCDM_FSTATS_F16)
    return launch_tn<f16, true, 1>((const f16*)x, d->ld, (const f16*)x, d->ld, shift, d->d, d->d, d->n, outer, d->d, st);
  return launch_tn<float, true, 1>((const float*)x, d->ld, (const float*)x, d->ld, shift, d->d, d->d, d->n, outer, d->d, st);
}

int rcdm_gemm_tn_f64(int32_t m, int32_t n, int32_t k, const double* a, int64_t lda, const double* b, int64_t ldb, double* c,
                     int64_t ldc, void* stream) {
  if (!a || !b || !c || m < 1 || n < 1 || k < 1 || lda < m || ldb < n || ldc < n) return RCDM_EINVAL;
  if (misaligned8(a) || misaligned8(b) || misaligned8(c)) return RCDM_EINVAL;
  if (m > fr::MAX_DIM || n > fr::MAX_DIM || k > (1 << 30)) return RCDM_ESHAPE;
  return launch_tn<double, false, 0>(a, lda, b, ldb, nullptr, m, n, k, c, ldc, (hipStream_t)stream);
}

int rcdm_feature_stats_finalize(int32_t d, int64_t n, const float* shift, const double* sum, const double* outer, double* mean,
                                double* cov, double* trace, void* stream) {
  if (!shift || !sum || !mean || d < 1 || n < 1) return RCDM_EINVAL;
  if (cov && (!outer || !trace || n < 2)) return RCDM_EINVAL;
  if (((uintptr_t)shift & 3) || misaligned8(sum) || misaligned8(outer) || misaligned8(mean) || misaligned8(cov) || misaligned8(trace))
    return RCDM_EINVAL;
  if (d > fr::MAX_DIM) return RCDM_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t items = cov ? (int64_t)d * d : d;
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((items + NT - 1) / NT)), dim3(NT), 0, st, shift, sum, outer, d, (double)n, mean, cov);
  const int rc = rcdm_check_launch();
  if (rc != RCDM_OK || !cov) return rc;
  hipLaunchKernelGGL(trace_kernel, dim3(1), dim3(NT), 0, st, (const double*)cov, d, trace);
  return rcdm_check_launch();
}

int rcdm_frechet_trace(int32_t d, const double* a, double* out, void* stream) {
  if (!a || !out || d < 1 || misaligned8(a) || misaligned8(out)) return RCDM_EINVAL;
  if (d > fr::MAX_DIM) return RCDM_ESHAPE;
  hipLaunchKernelGGL(trace_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a, d, out);
  return rcdm_check_launch();
}

int rcdm_frechet_mean_term(int32_t d, const double* mu_a, const double* mu_b, double* out, void* stream) {
  if (!mu_a || !mu_b || !out || d < 1 || misaligned8(mu_a) || misaligned8(mu_b) || misaligned8(out)) return RCDM_EINVAL;
  if (d > fr::MAX_DIM) return RCDM_ESHAPE;
  hipLaunchKernelGGL(mean_term_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, mu_a, mu_b, d, out);
  return rcdm_check_launch();
}

size_t rcdm_jacobi_workspace_bytes(const rcdm_jacobi_desc* d) {
  if (!d || jacobi_check(d) != RCDM_OK) return 0;
  return (size_t)(WS_HEAD + d->rows) * sizeof(double);
}

static int jacobi_args(const rcdm_jacobi_desc* d, const void* w, const void* workspace, size_t workspace_bytes) {
  if (!d || !w) return RCDM_EINVAL;
  const int rc = jacobi_check(d);
  if (rc != RCDM_OK) return rc;
  if (misaligned8(w) || misaligned8(workspace)) return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_jacobi_workspace_bytes(d)) return RCDM_EWORKSPACE;
  return RCDM_OK;
}

int rcdm_jacobi_sweep(const rcdm_jacobi_desc* d, double* w, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = jacobi_args(d, w, workspace, workspace_bytes);
  if (rc != RCDM_OK) return rc;
  if (!count || ((uintptr_t)count & 3)) return RCDM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  hipLaunchKernelGGL(norms_kernel, dim3(d->rows), dim3(NT), 0, st, (const double*)w, d->ld, d->len, 0, ws + WS_HEAD);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  hipLaunchKernelGGL(sweep_begin_kernel, dim3(1), dim3(NT), 0, st, ws, d->rows, count);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  for (int round = 0; round < d->rows - 1; ++round) {
    hipLaunchKernelGGL(jacobi_round_kernel, dim3(d->rows / 2), dim3(NT), 0, st, w, d->ld, d->rows, d->len, d->dim, round,
                       (const double*)ws, count);
    if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  }
  return RCDM_OK;
}

int rcdm_jacobi_norm_sum(const rcdm_jacobi_desc* d, const double* w, double* out, void* workspace, size_t workspace_bytes,
                         void* stream) {
  int rc = jacobi_args(d, w, workspace, workspace_bytes);
  if (rc != RCDM_OK) return rc;
  if (!out || misaligned8(out)) return RCDM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  hipLaunchKernelGGL(norms_kernel, dim3(d->rows), dim3(NT), 0, st, w, d->ld, d->len, 1, ws + WS_HEAD);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  hipLaunchKernelGGL(norm_sum_kernel, dim3(1), dim3(NT), 0, st, ws, d->rows, out);
  return rcdm_check_launch();
}

int rcdm_frechet_factor(const rcdm_jacobi_desc* d, const double* w, double* f, int64_t ldf, int32_t* rank, void* workspace,
                        size_t workspace_bytes, void* stream) {
  int rc = jacobi_args(d, w, workspace, workspace_bytes);
  if (rc != RCDM_OK) return rc;
  if (!f || !rank || misaligned8(f) || ((uintptr_t)rank & 3) || ldf < d->rows) return RCDM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  hipLaunchKernelGGL(norms_kernel, dim3(d->rows), dim3(NT), 0, st, w, d->ld, d->len, 1, ws + WS_HEAD);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  hipLaunchKernelGGL(norm_sum_kernel, dim3(1), dim3(NT), 0, st, ws, d->rows, (double*)nullptr);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  hipLaunchKernelGGL(factor_kernel, dim3((d->len + 31) / 32, (d->rows + 31) / 32), dim3(256), 0, st, w, d->ld, d->rows, d->len, d->dim,
                     (const double*)ws, f, ldf);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  hipLaunchKernelGGL(rank_kernel, dim3(1), dim3(NT), 0, st, (const double*)ws, d->rows, d->dim, rank);
  return rcdm_check_launch();
}

size_t rcdm_cholesky_workspace_bytes(const rcdm_cholesky_desc* d) {
  if (!d || cholesky_check(d) != RCDM_OK) return 0;
  return chol_bytes(d->d, d->nb ? d->nb : fr::CHOL_NB);
}

int rcdm_cholesky_pivoted_f64(const rcdm_cholesky_desc* d, const double* a, double* f, int32_t* rank, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!d || !a || !f || !rank) return RCDM_EINVAL;
  int rc = cholesky_check(d);
  if (rc != RCDM_OK) return rc;
  if (misaligned8(a) || misaligned8(f) || ((uintptr_t)rank & 3) || misaligned8(workspace)) return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_cholesky_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int n = d->d, nb = d->nb ? d->nb : fr::CHOL_NB;
  const chol_ws w = chol_carve(workspace, n, nb);
  const int64_t items = (int64_t)n * n;
  hipLaunchKernelGGL(chol_begin_kernel, dim3((unsigned)((items + NT - 1) / NT)), dim3(NT), 0, st, a, d->ld, n, w.work, f, d->ldf);
  if ((rc = rcdm_check_launch()) != RCDM_OK) return rc;
  if (nb == 16) return chol_run<16>(d, w, f, rank, st);
  if (nb == 32) return chol_run<32>(d, w, f, rank, st);
  if (nb == 64) return chol_run<64>(d, w, f, rank, st);
  return chol_run<128>(d, w, f, rank, st);
}

}  // extern "C"
