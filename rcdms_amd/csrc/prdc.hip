// prdc.hip — the k-nearest-neighbour manifold figures on the device (include/rcdm.h, "Manifold figures"): improved precision and
// recall, density and coverage over stored feature rows.  csrc/prdc_core.h has the definitions and the order of everything.
//   rcdm_row_norms2_f64   |row|^2 of a set in float64, fr's fixed sum, one workgroup per row.
//   rcdm_knn_radii2       r2[i] = the k-th smallest D2 of row i to the other rows of its set.
//   rcdm_prdc_counts      fake_count, real_hit, real_min2 and the four int64 numerators from one sweep of the nx x ny tiles.
// Tile product: kid.hip's (copied, so that KID's bits stay pinned by its own file): an NT product on v_mfma_f64_16x16x4_f64 over
// the contiguous feature axis, a 64 x 64 tile per workgroup of four waves, a wave a 32 x 32 quarter as 2 x 2 MFMA results, one row
// per lane, 16-byte (f32) or 8-byte (f16) loads where pointers and pitches allow, int64 row addresses, dead rows and columns
// beyond d entering as 0.0 without being read.  The results sit in the f64 C/D map, which kid::element restates.
// Radius sweep, grid (row strips, column chunks): a workgroup walks the tile columns of its chunk.  Per tile the epilogue turns
// dots into D2, sets positions outside the set and the position-diagonal to +inf (zero operands mask nothing) and writes the tile
// to LDS, 65 doubles per row (33 280 bytes).  Then four threads share a row, 16 columns each, and every thread keeps the k smallest
// values in a sorted register list whose indices are all compile-time constants (prdc::list_insert).  After the last tile the four
// lists of a row are merged through LDS and the k candidates go to the workspace; a second launch merges the chunks' candidates
// into the k-th smallest.  The distances never reach HBM as a matrix.
// LDS banks: a thread's walk reads row * 65 + 16 seg + c — the sixteen rows and four segments of a wave fall on 64 distinct
// 8-byte slots of two passes, conflict-free at the ds_read_b64 rate.  The epilogue's writes (row = lq + 4 r, col = li) meet four
// ways at most: sixteen writes per thread per tile against d / 4 MFMA steps.
// Count sweep, grid (row strips, column chunks): per tile the column counts of fake_count go through a small LDS array (eight
// partial counts per column, added by 64 threads: no atomics) to one byte per (row strip, column); the row ors of real_hit and the
// row minima of real_min2 stay in registers over the whole chunk and are folded once, through LDS, into one partial per (chunk,
// row).  A fold launch adds the bytes over the row strips, ors and minimises over the chunks and forms four int64 partial
// numerators per workgroup; a last launch of one workgroup adds those.  Integer sums, ors and minima only: any order gives the
// same bits.  No memset, no atomics, no scratch (profiles/prdc_kernel_resources.txt).
#include "common.h"
#include "prdc_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = prdc::THREADS;
constexpr int TILE = prdc::TILE;
typedef double f64x4 __attribute__((ext_vector_type(4)));

// features k .. k + 3 of one row as doubles; a dead row and features beyond d are 0.0 and are not read
template <typename T, bool VEC>
__device__ __forceinline__ void load4(const T* __restrict__ row, bool live, int k, int d, double out[4]) {
  if (VEC && live && k + 3 < d) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 v = *(const f32x4*)(row + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = (double)v[j];
    } else {
      const f16x4 v = *(const f16x4*)(row + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = (double)v[j];
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = live && k + j < d ? (double)row[k + j] : 0.0;
}

// acc[u][v] = the 16 x 16 products of rows i0 + 16 u + .. of a (na rows) against rows j0 + 16 v + .. of b (nb rows); i0, j0 are
// the wave's quarter.  The whole wave skips a quarter that lies outside either set (acc stays 0.0).
template <typename T, bool VEC>
__device__ __forceinline__ void tile_product(const T* __restrict__ abase, int64_t lda, int na, const T* __restrict__ bbase,
                                             int64_t ldb, int nb, int i0, int j0, int d, int lane, f64x4 (&acc)[2][2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
  if (i0 >= na || j0 >= nb) return;
  const int li = lane & 15, lq = lane >> 4;
  const T* arow[2];
  const T* brow[2];
  bool alive[2], blive[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = i0 + 16 * u + li, j = j0 + 16 * u + li;
    alive[u] = i < na;
    blive[u] = j < nb;
    arow[u] = abase + (alive[u] ? (int64_t)i : (int64_t)0) * lda;
    brow[u] = bbase + (blive[u] ? (int64_t)j : (int64_t)0) * ldb;
  }
  for (int k0 = 0; k0 < d; k0 += 16) {
    const int k = k0 + 4 * lq;
    double av[2][4], bv[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      load4<T, VEC>(arow[u], alive[u], k, d, av[u]);
      load4<T, VEC>(brow[u], blive[u], k, d, bv[u]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][j], bv[v][j], acc[u][v], 0, 0, 0);
  }
}

// ---- row norms: grid nx + ny, one workgroup per row; rows 0 .. nx - 1 are x's, the others y's (ny may be 0)
template <typename T>
__global__ __launch_bounds__(fr::LANES) void norms_kernel(const T* __restrict__ x, int64_t ldx, int nx, double* __restrict__ outx,
                                                          const T* __restrict__ y, int64_t ldy, double* __restrict__ outy, int d) {
  __shared__ double red[fr::LANES];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const T* row = r < nx ? x + (int64_t)r * ldx : y + (int64_t)(r - nx) * ldy;
  double s = 0.0;
  for (int k = tid; k < d; k += fr::LANES) {
    const double v = (double)row[k];
    s += v * v;
  }
  red[tid] = s;
  __syncthreads();
  for (int h = fr::LANES / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    if (r < nx) outx[r] = red[0];
    else outy[r - nx] = red[0];
  }
}

// ---- radius sweep
struct knn_args {
  const void* x;
  int64_t ld;
  int n, d, k, chunks, tiles;
  const double* norms;             // [n]
  double* cand;                    // [chunks][n][k]
};

// Three waves per SIMD: left alone the compiler takes 192 VGPRs + 32 AGPRs (two waves) and the k-loop, which has no software
// pipeline, is then short of waves to hide its loads behind (profiles/prdc.txt has the A/B: 0.67 -> 0.84 of rcdm_poly_mmd's issued
// rate).  Held to 168 registers it fits without scratch (profiles/prdc_kernel_resources.txt); four waves would need scratch.
#define PRDC_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(3, 3)))
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) PRDC_WAVES_ATTR void knn_tile_kernel(const knn_args a) {
  __shared__ double tile[TILE * prdc::TILE_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ti = blockIdx.x, chunk = blockIdx.y;
  const int n = a.n, k = a.k;
  int t0, t1;
  prdc::chunk_tiles(a.tiles, a.chunks, chunk, &t0, &t1);
  const int srow = tid / prdc::SEGMENTS, seg = tid - srow * prdc::SEGMENTS;      // the scan: row of the tile, segment of it
  double list[prdc::LIST];
  prdc::list_init(list, k);

  double nrow[8];                  // |x_i|^2 of the eight rows this thread's results lie in: e >> 3 and e & 3
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int row, col;
    kid::element(tid, (q >> 2) * 8 + (q & 3), &row, &col);
    const int i = ti * TILE + row;
    nrow[q] = i < n ? a.norms[i] : 0.0;
  }

  for (int tj = t0; tj < t1; ++tj) {
    f64x4 acc[2][2];
    tile_product<T, VEC>((const T*)a.x, a.ld, n, (const T*)a.x, a.ld, n, ti * TILE + (wave >> 1) * 32, tj * TILE + (wave & 1) * 32,
                         a.d, lane, acc);
    double ncol[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      int row, col;
      kid::element(tid, v * 4, &row, &col);
      const int j = tj * TILE + col;
      ncol[v] = j < n ? a.norms[j] : 0.0;
    }
    __syncthreads();               // the scan of the tile before is over
#pragma unroll
    for (int e = 0; e < prdc::REGS; ++e) {
      int row, col;
      kid::element(tid, e, &row, &col);
      const int i = ti * TILE + row, j = tj * TILE + col;
      const double d2 = prdc::dist2(nrow[(e >> 3) * 4 + (e & 3)], ncol[(e >> 2) & 1], acc[e >> 3][(e >> 2) & 1][e & 3]);
      tile[row * prdc::TILE_LD + col] = (i < n && j < n && i != j) ? d2 : INFINITY;
    }
    __syncthreads();
    const double* p = tile + srow * prdc::TILE_LD + seg * prdc::SEG_COLS;
#pragma unroll 4
    for (int c = 0; c < prdc::SEG_COLS; ++c) prdc::list_insert(list, p[c]);
  }

  // the four lists of a row into one: through the tile's LDS, [thread][LIST]
  __syncthreads();
#pragma unroll
  for (int p = 0; p < prdc::LIST; ++p) tile[tid * prdc::LIST + p] = list[p];
  __syncthreads();
  if (seg == 0) {
    for (int s = 1; s < prdc::SEGMENTS; ++s)
      for (int p = prdc::LIST - k; p < prdc::LIST; ++p) prdc::list_insert(list, tile[(tid + s) * prdc::LIST + p]);
#pragma unroll
    for (int p = 0; p < prdc::LIST; ++p) tile[tid * prdc::LIST + p] = list[p];
    const int i = ti * TILE + srow;
    if (i < n) {
      double* out = a.cand + ((int64_t)chunk * n + i) * k;
      for (int q = 0; q < k; ++q) out[q] = tile[tid * prdc::LIST + prdc::LIST - k + q];       // own slots: no barrier needed
    }
  }
}

// one thread per row: the k-th smallest of the chunks' candidates
__global__ __launch_bounds__(NT) void knn_merge_kernel(const double* __restrict__ cand, int n, int k, int chunks, double* __restrict__ r2) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  double list[prdc::LIST];
  prdc::list_init(list, k);
  for (int c = 0; c < chunks; ++c) {
    const double* p = cand + ((int64_t)c * n + i) * k;
    for (int q = 0; q < k; ++q) prdc::list_insert(list, p[q]);
  }
  r2[i] = prdc::list_kth(list);
}

// ---- count sweep
struct cnt_args {
  const void *x, *y;
  int64_t ldx, ldy;
  int nx, ny, d, chunks, tx, ty;
  const double *normx, *normy, *rx2, *ry2;
  uint8_t* colcnt;                 // [tx][ny]: of the 64 rows of strip ti, those whose ball holds column j
  int32_t* rowhit;                 // [chunks][nx]
  double* rowmin;                  // [chunks][nx]
};

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) PRDC_WAVES_ATTR void cnt_tile_kernel(const cnt_args a) {
  __shared__ int colpart[8][TILE + 1];              // [row group of a column: 2 wave rows x 4 lane groups][column]
  __shared__ double minpart[32][TILE + 1];          // [column group of a row: 2 wave columns x 16 lanes][row]
  __shared__ int hitpart[32][TILE + 1];          // + 1: the sixteen lanes of a row group do not meet in one bank
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ti = blockIdx.x, chunk = blockIdx.y;
  const int nx = a.nx, ny = a.ny;
  int t0, t1;
  prdc::chunk_tiles(a.ty, a.chunks, chunk, &t0, &t1);

  double nrow[8], rrow[8], rmin[8];
  int rhit[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int row, col;
    kid::element(tid, (q >> 2) * 8 + (q & 3), &row, &col);
    const int i = ti * TILE + row;
    nrow[q] = i < nx ? a.normx[i] : 0.0;
    rrow[q] = i < nx ? a.rx2[i] : 0.0;
    rmin[q] = INFINITY;
    rhit[q] = 0;
  }

  for (int tj = t0; tj < t1; ++tj) {
    f64x4 acc[2][2];
    tile_product<T, VEC>((const T*)a.x, a.ldx, nx, (const T*)a.y, a.ldy, ny, ti * TILE + (wave >> 1) * 32, tj * TILE + (wave & 1) * 32,
                         a.d, lane, acc);
    double ncol[2], rcol[2];
    int ccnt[2] = {0, 0};
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      int row, col;
      kid::element(tid, v * 4, &row, &col);
      const int j = tj * TILE + col;
      ncol[v] = j < ny ? a.normy[j] : 0.0;
      rcol[v] = j < ny ? a.ry2[j] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < prdc::REGS; ++e) {
      int row, col;
      kid::element(tid, e, &row, &col);
      const int i = ti * TILE + row, j = tj * TILE + col;
      const int q = (e >> 3) * 4 + (e & 3), v = (e >> 2) & 1;
      if (i < nx && j < ny) {      // a position outside either set takes part in nothing
        const double d2 = prdc::dist2(nrow[q], ncol[v], acc[e >> 3][v][e & 3]);
        ccnt[v] += prdc::in_ball(d2, rrow[q]) ? 1 : 0;
        rhit[q] |= prdc::in_ball(d2, rcol[v]) ? 1 : 0;
        rmin[q] = d2 < rmin[q] ? d2 : rmin[q];
      }
    }
    __syncthreads();               // the fold of the tile before is over
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      int row, col;
      kid::element(tid, v * 4, &row, &col);
      colpart[(wave >> 1) * 4 + (lane >> 4)][col] = ccnt[v];
    }
    __syncthreads();
    if (tid < TILE) {
      int s = 0;
#pragma unroll
      for (int g = 0; g < 8; ++g) s += colpart[g][tid];
      const int j = tj * TILE + tid;
      if (j < ny) a.colcnt[(int64_t)ti * ny + j] = (uint8_t)s;        // at most 64
    }
  }

#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int row, col;
    kid::element(tid, (q >> 2) * 8 + (q & 3), &row, &col);
    const int g = (wave & 1) * 16 + (lane & 15);
    minpart[g][row] = rmin[q];
    hitpart[g][row] = rhit[q];
  }
  __syncthreads();
  if (tid < TILE) {
    double m = INFINITY;
    int h = 0;
    for (int g = 0; g < 32; ++g) {
      const double v = minpart[g][tid];
      m = v < m ? v : m;
      h |= hitpart[g][tid];
    }
    const int i = ti * TILE + tid;
    if (i < nx) {
      a.rowmin[(int64_t)chunk * nx + i] = m;
      a.rowhit[(int64_t)chunk * nx + i] = h;
    }
  }
}

// thread t of the grid: column t of Y (fake_count) and row t of X (real_hit, real_min2, coverage); four partial numerators per
// workgroup
__global__ __launch_bounds__(NT) void cnt_fold_kernel(const cnt_args a, int32_t* __restrict__ fake_count, int32_t* __restrict__ real_hit,
                                                      double* __restrict__ real_min2, int64_t* __restrict__ parts) {
  __shared__ int red[4][NT];
  const int tid = threadIdx.x, t = blockIdx.x * NT + tid;
  int v[4] = {0, 0, 0, 0};
  if (t < a.ny) {
    int c = 0;
    for (int ti = 0; ti < a.tx; ++ti) c += a.colcnt[(int64_t)ti * a.ny + t];
    fake_count[t] = c;
    v[prdc::PRECISION] = c > 0 ? 1 : 0;
    v[prdc::DENSITY] = c;          // at most nx <= 65536 per column, 2^24 per workgroup: int32 holds it
  }
  if (t < a.nx) {
    double m = INFINITY;
    int h = 0;
    for (int c = 0; c < a.chunks; ++c) {
      const double w = a.rowmin[(int64_t)c * a.nx + t];
      m = w < m ? w : m;
      h |= a.rowhit[(int64_t)c * a.nx + t];
    }
    real_hit[t] = h;
    real_min2[t] = m;
    v[prdc::RECALL] = h;
    v[prdc::COVERAGE] = prdc::in_ball(m, a.rx2[t]) ? 1 : 0;
  }
#pragma unroll
  for (int f = 0; f < 4; ++f) red[f][tid] = v[f];
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int f = 0; f < 4; ++f) red[f][tid] += red[f][tid + h];
    }
    __syncthreads();
  }
  if (tid < 4) parts[(int64_t)blockIdx.x * 4 + tid] = (int64_t)red[tid][0];
}

__global__ __launch_bounds__(NT) void cnt_final_kernel(const int64_t* __restrict__ parts, int blocks, int64_t* __restrict__ out) {
  __shared__ int64_t red[4][NT];
  const int tid = threadIdx.x;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    int64_t s = 0;
    for (int b = tid; b < blocks; b += NT) s += parts[(int64_t)b * 4 + f];
    red[f][tid] = s;
  }
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int f = 0; f < 4; ++f) red[f][tid] += red[f][tid + h];
    }
    __syncthreads();
  }
  if (tid < 4) out[tid] = red[tid][0];
}

// ---- host side
bool dtype_ok(int dtype) { return dtype == RCDM_FSTATS_F32 || dtype == RCDM_FSTATS_F16; }
uintptr_t elem_mask(int dtype) { return dtype == RCDM_FSTATS_F16 ? 1 : 3; }
bool vec_ok(int dtype, const void* p, int64_t ld) { return !((uintptr_t)p & (dtype == RCDM_FSTATS_F16 ? 7 : 15)) && !(ld & 3); }
size_t round8(size_t v) { return (v + 7) & ~(size_t)7; }

int knn_check(const rcdm_knn_desc* d) {
  if (d->d < 1 || d->n < 1 || d->ld < d->d || d->k < 1 || d->k > prdc::MAX_K || d->n < d->k + 1) return RCDM_EINVAL;
  if (d->col_chunks < 0 || d->col_chunks > prdc::MAX_CHUNKS || d->flags != 0 || !dtype_ok(d->dtype)) return RCDM_EINVAL;
  if (d->d > prdc::MAX_DIM || d->n > prdc::MAX_N) return RCDM_ESHAPE;
  return RCDM_OK;
}

int knn_chunks(const rcdm_knn_desc* d) {
  const int t = prdc::tiles(d->n);
  return d->col_chunks ? d->col_chunks : prdc::default_chunks(t, t);
}

int cnt_check(const rcdm_prdc_desc* d) {
  if (d->d < 1 || d->nx < 1 || d->ny < 1 || d->ldx < d->d || d->ldy < d->d) return RCDM_EINVAL;
  if (d->col_chunks < 0 || d->col_chunks > prdc::MAX_CHUNKS || d->flags != 0 || !dtype_ok(d->dtype)) return RCDM_EINVAL;
  if (d->d > prdc::MAX_DIM || d->nx > prdc::MAX_N || d->ny > prdc::MAX_N) return RCDM_ESHAPE;
  return RCDM_OK;
}

int cnt_chunks(const rcdm_prdc_desc* d) {
  return d->col_chunks ? d->col_chunks : prdc::default_chunks(prdc::tiles(d->nx), prdc::tiles(d->ny));
}

int cnt_fold_blocks(const rcdm_prdc_desc* d) { return ((d->nx > d->ny ? d->nx : d->ny) + NT - 1) / NT; }

void norms_launch(int dtype, const void* x, int64_t ldx, int nx, double* outx, const void* y, int64_t ldy, int ny, double* outy, int d,
                  hipStream_t st) {
  const dim3 grid((unsigned)(nx + ny)), threads(fr::LANES);
  if (dtype == RCDM_FSTATS_F16)
    hipLaunchKernelGGL(norms_kernel<f16>, grid, threads, 0, st, (const f16*)x, ldx, nx, outx, (const f16*)y, ldy, outy, d);
  else
    hipLaunchKernelGGL(norms_kernel<float>, grid, threads, 0, st, (const float*)x, ldx, nx, outx, (const float*)y, ldy, outy, d);
}

}  // namespace

extern "C" {

int rcdm_row_norms2_f64(const void* x, int32_t n, int32_t d, int64_t ld, int32_t dtype, double* out, void* stream) {
  if (!x || !out || n < 1 || d < 1 || ld < d || !dtype_ok(dtype)) return RCDM_EINVAL;
  if (((uintptr_t)x & elem_mask(dtype)) || ((uintptr_t)out & 7)) return RCDM_EINVAL;
  if (d > prdc::MAX_DIM || n > prdc::MAX_N) return RCDM_ESHAPE;
  norms_launch(dtype, x, ld, n, out, nullptr, 0, 0, nullptr, d, (hipStream_t)stream);
  return rcdm_check_launch();
}

size_t rcdm_knn_radii2_workspace_bytes(const rcdm_knn_desc* d) {
  if (!d || knn_check(d) != RCDM_OK) return 0;
  return ((size_t)d->n + (size_t)knn_chunks(d) * d->n * d->k) * sizeof(double);
}

int rcdm_knn_radii2(const rcdm_knn_desc* d, const void* x, double* r2, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !x || !r2) return RCDM_EINVAL;
  const int rc = knn_check(d);
  if (rc != RCDM_OK) return rc;
  if (((uintptr_t)x & elem_mask(d->dtype)) || ((uintptr_t)r2 & 7) || ((uintptr_t)workspace & 7)) return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_knn_radii2_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  knn_args a;
  a.x = x;
  a.ld = d->ld;
  a.n = d->n;
  a.d = d->d;
  a.k = d->k;
  a.chunks = knn_chunks(d);
  a.tiles = prdc::tiles(d->n);
  double* norms = (double*)workspace;
  a.norms = norms;
  a.cand = norms + d->n;
  norms_launch(d->dtype, x, d->ld, d->n, norms, nullptr, 0, 0, nullptr, d->d, st);
  int lrc = rcdm_check_launch();
  if (lrc != RCDM_OK) return lrc;
  const dim3 grid((unsigned)a.tiles, (unsigned)a.chunks), threads(NT);
  const bool vec = vec_ok(d->dtype, x, d->ld);
  if (d->dtype == RCDM_FSTATS_F16) {
    if (vec) hipLaunchKernelGGL((knn_tile_kernel<f16, true>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((knn_tile_kernel<f16, false>), grid, threads, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((knn_tile_kernel<float, true>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((knn_tile_kernel<float, false>), grid, threads, 0, st, a);
  }
  if ((lrc = rcdm_check_launch()) != RCDM_OK) return lrc;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((d->n + NT - 1) / NT)), threads, 0, st, (const double*)a.cand, d->n, d->k,
                     a.chunks, r2);
  return rcdm_check_launch();
}

size_t rcdm_prdc_counts_workspace_bytes(const rcdm_prdc_desc* d) {
  if (!d || cnt_check(d) != RCDM_OK) return 0;
  const size_t nx = (size_t)d->nx, ny = (size_t)d->ny, chunks = (size_t)cnt_chunks(d);
  return (nx + ny + chunks * nx) * sizeof(double) + (size_t)cnt_fold_blocks(d) * 4 * sizeof(int64_t) +
         round8(chunks * nx * sizeof(int32_t)) + round8((size_t)prdc::tiles(d->nx) * ny);
}

int rcdm_prdc_counts(const rcdm_prdc_desc* d, const void* x, const void* y, const double* rx2, const double* ry2, int64_t* out,
                     int32_t* fake_count, int32_t* real_hit, double* real_min2, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !x || !y || !rx2 || !ry2 || !out || !fake_count || !real_hit || !real_min2) return RCDM_EINVAL;
  const int rc = cnt_check(d);
  if (rc != RCDM_OK) return rc;
  const uintptr_t em = elem_mask(d->dtype);
  if (((uintptr_t)x & em) || ((uintptr_t)y & em) || (((uintptr_t)rx2 | (uintptr_t)ry2 | (uintptr_t)out | (uintptr_t)real_min2) & 7) ||
      (((uintptr_t)fake_count | (uintptr_t)real_hit) & 3) || ((uintptr_t)workspace & 7))
    return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_prdc_counts_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  cnt_args a;
  a.x = x;
  a.y = y;
  a.ldx = d->ldx;
  a.ldy = d->ldy;
  a.nx = d->nx;
  a.ny = d->ny;
  a.d = d->d;
  a.chunks = cnt_chunks(d);
  a.tx = prdc::tiles(d->nx);
  a.ty = prdc::tiles(d->ny);
  const size_t nx = (size_t)d->nx, ny = (size_t)d->ny, chunks = (size_t)a.chunks;
  const int blocks = cnt_fold_blocks(d);
  double* normx = (double*)workspace;
  double* normy = normx + nx;
  a.normx = normx;
  a.normy = normy;
  a.rx2 = rx2;
  a.ry2 = ry2;
  a.rowmin = normy + ny;
  int64_t* parts = (int64_t*)(a.rowmin + chunks * nx);
  a.rowhit = (int32_t*)(parts + (size_t)blocks * 4);
  a.colcnt = (uint8_t*)a.rowhit + round8(chunks * nx * sizeof(int32_t));
  norms_launch(d->dtype, x, d->ldx, d->nx, normx, y, d->ldy, d->ny, normy, d->d, st);
  int lrc = rcdm_check_launch();
  if (lrc != RCDM_OK) return lrc;
  const dim3 grid((unsigned)a.tx, (unsigned)a.chunks), threads(NT);
  const bool vec = vec_ok(d->dtype, x, d->ldx) && vec_ok(d->dtype, y, d->ldy);
  if (d->dtype == RCDM_FSTATS_F16) {
    if (vec) hipLaunchKernelGGL((cnt_tile_kernel<f16, true>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((cnt_tile_kernel<f16, false>), grid, threads, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((cnt_tile_kernel<float, true>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((cnt_tile_kernel<float, false>), grid, threads, 0, st, a);
  }
  if ((lrc = rcdm_check_launch()) != RCDM_OK) return lrc;
  hipLaunchKernelGGL(cnt_fold_kernel, dim3((unsigned)blocks), threads, 0, st, a, fake_count, real_hit, real_min2, parts);
  if ((lrc = rcdm_check_launch()) != RCDM_OK) return lrc;
  hipLaunchKernelGGL(cnt_final_kernel, dim3(1), threads, 0, st, (const int64_t*)parts, blocks, out);
  return rcdm_check_launch();
}

}  // extern "C"
