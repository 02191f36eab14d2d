// kid.hip — the kernel distance on the device (include/rcdm.h, "Kernel distance"): the polynomial-kernel MMD^2 between subsets of
// stored feature rows, all subsets and all three blocks (xx, yy, xy) in one launch of the tile kernel and one of the reduce.
//   rcdm_poly_mmd        out[subset] = Sxx, Syy, Sxy, mmd2 (csrc/kid_core.h has the definition and the order of every sum).
//   rcdm_poly_gram_f64   the unmasked kernel matrix of the first subset, from the same tile body with a storing epilogue.
// Tile kernel: an NT product on v_mfma_f64_16x16x4_f64, contracting over the contiguous feature axis with both operands' rows
// gathered through the index lists.  A workgroup of four waves owns a 64 x 64 tile of one block of one subset, a wave a 32 x 32
// quarter as 2 x 2 MFMA results.  Lane l holds row idx[i0 + (l & 15)] of its operand — one row per lane — and of a 16-wide
// k-step the four consecutive features k0 + 4 (l >> 4) + 0 .. 3, one 16-byte (f32) or 8-byte (f16) load where the rows are so
// aligned (pointers and pitches multiples of four elements; single elements otherwise and in the tail of a row), i.e. one
// 64-byte segment per row per step.  MFMA j = 0 .. 3 of the step contracts over feature k0 + 4 q + j of the four lane groups
// q: which k meets which MFMA is free, the sum is over all of them.  Rows beyond m and columns beyond d enter as 0.0 and are
// never read (nor is the index list beyond m); row addresses are formed in int64.  The results sit in the f64 C/D map
// (col = lane & 15, row = (lane >> 4) + 4 reg: NOT the f32 one), which kid::element restates for the host model.
// Epilogue: k = (gamma dot + c)^p per result, skipped where the position is outside the subset or on the masked diagonal
// (zero operands mask nothing: a padded row has k = c^p), a thread's 16 values added in register order, the tile's 256 sums
// through a tree in LDS, one partial per tile (doubled for an off-diagonal tile of a symmetric block, whose mirror image is not
// computed).  No atomics; no scratch (profiles/kid_kernel_resources.txt).
#include "common.h"
#include "kid_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = kid::THREADS;
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct mmd_args {
  const void *x, *y;
  const int32_t *ix, *iy;          // [subsets][m], or null: rows 0 .. m - 1
  int64_t ldx, ldy;
  int m, d, degree, tiles;
  double gamma, coef0;
  double* partials;                // [subsets][3][tiles * tiles]
  double* gram;                    // the storing epilogue's [m][ldo]
  int64_t ldo;
};

// features k .. k + 3 of one row as doubles; a dead row (beyond m) and features beyond d are 0.0 and are not read
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

// grid (tiles * tiles, blocks, subsets).  STORE: the kernel matrix of block xy of subset 0 goes to a.gram, nothing is summed.
template <typename T, bool VEC, bool STORE>
__global__ __launch_bounds__(NT) void mmd_tile_kernel(const mmd_args a) {
  __shared__ double red[NT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ti = blockIdx.x / a.tiles, tj = blockIdx.x - ti * a.tiles;
  const int block = STORE ? kid::XY : (int)blockIdx.y, subset = blockIdx.z;
  const int m = a.m, d = a.d;
  double* part = STORE ? nullptr : a.partials + ((int64_t)subset * 3 + block) * ((int64_t)a.tiles * a.tiles) + blockIdx.x;
  const int weight = kid::tile_weight(block, ti, tj);
  if (weight == 0) {                       // the whole workgroup: the mirror image of a tile that counts twice
    if (tid == 0) *part = 0.0;
    return;
  }
  const T* abase = (const T*)(block == kid::YY ? a.y : a.x);
  const T* bbase = (const T*)(block == kid::XX ? a.x : a.y);
  const int64_t lda = block == kid::YY ? a.ldy : a.ldx, ldb = block == kid::XX ? a.ldx : a.ldy;
  const int32_t* alist = block == kid::YY ? a.iy : a.ix;
  const int32_t* blist = block == kid::XX ? a.ix : a.iy;
  const int i0 = ti * kid::TILE + (wave >> 1) * 32, j0 = tj * kid::TILE + (wave & 1) * 32;
  const int li = lane & 15, lq = lane >> 4;

  f64x4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};

  if (i0 < m && j0 < m) {                  // the whole wave
    const T* arow[2];
    const T* brow[2];
    bool alive[2], blive[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = i0 + 16 * u + li, j = j0 + 16 * u + li;
      alive[u] = i < m;
      blive[u] = j < m;
      const int64_t ra = !alive[u] ? 0 : alist ? (int64_t)alist[(int64_t)subset * m + i] : (int64_t)i;
      const int64_t rb = !blive[u] ? 0 : blist ? (int64_t)blist[(int64_t)subset * m + j] : (int64_t)j;
      arow[u] = abase + ra * lda;
      brow[u] = bbase + rb * ldb;
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

  double s = 0.0;
#pragma unroll
  for (int e = 0; e < kid::REGS; ++e) {
    int row, col;
    kid::element(tid, e, &row, &col);
    const int i = ti * kid::TILE + row, j = tj * kid::TILE + col;
    const double dot = acc[e >> 3][(e >> 2) & 1][e & 3];
    if (STORE) {
      if (i < m && j < m) a.gram[(int64_t)i * a.ldo + j] = kid::kernel_value(dot, a.gamma, a.coef0, a.degree);
    } else if (!kid::skipped(block, i, j, m)) {
      s += kid::kernel_value(dot, a.gamma, a.coef0, a.degree);
    }
  }
  if (STORE) return;
  red[tid] = s;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) *part = weight == 2 ? 2.0 * red[0] : red[0];
}

// one workgroup per subset: fr's fixed sum over the n tile partials of each block, then mmd2
__global__ __launch_bounds__(fr::LANES) void mmd_reduce_kernel(const double* __restrict__ partials, int64_t n, int m,
                                                                 double* __restrict__ out) {
  __shared__ double red[3][fr::LANES];
  const int tid = threadIdx.x;
  const double* p = partials + (int64_t)blockIdx.x * 3 * n;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    double v = 0.0;
    for (int64_t k = tid; k < n; k += fr::LANES) v += p[b * n + k];
    red[b][tid] = v;
  }
  __syncthreads();
  for (int h = fr::LANES / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int b = 0; b < 3; ++b) red[b][tid] += red[b][tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + (int64_t)blockIdx.x * 4;
    o[kid::XX] = red[kid::XX][0];
    o[kid::YY] = red[kid::YY][0];
    o[kid::XY] = red[kid::XY][0];
    o[3] = kid::mmd2(red[kid::XX][0], red[kid::YY][0], red[kid::XY][0], m);
  }
}

int mmd_check(const rcdm_mmd_desc* d) {
  if (d->d < 1 || d->m < 2 || d->subsets < 1 || d->nx < 1 || d->ny < 1 || d->ldx < d->d || d->ldy < d->d) return RCDM_EINVAL;
  if (d->degree < 1 || d->degree > kid::MAX_DEGREE || d->flags != 0) return RCDM_EINVAL;
  if (d->dtype != RCDM_FSTATS_F32 && d->dtype != RCDM_FSTATS_F16) return RCDM_EINVAL;
  if (d->d > kid::MAX_DIM || d->m > kid::MAX_M || d->subsets > kid::MAX_SUBSETS) return RCDM_ESHAPE;
  return RCDM_OK;
}

// the checks both entries share; a null list stands for rows 0 .. m - 1, which must exist
int mmd_operands(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy, const double* out) {
  if (!d || !x || !y || !out) return RCDM_EINVAL;
  const int rc = mmd_check(d);
  if (rc != RCDM_OK) return rc;
  const uintptr_t esz = d->dtype == RCDM_FSTATS_F16 ? 2 : 4;
  if (((uintptr_t)x & (esz - 1)) || ((uintptr_t)y & (esz - 1)) || ((uintptr_t)ix & 3) || ((uintptr_t)iy & 3) || ((uintptr_t)out & 7))
    return RCDM_EINVAL;
  if ((!ix && d->m > d->nx) || (!iy && d->m > d->ny)) return RCDM_EINVAL;
  return RCDM_OK;
}

template <bool STORE>
int mmd_launch(const rcdm_mmd_desc* d, const mmd_args& a, hipStream_t st) {
  const uintptr_t vec = d->dtype == RCDM_FSTATS_F16 ? 7 : 15;          // four elements
  const bool aligned = !(((uintptr_t)a.x | (uintptr_t)a.y) & vec) && !((a.ldx | a.ldy) & 3);
  const dim3 grid((unsigned)(a.tiles * a.tiles), STORE ? 1 : 3, STORE ? 1 : (unsigned)d->subsets), threads(NT);
  if (d->dtype == RCDM_FSTATS_F16) {
    if (aligned) hipLaunchKernelGGL((mmd_tile_kernel<f16, true, STORE>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((mmd_tile_kernel<f16, false, STORE>), grid, threads, 0, st, a);
  } else {
    if (aligned) hipLaunchKernelGGL((mmd_tile_kernel<float, true, STORE>), grid, threads, 0, st, a);
    else hipLaunchKernelGGL((mmd_tile_kernel<float, false, STORE>), grid, threads, 0, st, a);
  }
  return rcdm_check_launch();
}

mmd_args mmd_pack(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy) {
  mmd_args a;
  a.x = x;
  a.y = y;
  a.ix = ix;
  a.iy = iy;
  a.ldx = d->ldx;
  a.ldy = d->ldy;
  a.m = d->m;
  a.d = d->d;
  a.degree = d->degree;
  a.tiles = kid::tiles(d->m);
  a.gamma = d->gamma;
  a.coef0 = d->coef0;
  a.partials = nullptr;
  a.gram = nullptr;
  a.ldo = 0;
  return a;
}

}  // namespace

extern "C" {

size_t rcdm_poly_mmd_workspace_bytes(const rcdm_mmd_desc* d) {
  if (!d || mmd_check(d) != RCDM_OK) return 0;
  const size_t t = (size_t)kid::tiles(d->m);
  return (size_t)d->subsets * 3 * t * t * sizeof(double);
}

int rcdm_poly_mmd(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy, double* out,
                  void* workspace, size_t workspace_bytes, void* stream) {
  int rc = mmd_operands(d, x, y, ix, iy, out);
  if (rc != RCDM_OK) return rc;
  if ((uintptr_t)workspace & 7) return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_poly_mmd_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  mmd_args a = mmd_pack(d, x, y, ix, iy);
  a.partials = (double*)workspace;
  if ((rc = mmd_launch<false>(d, a, st)) != RCDM_OK) return rc;
  hipLaunchKernelGGL(mmd_reduce_kernel, dim3((unsigned)d->subsets), dim3(fr::LANES), 0, st, (const double*)a.partials,
                     (int64_t)a.tiles * a.tiles, d->m, out);
  return rcdm_check_launch();
}

int rcdm_poly_gram_f64(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy, double* out,
                       int64_t ldo, void* stream) {
  const int rc = mmd_operands(d, x, y, ix, iy, out);
  if (rc != RCDM_OK) return rc;
  if (ldo < d->m) return RCDM_EINVAL;
  mmd_args a = mmd_pack(d, x, y, ix, iy);
  a.gram = out;
  a.ldo = ldo;
  return mmd_launch<true>(d, a, (hipStream_t)stream);
}

}  // extern "C"
