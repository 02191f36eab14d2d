// metrics.hip — per-frame quality figures of a story on the device (include/rcdm.h, "Frame metrics").
//   rcdm_frame_metrics  n pairs of uint8 HWC RGB images -> per pair and channel the mean SSIM (scikit-image's definition, box
//                       7 x 7 or Gaussian 11 x 11 window) in float64 and the exact integer sums of squared and absolute
//                       differences.  Two launches: a tile kernel that leaves nine partial sums per block in the workspace,
//                       and a finish kernel that adds each figure's partials in block-index order.
// A block owns TH x TW map values (a map value = one window position) of one pair, all three channels: it stages the two
// uint8 tiles with their win - 1 halo in LDS (byte loads: neither base nor pitch is aligned), runs the horizontal pass of
// the five window sums into LDS (int32 for the box, double for the Gaussian), then the vertical pass + the map value per
// thread.  Items are (row, byte column) with 3 TW byte columns per row and NT a multiple of 3, so a thread's channel is
// tid % 3 throughout and it keeps ONE accumulator per figure.  Nothing is atomic and no order depends on timing: the same
// inputs give the same bits.  The arithmetic itself is ssim_core.h, shared with tools/ssim_host.cpp.
// TH = 20 and TW = 12 divide none of the sizes the tests use, so every test has ragged tiles on both axes.
#include <type_traits>

#include "common.h"
#include "ssim_core.h"

namespace {

constexpr int TH = 20, TW = 12;         // map values per tile: rows, columns
constexpr int CW = 3 * TW;              // byte columns of a tile's results
constexpr int NT = 192;                 // a multiple of 3: idx % 3 == tid % 3 for idx = tid + k NT
constexpr int FIGURES = 9;              // per pair: ssim[3], sse[3], sad[3]
constexpr int MAX_SIDE = 8192;
constexpr int FINISH_NT = 256, FINISH_CHUNK = 1024;

template <int WIN, bool BOX>
__global__ __launch_bounds__(NT) void metrics_tile_kernel(rcdm_metrics_desc d, const uint8_t* __restrict__ a,
                                                          const uint8_t* __restrict__ b, const double* __restrict__ win, double cn,
                                                          double* __restrict__ part) {
  typedef typename std::conditional<BOX, int32_t, double>::type T;
  constexpr int PAD = (WIN - 1) / 2, ROWS = TH + WIN - 1, PB = 3 * (TW + WIN - 1);
  __shared__ uint8_t ta[ROWS * PB], tb[ROWS * PB];     // the two tiles with their halo
  __shared__ T inter[5][ROWS][CW];                     // horizontal pass: quantity, tile row, byte column
  __shared__ double red[NT];
  __shared__ int32_t redi[2][NT];
  __shared__ double sw[WIN];
  const int tid = threadIdx.x, img = blockIdx.z;
  const int mh = d.H - WIN + 1, mw = d.W - WIN + 1;    // the map: window positions inside the image
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int tw = min(TW, mw - x0), th = min(TH, mh - y0);
  const int rows = th + WIN - 1, pbw = 3 * (tw + WIN - 1), cw = 3 * tw;

  if (!BOX && tid < WIN) sw[tid] = win[tid];
  // stage image rows y0 .. y0 + rows, bytes 3 x0 .. 3 x0 + pbw: x0 + tw + WIN - 1 <= W, so no byte beyond 3 W of a row is read
  const uint8_t* pa = a + (size_t)img * (size_t)d.a_stride + (size_t)y0 * (size_t)d.a_pitch + 3 * x0;
  const uint8_t* pb = b + (size_t)img * (size_t)d.b_stride + (size_t)y0 * (size_t)d.b_pitch + 3 * x0;
  // every load of the thread is issued before the first one is waited for: LOADS independent byte loads per side in flight
  constexpr int LOADS = (ROWS * PB + NT - 1) / NT;
  uint8_t va[LOADS], vb[LOADS];
#pragma unroll
  for (int k = 0; k < LOADS; ++k) {
    const int idx = tid + k * NT, r = idx / pbw, j = idx - r * pbw;
    const bool live = idx < rows * pbw;
    va[k] = live ? pa[(size_t)r * (size_t)d.a_pitch + j] : (uint8_t)0;
    vb[k] = live ? pb[(size_t)r * (size_t)d.b_pitch + j] : (uint8_t)0;
  }
#pragma unroll
  for (int k = 0; k < LOADS; ++k) {
    const int idx = tid + k * NT, r = idx / pbw, j = idx - r * pbw;
    if (idx < rows * pbw) {
      ta[r * PB + j] = va[k];
      tb[r * PB + j] = vb[k];
    }
  }
  __syncthreads();

  // squared and absolute differences over the pixels this tile owns: its map values' centres, plus the image border next to
  // a first / last tile — the tiles' regions cover every pixel of the image once
  const int ry0 = blockIdx.y == 0 ? 0 : PAD, ry1 = blockIdx.y == gridDim.y - 1 ? rows : PAD + th;
  const int rx0 = blockIdx.x == 0 ? 0 : PAD, rx1 = blockIdx.x == gridDim.x - 1 ? tw + WIN - 1 : PAD + tw;
  const int rw = 3 * (rx1 - rx0);
  int32_t sse = 0, sad = 0;
  for (int idx = tid; idx < (ry1 - ry0) * rw; idx += NT) {
    const int r = idx / rw, j = idx - r * rw;
    const int at = (ry0 + r) * PB + 3 * rx0 + j;
    const int df = (int)ta[at] - (int)tb[at];
    sse += df * df;
    sad += df < 0 ? -df : df;
  }

  // horizontal pass
  for (int idx = tid; idx < rows * cw; idx += NT) {
    const int r = idx / cw, j = idx - r * cw;
    T s[5];
    if constexpr (BOX) ssim::row_sums_box<WIN>(ta + r * PB + j, tb + r * PB + j, 3, s);
    else ssim::row_sums_weighted<WIN>(ta + r * PB + j, tb + r * PB + j, 3, sw, s);
#pragma unroll
    for (int q = 0; q < 5; ++q) inter[q][r][j] = s[q];
  }
  __syncthreads();

  // vertical pass and the map value; a thread's items come in ascending order
  double acc = 0.0;
  for (int idx = tid; idx < th * cw; idx += NT) {
    const int y = idx / cw, j = idx - y * cw;
    T s[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      if constexpr (BOX) s[q] = ssim::col_sum_box<WIN>(&inter[q][y][j], CW);
      else s[q] = ssim::col_sum_weighted<WIN>(&inter[q][y][j], CW, sw);
    }
    if constexpr (BOX) acc += ssim::map_value_box(s, WIN, cn);
    else acc += ssim::map_value_weighted(s, cn);
  }
  red[tid] = acc;
  redi[0][tid] = sse;
  redi[1][tid] = sad;
  __syncthreads();
  if (tid < FIGURES) {               // figure tid = kind * 3 + channel: threads c, c + 3, ... in ascending order
    const int kind = tid / 3, c = tid - 3 * kind;
    const size_t nblk = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    double* o = part + ((size_t)img * FIGURES + tid) * nblk + blk;
    if (kind == 0) {
      double s = 0.0;
      for (int k = c; k < NT; k += 3) s += red[k];
      *o = s;
    } else {
      int64_t s = 0;
      for (int k = c; k < NT; k += 3) s += redi[kind - 1][k];
      *(int64_t*)o = s;
    }
  }
}

// one block per (pair, figure): the figure's per-tile partials are added in tile-index order by one thread, staged through
// LDS FINISH_CHUNK at a time
__global__ __launch_bounds__(FINISH_NT) void metrics_finish_kernel(const uint64_t* __restrict__ part, int nblk, double count,
                                                                   double* __restrict__ ssim_out, int64_t* __restrict__ sse,
                                                                   int64_t* __restrict__ sad) {
  __shared__ uint64_t buf[FINISH_CHUNK];     // a partial is 8 bytes: a double (ssim) or an int64 (sse, sad)
  const int img = blockIdx.x, fig = blockIdx.y, tid = threadIdx.x;
  const int kind = fig / 3, c = fig - 3 * kind;
  const uint64_t* p = part + ((size_t)img * FIGURES + fig) * (size_t)nblk;
  double fs = 0.0;
  int64_t is = 0;
  for (int base = 0; base < nblk; base += FINISH_CHUNK) {
    const int m = min(FINISH_CHUNK, nblk - base);
    for (int k = tid; k < m; k += FINISH_NT) buf[k] = p[base + k];
    __syncthreads();
    if (tid == 0) {
      if (kind == 0)
        for (int k = 0; k < m; ++k) fs += __longlong_as_double((long long)buf[k]);
      else
        for (int k = 0; k < m; ++k) is += (int64_t)buf[k];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (kind == 0) ssim_out[img * 3 + c] = fs / count;
    else if (kind == 1) sse[img * 3 + c] = is;
    else sad[img * 3 + c] = is;
  }
}

int window_side(int window) {
  return window == RCDM_SSIM_UNIFORM7 ? ssim::UNIFORM_WIN : window == RCDM_SSIM_GAUSS11 ? ssim::GAUSS_WIN : 0;
}

// 0 when the descriptor is one the kernels take, else the status to return
int metrics_check(const rcdm_metrics_desc* d) {
  if (d->n <= 0 || d->H <= 0 || d->W <= 0) return RCDM_EINVAL;
  const int win = window_side(d->window);
  if (!win) return RCDM_EINVAL;
  if (d->channels != 3 || d->H < win || d->W < win || d->H > MAX_SIDE || d->W > MAX_SIDE || d->n > 65535) return RCDM_ESHAPE;
  if (d->a_pitch < 3 * (int64_t)d->W || d->b_pitch < 3 * (int64_t)d->W || d->a_stride < 0 || d->b_stride < 0) return RCDM_EINVAL;
  return RCDM_OK;
}

dim3 metrics_grid(const rcdm_metrics_desc* d) {
  const int win = window_side(d->window);
  return dim3((d->W - win + 1 + TW - 1) / TW, (d->H - win + 1 + TH - 1) / TH, d->n);
}

}  // namespace

extern "C" {

size_t rcdm_frame_metrics_workspace_bytes(const rcdm_metrics_desc* d) {
  if (!d || metrics_check(d) != RCDM_OK) return 0;
  const dim3 g = metrics_grid(d);
  return (size_t)g.x * g.y * g.z * FIGURES * sizeof(double);
}

int rcdm_frame_metrics(const rcdm_metrics_desc* d, const void* a, const void* b, const double* win, double* ssim_out, int64_t* sse,
                       int64_t* sad, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !a || !b || !ssim_out || !sse || !sad) return RCDM_EINVAL;
  const int rc = metrics_check(d);
  if (rc != RCDM_OK) return rc;
  if (d->window == RCDM_SSIM_GAUSS11 && !win) return RCDM_EINVAL;
  if (((uintptr_t)win | (uintptr_t)ssim_out | (uintptr_t)sse | (uintptr_t)sad | (uintptr_t)workspace) & 7) return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_frame_metrics_workspace_bytes(d)) return RCDM_EWORKSPACE;
  const dim3 grid = metrics_grid(d);
  const int nblk = (int)(grid.x * grid.y);
  const int side = window_side(d->window);
  const double cn = ssim::cov_norm(side, d->sample_covariance);
  const double count = (double)(d->H - side + 1) * (double)(d->W - side + 1);
  const uint8_t *pa = (const uint8_t*)a, *pb = (const uint8_t*)b;
  double* part = (double*)workspace;
  if (d->window == RCDM_SSIM_UNIFORM7)
    hipLaunchKernelGGL((metrics_tile_kernel<ssim::UNIFORM_WIN, true>), grid, dim3(NT), 0, (hipStream_t)stream, *d, pa, pb, win, cn, part);
  else
    hipLaunchKernelGGL((metrics_tile_kernel<ssim::GAUSS_WIN, false>), grid, dim3(NT), 0, (hipStream_t)stream, *d, pa, pb, win, cn, part);
  int st = rcdm_check_launch();
  if (st != RCDM_OK) return st;
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(d->n, FIGURES), dim3(FINISH_NT), 0, (hipStream_t)stream, (const uint64_t*)part, nblk, count, ssim_out, sse,
                     sad);
  return rcdm_check_launch();
}

}  // extern "C"
