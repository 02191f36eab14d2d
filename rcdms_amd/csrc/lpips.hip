// lpips.hip — the two kernels LPIPS needs beyond conv2d.hip (include/rcdm.h, "LPIPS"; rcdms_amd/lpips.py is the caller):
//   rcdm_lpips_head        one tap of P frame pairs: channel-normalise both feature maps, weight the squared difference by lin,
//                          mean over the pixels -> float64 per pair.  Two launches: tile partials, then one block per pair.
//                          A pixel is owned by a group of L = lp::lanes(C) lanes, 16 bytes of a and of b per lane: each row is read
//                          from HBM once, the norm and the difference come from the same registers, nothing but the tile
//                          partials (8 bytes per 64 pixels) is written.
//   rcdm_lpips_input_rows  uint8 HWC frames -> the towers' f16 input rows, scaling layer applied: the plain layout (VGG: 3
//                          channels padded to 8) or AlexNet's 11 x 11 stride-4 stem as space-to-depth rows of 48 channels.
// The summation orders are lpips_core.h's; tools/lpips_host.cpp runs the same core on the CPU.
#include "common.h"
#include "lpips_core.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_SIDE = 8192;
static_assert(NT % lp::TILE == 0 && lp::MAX_C / lp::CHUNK <= 64, "a workgroup covers a tile in whole passes, a pixel sits in one wave");

// part[t] + part[t ^ s] for s = L / 2 .. 1: lane 0 of the group (every lane, in fact) ends with lp::group_tree's part[0]
template <int L>
__device__ __forceinline__ float group_tree(float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = L / 2; s > 2; s >>= 1) v += __shfl_xor(v, s, 64);
  if constexpr (L >= 4) v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  if constexpr (L >= 2) v += dpp_f32<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  return v;
}

__device__ __forceinline__ void widen8(const Pack16& r, bool live, float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = live ? (float)r.e[e] : 0.0f;
}

template <int L>
__global__ __launch_bounds__(NT) void lpips_head_kernel(rcdm_lpips_head_desc d, int64_t hw, int64_t tiles, const f16* __restrict__ a,
                                                        const f16* __restrict__ b, const float* __restrict__ lin,
                                                        double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double vals[lp::TILE];
  constexpr int PER_PASS = NT / L;                                               // pixels per pass of the workgroup
  constexpr int PASSES = (lp::TILE + PER_PASS - 1) / PER_PASS;                   // L / 4; one pass, part of it idle, below L = 4
  const int tid = threadIdx.x, lane = tid & (L - 1), slot = tid / L;
  const bool chunk_live = lane * lp::CHUNK < d.c;
  const int col = chunk_live ? lane * lp::CHUNK : 0;
  float w[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = chunk_live ? lin[col + e] : 0.0f;
  const int64_t jobs = (int64_t)d.pairs * tiles;
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t pair = job / tiles, tile = job - pair * tiles;
    const int64_t row0 = pair * hw;
#pragma unroll(PASSES < 4 ? PASSES : 4)
    for (int pass = 0; pass < PASSES; ++pass) {
      const int q = pass * PER_PASS + slot;
      const int64_t pix = tile * lp::TILE + q;
      const bool in_tile = PER_PASS <= lp::TILE || q < lp::TILE;
      const bool live = in_tile && pix < hw && chunk_live;         // a dead lane reads a valid address and drops the value
      const int64_t row = row0 + (pix < hw ? pix : hw - 1);
      Pack16 ra, rb;
      ra.u = *(const uint4*)(a + row * d.lda + col);
      rb.u = *(const uint4*)(b + row * d.ldb + col);
      float fa[8], fb[8];
      widen8(ra, live, fa);
      widen8(rb, live, fb);
      const float na = lp::norm(group_tree<L>(lp::sumsq8(fa)));
      const float nb = lp::norm(group_tree<L>(lp::sumsq8(fb)));
      const float v = group_tree<L>(lp::term8(fa, fb, na, nb, w));
      if (lane == 0 && in_tile) vals[q] = pix < hw ? (double)v : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int s = lp::TILE / 2; s > 0; s >>= 1) {
      if (tid < s) vals[tid] += vals[tid + s];
      __syncthreads();
    }
    if (tid == 0) partials[job] = vals[0];
    __syncthreads();
  }
}

// fr's fixed sum over the tile partials of one pair, one division
__global__ __launch_bounds__(NT) void lpips_pair_kernel(int64_t hw, int64_t tiles, const double* __restrict__ partials,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double part[NT];
  const int tid = threadIdx.x;
  const double* p = partials + (int64_t)blockIdx.x * tiles;
  double s = 0.0;
  for (int64_t k = tid; k < tiles; k += NT) s += p[k];
  part[tid] = s;
  __syncthreads();
#pragma unroll
  for (int st = NT / 2; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = lp::pair_mean(part[0], hw);
}

// one thread per (output row, chunk of 8 channels).  space_to_depth == 1: channel j < 3 of pixel (Y, X) is source (Y, X, j).
// space_to_depth == 4: channel j = (dy 4 + dx) 3 + ch of cell (Y, X) is source (4 Y + dy - 2, 4 X + dx - 2, ch); outside: 0.
__global__ __launch_bounds__(NT) void lpips_input_kernel(rcdm_lpips_input_desc d, int out_h, int out_w, int chunks, size_t total,
                                                         const uint8_t* __restrict__ src, f16* __restrict__ dst) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const size_t rowi = i / chunks;
  const int chunk = (int)(i - rowi * chunks);
  const size_t hw = (size_t)out_h * out_w;
  const size_t img = rowi / hw, rem = rowi - img * hw;
  const int Y = (int)(rem / out_w), X = (int)(rem - (size_t)Y * out_w);
  const uint8_t* s = src + img * (size_t)d.src_stride;
  Pack16 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int j = chunk * 8 + e;
    int sy, sx, ch;
    bool in;
    if (d.space_to_depth == 1) {
      sy = Y, sx = X, ch = j;
      in = j < 3;
    } else {
      const int cell = j / 3;
      ch = j - 3 * cell;
      sy = 4 * Y + (cell >> 2) - 2;
      sx = 4 * X + (cell & 3) - 2;
      in = sy >= 0 && sy < d.in_h && sx >= 0 && sx < d.in_w;
    }
    float t = 0.0f;
    if (in) t = __builtin_fmaf((float)s[(size_t)sy * (size_t)d.src_pitch + 3 * (size_t)sx + ch] / 255.0f, d.mul[ch], d.add[ch]);
    v.e[e] = (f16)t;
  }
  *(uint4*)(dst + rowi * (size_t)d.ld + (size_t)chunk * 8) = v.u;
}

int head_check(const rcdm_lpips_head_desc* d) {
  if (d->pairs <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->lda < d->c || d->ldb < d->c || d->blocks < 0) return RCDM_EINVAL;
  if ((d->c & 7) || (d->lda & 7) || (d->ldb & 7) || d->c > lp::MAX_C || d->pairs > lp::MAX_PAIRS || d->h > MAX_SIDE || d->w > MAX_SIDE)
    return RCDM_ESHAPE;
  return RCDM_OK;
}

int input_sides(const rcdm_lpips_input_desc* d, int& out_h, int& out_w, int& c_row) {
  if (d->n <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->src_pitch < 3 * (int64_t)d->in_w || d->src_stride < 0) return RCDM_EINVAL;
  if (d->in_h > MAX_SIDE || d->in_w > MAX_SIDE) return RCDM_ESHAPE;
  if (d->space_to_depth == 1) {
    out_h = d->in_h, out_w = d->in_w, c_row = 8;
  } else if (d->space_to_depth == 4) {
    if (d->in_h < 7 || d->in_w < 7) return RCDM_ESHAPE;
    out_h = (d->in_h - 7) / 4 + 3, out_w = (d->in_w - 7) / 4 + 3, c_row = 48;
  } else {
    return RCDM_ESHAPE;
  }
  if ((d->ld & 7) || d->ld < c_row) return RCDM_EINVAL;
  return RCDM_OK;
}

}  // namespace

extern "C" {

size_t rcdm_lpips_head_workspace_bytes(const rcdm_lpips_head_desc* d) {
  if (!d || head_check(d) != RCDM_OK) return 0;
  return (size_t)d->pairs * (size_t)lp::tiles((int64_t)d->h * d->w) * sizeof(double);
}

int rcdm_lpips_head(const rcdm_lpips_head_desc* d, const void* a, const void* b, const float* lin, double* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!d || !a || !b || !lin || !out || !workspace) return RCDM_EINVAL;
  const int rc = head_check(d);
  if (rc != RCDM_OK) return rc;
  if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)lin | (uintptr_t)workspace) & 15) || ((uintptr_t)out & 7)) return RCDM_EINVAL;
  if (workspace_bytes < rcdm_lpips_head_workspace_bytes(d)) return RCDM_EWORKSPACE;
  const int64_t hw = (int64_t)d->h * d->w, tiles = lp::tiles(hw), jobs = (int64_t)d->pairs * tiles;
  int64_t blocks = d->blocks > 0 ? d->blocks : 8 * (int64_t)rcdm_num_cus();
  if (blocks > jobs) blocks = jobs;
  const dim3 grid((unsigned)blocks), block(NT);
  const f16* pa = (const f16*)a;
  const f16* pb = (const f16*)b;
  double* ws = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  switch (lp::lanes(d->c)) {
    case 1: hipLaunchKernelGGL(lpips_head_kernel<1>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    case 2: hipLaunchKernelGGL(lpips_head_kernel<2>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    case 4: hipLaunchKernelGGL(lpips_head_kernel<4>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    case 8: hipLaunchKernelGGL(lpips_head_kernel<8>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    case 16: hipLaunchKernelGGL(lpips_head_kernel<16>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    case 32: hipLaunchKernelGGL(lpips_head_kernel<32>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
    default: hipLaunchKernelGGL(lpips_head_kernel<64>, grid, block, 0, st, *d, hw, tiles, pa, pb, lin, ws); break;
  }
  const int rl = rcdm_check_launch();
  if (rl != RCDM_OK) return rl;
  hipLaunchKernelGGL(lpips_pair_kernel, dim3((unsigned)d->pairs), block, 0, st, hw, tiles, (const double*)ws, out);
  return rcdm_check_launch();
}

int rcdm_lpips_input_sides(const rcdm_lpips_input_desc* d, int32_t* out_h, int32_t* out_w, int32_t* channels) {
  if (!d || !out_h || !out_w || !channels) return RCDM_EINVAL;
  int h = 0, w = 0, c = 0;
  const int rc = input_sides(d, h, w, c);
  if (rc != RCDM_OK) return rc;
  *out_h = h, *out_w = w, *channels = c;
  return RCDM_OK;
}

int rcdm_lpips_input_rows(const rcdm_lpips_input_desc* d, const void* src_u8, void* dst, void* stream) {
  if (!d || !src_u8 || !dst) return RCDM_EINVAL;
  int out_h = 0, out_w = 0, c_row = 0;
  const int rc = input_sides(d, out_h, out_w, c_row);
  if (rc != RCDM_OK) return rc;
  if ((uintptr_t)dst & 15) return RCDM_EINVAL;
  for (int ch = 0; ch < 3; ++ch)
    if (!(d->mul[ch] == d->mul[ch]) || !(d->add[ch] == d->add[ch])) return RCDM_EINVAL;
  const int chunks = c_row / 8;
  const size_t total = (size_t)d->n * out_h * out_w * (size_t)chunks;
  const size_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffffu) return RCDM_ESHAPE;
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *d, out_h, out_w, chunks, total,
                     (const uint8_t*)src_u8, (f16*)dst);
  return rcdm_check_launch();
}

}  // extern "C"
