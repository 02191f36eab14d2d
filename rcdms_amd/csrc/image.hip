// image.hip — the 8-bit image front and back end of the story pipeline (include/rcdm.h, "Images").
//   rcdm_image_resample  Pillow's ImagingResample for 8-bit channels (integer coefficients of 22 fractional bits, horizontal
//                        pass rounded to uint8, vertical pass over that), both passes in one launch: a block owns a
//                        32 x 32 output tile, runs the horizontal pass for the source rows the tile needs into LDS as uint8
//                        and the vertical pass out of LDS, so the intermediate image never exists in HBM.
//   rcdm_frames_to_u8    decoder output (f16 pixel rows or fp32 NCHW) -> uint8 HWC, the pipeline's
//                        (x / 2 + 0.5).clamp(0, 1) * 255 truncated, at a caller-given pitch / image stride.
// Both are byte movers: a story is 5 frames, the source of a resample (48 KB a frame) lives in L2, the coefficient rows of a
// tile are staged in LDS once.  The kernels trust NO value of the device tables: every bound read from them is clamped to
// the source image and to the staged rows before it addresses anything.
#include "common.h"

namespace {

constexpr int TILE = RCDM_IMAGE_TILE;   // output tile side
constexpr int ROWB = TILE * 3;          // bytes of one staged row: TILE pixels x 3 channels
constexpr int NT = 256;
constexpr int MAX_TAPS = 40;
constexpr int MAX_SIDE = 8192;
constexpr size_t MAX_LDS = 64 * 1024;

struct NormArgs {
  float mean[3], istd[3];
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;              // arithmetic shift, as Pillow's clip8
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (u8 * (1/255) - mean) * (1/std): three roundings after the two rounded constants, never contracted — the f16 rows of
// mode 2 are this value rounded once more, bit for bit what mode 1 stores
__device__ __forceinline__ float norm_px(int u, float mean, float istd) {
#pragma clang fp contract(off)
  float t = (float)u * (1.0f / 255.0f);
  t = t - mean;
  return t * istd;
}

// trunc(clamp(x * 0.5 + 0.5, 0, 1) * 255): the multiply by 255 is its own rounding (numpy's `* 255` on the clamped fp32
// array); fmaxf drops a NaN, so NaN -> 0
__device__ __forceinline__ uint8_t unit_to_u8(float x) {
#pragma clang fp contract(off)
  float t = x * 0.5f;
  t = t + 0.5f;
  t = __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f);
  t = t * 255.0f;
  return (uint8_t)(int)t;
}

template <int MODE>
__global__ __launch_bounds__(NT) void image_resample_kernel(rcdm_resample_desc d, NormArgs nrm, const uint8_t* __restrict__ src,
                                                            const int32_t* __restrict__ kx, const int32_t* __restrict__ bx,
                                                            const int32_t* __restrict__ ky, const int32_t* __restrict__ by,
                                                            void* __restrict__ dst) {
  extern __shared__ int32_t smem[];
  const int tx = d.taps_x, ty = d.taps_y;
  int32_t* skx = smem;                    // [TILE][tx] coefficients of the tile's columns
  int32_t* sky = skx + TILE * tx;         // [TILE][ty] ... and rows
  int32_t* sbx = sky + TILE * ty;         // [TILE][2] (first source column, count), clamped
  int32_t* sby = sbx + TILE * 2;          // [TILE][2] (first source row, count), clamped
  uint8_t* inter = (uint8_t*)(sby + TILE * 2);   // [tile_rows][ROWB] horizontal pass of the rows this tile reads
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, img = blockIdx.z;
  const int tw = min(TILE, d.out_w - x0), th = min(TILE, d.out_h - y0);

  for (int i = tid; i < tw * tx; i += NT) skx[i] = kx[(size_t)x0 * tx + i];
  for (int i = tid; i < th * ty; i += NT) sky[i] = ky[(size_t)y0 * ty + i];
  if (tid < tw) {
    int lo = bx[2 * (x0 + tid)], n = bx[2 * (x0 + tid) + 1];
    lo = max(0, min(lo, d.in_w - 1));
    n = max(0, min(n, min(tx, d.in_w - lo)));
    sbx[2 * tid] = lo;
    sbx[2 * tid + 1] = n;
  } else if (tid >= 64 && tid - 64 < th) {
    const int t = tid - 64;
    int lo = by[2 * (y0 + t)], n = by[2 * (y0 + t) + 1];
    lo = max(0, min(lo, d.in_h - 1));
    n = max(0, min(n, min(ty, d.in_h - lo)));
    sby[2 * t] = lo;
    sby[2 * t + 1] = n;
  }
  __syncthreads();
  // source rows of this tile: [r0, r0 + span), never more than the rows the launch has LDS for
  int r0 = d.in_h, r1 = 0;
  for (int i = 0; i < th; ++i) {
    r0 = min(r0, sby[2 * i]);
    r1 = max(r1, sby[2 * i] + sby[2 * i + 1]);
  }
  const int span = max(0, min(r1 - r0, d.tile_rows));

  // horizontal pass: source rows r0 .. r0 + span, the tile's columns, rounded to uint8
  const uint8_t* s = src + (size_t)img * (size_t)d.src_stride;
  for (int idx = tid; idx < span * ROWB; idx += NT) {
    const int r = idx / ROWB, rem = idx - r * ROWB;
    const int x = rem / 3, c = rem - 3 * x;
    int v = 0;
    if (x < tw) {
      const int lo = sbx[2 * x], n = sbx[2 * x + 1];
      const uint8_t* p = s + (size_t)(r0 + r) * (size_t)d.src_pitch + lo * 3 + c;
      const int32_t* k = skx + x * tx;
      int acc = 1 << 21;
      for (int i = 0; i < n; ++i) acc += (int)p[3 * i] * k[i];
      v = clip8(acc);
    }
    inter[idx] = (uint8_t)v;
  }
  __syncthreads();

  // vertical pass out of LDS.  column(y, j): j = 3 x + c of the staged row
  auto column = [&](int y, int j) {
    const int lo = sby[2 * y] - r0;
    const int n = min(sby[2 * y + 1], span - lo);
    const int32_t* k = sky + y * ty;
    int acc = 1 << 21;
    for (int i = 0; i < n; ++i) acc += (int)inter[(lo + i) * ROWB + j] * k[i];
    return clip8(acc);
  };
  if constexpr (MODE == RCDM_IMAGE_U8) {            // uint8 HWC: consecutive threads store consecutive bytes of a row
    uint8_t* o = (uint8_t*)dst + (size_t)img * (size_t)d.dst_stride;
    for (int idx = tid; idx < th * ROWB; idx += NT) {
      const int y = idx / ROWB, rem = idx - y * ROWB;
      const int x = rem / 3, c = rem - 3 * x;
      if (x >= tw) continue;
      const int cc = d.flip_channels ? 2 - c : c;
      o[(size_t)(y0 + y) * (size_t)d.dst_pitch + (size_t)(x0 + x) * 3 + cc] = (uint8_t)column(y, rem);
    }
  } else if constexpr (MODE == RCDM_IMAGE_F32_NCHW) {   // fp32 planes: x fastest, so a wave stores runs of 32 floats
    float* o = (float*)dst + (size_t)img * 3 * d.out_h * d.out_w;
    for (int idx = tid; idx < 3 * TILE * TILE; idx += NT) {
      const int c = idx / (TILE * TILE), rem = idx - c * (TILE * TILE);
      const int y = rem / TILE, x = rem - y * TILE;
      if (y >= th || x >= tw) continue;
      const int cc = d.flip_channels ? 2 - c : c;
      o[((size_t)cc * d.out_h + (y0 + y)) * d.out_w + (x0 + x)] = norm_px(column(y, 3 * x + c), nrm.mean[cc], nrm.istd[cc]);
    }
  } else {                                          // f16 pixel rows: one 16-byte store per 8 channels, pad channels zero
    f16* o = (f16*)dst + (size_t)img * d.out_h * d.out_w * d.ld;
    for (int p = tid; p < TILE * TILE; p += NT) {
      const int y = p / TILE, x = p - y * TILE;
      if (y >= th || x >= tw) continue;
      const int a = column(y, 3 * x), b = column(y, 3 * x + 1), c = column(y, 3 * x + 2);
      Pack16 v;
      v.u = make_uint4(0, 0, 0, 0);
      v.e[0] = (f16)norm_px(d.flip_channels ? c : a, nrm.mean[0], nrm.istd[0]);
      v.e[1] = (f16)norm_px(b, nrm.mean[1], nrm.istd[1]);
      v.e[2] = (f16)norm_px(d.flip_channels ? a : c, nrm.mean[2], nrm.istd[2]);
      uint4* row = (uint4*)(o + ((size_t)(y0 + y) * d.out_w + (x0 + x)) * d.ld);
      row[0] = v.u;
      for (int j = 1; j < d.c_pad / 8; ++j) row[j] = make_uint4(0, 0, 0, 0);
    }
  }
}

template <int SRC>
__global__ __launch_bounds__(NT) void frames_to_u8_kernel(rcdm_frames_u8_desc d, const void* __restrict__ src, uint8_t* __restrict__ dst) {
  const size_t hw = (size_t)d.H * d.W, total = hw * d.n;
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  const size_t img = p / hw, rem = p - img * hw;
  const int y = (int)(rem / d.W), x = (int)(rem - (size_t)y * d.W);
  float v[3];
  if constexpr (SRC == RCDM_FRAMES_F16_ROWS) {
    const f16* r = (const f16*)src + p * d.ld;
    for (int c = 0; c < 3; ++c) v[c] = (float)r[c];
  } else {
    const float* f = (const float*)src + img * 3 * hw + rem;
    for (int c = 0; c < 3; ++c) v[c] = f[c * hw];
  }
  uint8_t* o = dst + img * (size_t)d.dst_stride + (size_t)y * (size_t)d.dst_pitch + (size_t)x * 3;
  for (int c = 0; c < 3; ++c) o[c] = unit_to_u8(v[c]);
}

// 0 when the descriptor is one the kernel takes, else the status to return
int resample_check(const rcdm_resample_desc* d) {
  if (d->n <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->out_h <= 0 || d->out_w <= 0 || d->taps_x <= 0 || d->taps_y <= 0 ||
      d->tile_rows <= 0)
    return RCDM_EINVAL;
  if (d->channels != 3 || d->taps_x > MAX_TAPS || d->taps_y > MAX_TAPS || d->in_h > MAX_SIDE || d->in_w > MAX_SIDE ||
      d->out_h > MAX_SIDE || d->out_w > MAX_SIDE || d->n > 65535)
    return RCDM_ESHAPE;
  if (d->src_pitch < 3 * (int64_t)d->in_w || d->src_stride < 0) return RCDM_EINVAL;
  if (d->mode == RCDM_IMAGE_U8) {
    if (d->dst_pitch < 3 * (int64_t)d->out_w || d->dst_stride < 0) return RCDM_EINVAL;
  } else if (d->mode == RCDM_IMAGE_F32_NCHW || d->mode == RCDM_IMAGE_F16_ROWS) {
    for (int c = 0; c < 3; ++c)
      if (!(d->std[c] > 0.0f) || !(d->mean[c] == d->mean[c])) return RCDM_EINVAL;
    if (d->mode == RCDM_IMAGE_F16_ROWS && (d->c_pad < 8 || (d->c_pad & 7) || (d->ld & 7) || d->ld < d->c_pad)) return RCDM_EINVAL;
  } else {
    return RCDM_EINVAL;
  }
  return RCDM_OK;
}

size_t resample_lds(const rcdm_resample_desc* d) {
  return (size_t)(TILE * d->taps_x + TILE * d->taps_y + 4 * TILE) * sizeof(int32_t) + (size_t)d->tile_rows * ROWB;
}

}  // namespace

extern "C" {

size_t rcdm_image_resample_lds_bytes(const rcdm_resample_desc* d) {
  if (!d || resample_check(d) != RCDM_OK) return 0;
  return resample_lds(d);
}

int rcdm_image_resample(const rcdm_resample_desc* d, const void* src, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                        const int32_t* by, void* dst, void* stream) {
  if (!d || !src || !kx || !bx || !ky || !by || !dst) return RCDM_EINVAL;
  const int rc = resample_check(d);
  if (rc != RCDM_OK) return rc;
  if (d->mode == RCDM_IMAGE_F16_ROWS && ((uintptr_t)dst & 15)) return RCDM_EINVAL;
  if (d->mode == RCDM_IMAGE_F32_NCHW && ((uintptr_t)dst & 3)) return RCDM_EINVAL;
  if (((uintptr_t)kx | (uintptr_t)bx | (uintptr_t)ky | (uintptr_t)by) & 3) return RCDM_EINVAL;
  const size_t lds = resample_lds(d);
  if (lds > MAX_LDS) return RCDM_ESHAPE;
  NormArgs nrm;
  for (int c = 0; c < 3; ++c) {
    nrm.mean[c] = d->mode == RCDM_IMAGE_U8 ? 0.0f : d->mean[c];
    nrm.istd[c] = d->mode == RCDM_IMAGE_U8 ? 1.0f : 1.0f / d->std[c];
  }
  const dim3 grid((d->out_w + TILE - 1) / TILE, (d->out_h + TILE - 1) / TILE, d->n);
  const uint8_t* s = (const uint8_t*)src;
  if (d->mode == RCDM_IMAGE_U8)
    hipLaunchKernelGGL(image_resample_kernel<RCDM_IMAGE_U8>, grid, dim3(NT), lds, (hipStream_t)stream, *d, nrm, s, kx, bx, ky, by, dst);
  else if (d->mode == RCDM_IMAGE_F32_NCHW)
    hipLaunchKernelGGL(image_resample_kernel<RCDM_IMAGE_F32_NCHW>, grid, dim3(NT), lds, (hipStream_t)stream, *d, nrm, s, kx, bx, ky,
                       by, dst);
  else
    hipLaunchKernelGGL(image_resample_kernel<RCDM_IMAGE_F16_ROWS>, grid, dim3(NT), lds, (hipStream_t)stream, *d, nrm, s, kx, bx, ky,
                       by, dst);
  return rcdm_check_launch();
}

int rcdm_frames_to_u8(const rcdm_frames_u8_desc* d, const void* src, void* dst, void* stream) {
  if (!d || !src || !dst) return RCDM_EINVAL;
  if (d->n <= 0 || d->H <= 0 || d->W <= 0) return RCDM_EINVAL;
  if (d->channels != 3 || d->H > MAX_SIDE || d->W > MAX_SIDE) return RCDM_ESHAPE;
  if (d->dst_pitch < 3 * (int64_t)d->W || d->dst_stride < 0) return RCDM_EINVAL;
  if (d->src_kind != RCDM_FRAMES_F16_ROWS && d->src_kind != RCDM_FRAMES_F32_NCHW) return RCDM_EINVAL;
  if (d->src_kind == RCDM_FRAMES_F16_ROWS && (d->ld < 3 || ((uintptr_t)src & 1))) return RCDM_EINVAL;
  if (d->src_kind == RCDM_FRAMES_F32_NCHW && ((uintptr_t)src & 3)) return RCDM_EINVAL;
  const size_t total = (size_t)d->n * d->H * d->W;
  const size_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffffu) return RCDM_ESHAPE;
  if (d->src_kind == RCDM_FRAMES_F16_ROWS)
    hipLaunchKernelGGL(frames_to_u8_kernel<RCDM_FRAMES_F16_ROWS>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *d, src,
                       (uint8_t*)dst);
  else
    hipLaunchKernelGGL(frames_to_u8_kernel<RCDM_FRAMES_F32_NCHW>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *d, src,
                       (uint8_t*)dst);
  return rcdm_check_launch();
}

}  // extern "C"
