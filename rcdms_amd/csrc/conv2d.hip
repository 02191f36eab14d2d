// conv2d.hip — the kernels an Inception-v3 forward needs on top of the library (include/rcdm.h, "General conv2d, pools"):
//   rcdm_conv2d               kh x kw convolution (<= 7 x 7, stride 1 | 2, zero padding) as an implicit GEMM on
//                             v_mfma_f32_16x16x32_f16: a 4-wave block owns a 64 x 64 output tile (waves 2 x 2, a 32 x 32
//                             quarter each), the k-loop steps 32 deep through two LDS stages that are filled from registers:
//                             the operand chunks of step s + 1 are loaded (global -> VGPR) before the MFMAs of step s and
//                             written to the other stage after them, one barrier per step.  A thread stages ONE 16-byte
//                             chunk of each operand per step: c_in % 8 == 0, so a chunk never straddles a tap and a tap
//                             outside the image (or a row >= M, a column >= c_out, a k >= K) is a chunk of zeros.
//                             Epilogue (bias, ReLU) in fp32 on the accumulators, rounded once, tile staged in LDS and stored
//                             in 16-byte pieces.
//   rcdm_pool2d               max / average pooling, window <= 3 x 3, a thread per (output pixel, 8 channels)
//   rcdm_global_avgpool       fp32 mean over the rows of each image, a thread per (image, 8 channels), rows in order
//   rcdm_image_bilinear_rows  uint8 HWC frames -> f16 pixel rows, torch's bilinear (align_corners = False, no antialias)
// No atomics anywhere: the same input gives the same bits.  Every row and byte offset is 64-bit.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BM = 64, BN = 64, BK = 32;
constexpr int LDT = BK + 8;        // halves per staged row: 80 bytes, so the 16 rows of a fragment read spread over the banks
constexpr int LDO = BN + 8;        // halves per row of the staged output tile
constexpr int MAX_K = 7;
constexpr int MAX_SIDE = 8192;

static_assert(2 * (BM + BN) * LDT >= BM * LDO, "the output tile is staged in the operand stages");

__device__ __forceinline__ float relu_f(float v) { return v > 0.0f ? v : (v != v ? v : 0.0f); }   // NaN stays NaN, -0.0 -> +0.0

__global__ __launch_bounds__(NT) void conv2d_kernel(rcdm_conv2d_desc d, int h_out, int w_out, int M, int K,
                                                    const f16* __restrict__ in, const f16* __restrict__ W,
                                                    const float* __restrict__ bias, f16* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) f16 smem[2 * (BM + BN) * LDT];
  constexpr int STAGE = (BM + BN) * LDT;   // halves of one stage: the A rows, then the W rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  // the operand chunks this thread stages: row sr of the tile, halves sk .. sk + 7 of the k-step
  const int sr = tid >> 2, sk = (tid & 3) * 8;
  const int m = m0 + sr;
  const bool m_ok = m < M;
  int iy0 = 0, ix0 = 0;
  const f16* img_base = in;
  if (m_ok) {
    const int hw = h_out * w_out;
    const int img = m / hw, rem = m - img * hw;
    const int oy = rem / w_out, ox = rem - oy * w_out;
    iy0 = oy * d.stride_h - d.pad_h;
    ix0 = ox * d.stride_w - d.pad_w;
    img_base = in + (size_t)img * d.h_in * d.w_in * (size_t)d.lda;
  }
  const int n = n0 + sr;
  const bool n_ok = n < d.c_out;
  const f16* w_row = W + (size_t)(n_ok ? n : 0) * (size_t)K;
  // (ky, kx, c) of this thread's chunk, advanced by BK channels per step
  int c = sk, kx = 0, ky = 0;
  while (c >= d.c_in) {
    c -= d.c_in;
    if (++kx == d.kw) { kx = 0; ++ky; }
  }
  int k = sk;

  auto load_a = [&]() -> uint4 {
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (m_ok && k < K && iy >= 0 && iy < d.h_in && ix >= 0 && ix < d.w_in)
      return *(const uint4*)(img_base + ((size_t)iy * d.w_in + ix) * (size_t)d.lda + c);
    return make_uint4(0, 0, 0, 0);
  };
  auto load_b = [&]() -> uint4 {
    if (n_ok && k < K) return *(const uint4*)(w_row + k);
    return make_uint4(0, 0, 0, 0);
  };
  auto advance = [&]() {
    k += BK;
    c += BK;
    while (c >= d.c_in) {
      c -= d.c_in;
      if (++kx == d.kw) { kx = 0; ++ky; }
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int steps = (K + BK - 1) / BK;
  uint4 ra = load_a(), rb = load_b();
  *(uint4*)(smem + sr * LDT + sk) = ra;
  *(uint4*)(smem + (BM + sr) * LDT + sk) = rb;
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;   // block-uniform
    if (more) {
      advance();
      ra = load_a();
      rb = load_b();
    }
    const f16* st = smem + (s & 1) * STAGE;
    const f16* a = st + (wm * 32 + fr) * LDT + fq * 8;
    const f16* b = st + (BM + wn * 32 + fr) * LDT + fq * 8;
    const f16x8 a0 = *(const f16x8*)a, a1 = *(const f16x8*)(a + 16 * LDT);
    const f16x8 b0 = *(const f16x8*)b, b1 = *(const f16x8*)(b + 16 * LDT);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, acc[1][1], 0, 0, 0);
    if (more) {
      f16* nx = smem + ((s + 1) & 1) * STAGE;
      *(uint4*)(nx + sr * LDT + sk) = ra;
      *(uint4*)(nx + (BM + sr) * LDT + sk) = rb;
    }
    __syncthreads();
  }

  // epilogue: C/D element j of the lane is row fq * 4 + j, column fr of its 16 x 16 tile
  f16* so = smem;   // [BM][LDO]; every wave is past the last barrier, so no stage is being read
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = wn * 32 + ni * 16 + fr;
    float bv = 0.0f;
    if ((d.epilogue & RCDM_EPI_BIAS) && n0 + col < d.c_out) bv = bias[n0 + col];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = acc[mi][ni][j] + bv;
        if (d.epilogue & RCDM_EPI_RELU) v = relu_f(v);
        so[(wm * 32 + mi * 16 + fq * 4 + j) * LDO + col] = (f16)v;
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < (BM * BN / 8) / NT; ++i) {
    const int idx = tid + i * NT;
    const int r = idx >> 3, cc = (idx & 7) * 8;
    if (m0 + r < M && n0 + cc < d.c_out)   // c_out % 8 == 0: a piece is inside or outside as a whole
      *(uint4*)(out + (size_t)(m0 + r) * (size_t)d.ldc + n0 + cc) = *(const uint4*)(so + r * LDO + cc);
  }
}

__global__ __launch_bounds__(NT) void pool2d_kernel(rcdm_pool2d_desc d, int h_out, int w_out, size_t total,
                                                    const f16* __restrict__ in, f16* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int chunks = d.c >> 3;
  const size_t p = idx / chunks;
  const int ch = (int)(idx - p * chunks) * 8;
  const size_t hw = (size_t)h_out * w_out;
  const size_t img = p / hw, rem = p - img * hw;
  const int oy = (int)(rem / w_out), ox = (int)(rem - (size_t)oy * w_out);
  const f16* base = in + img * d.h_in * d.w_in * (size_t)d.ld_in + ch;
  const bool is_max = d.mode == RCDM_POOL_MAX;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = is_max ? -__builtin_inff() : 0.0f;
  int count = 0;
  for (int ky = 0; ky < d.kh; ++ky) {
    const int iy = oy * d.stride_h - d.pad_h + ky;
    if (iy < 0 || iy >= d.h_in) continue;
    for (int kx = 0; kx < d.kw; ++kx) {
      const int ix = ox * d.stride_w - d.pad_w + kx;
      if (ix < 0 || ix >= d.w_in) continue;
      Pack16 x;
      x.u = *(const uint4*)(base + ((size_t)iy * d.w_in + ix) * (size_t)d.ld_in);
      ++count;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = (float)x.e[e];
        if (is_max) v[e] = (f > v[e] || f != f) ? f : v[e];   // a NaN in the window is the result
        else v[e] = v[e] + f;
      }
    }
  }
  Pack16 o;
  if (is_max) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = (f16)v[e];
  } else {
    const float div = d.mode == RCDM_POOL_AVG_INCLUDE_PAD ? (float)(d.kh * d.kw) : (float)count;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = (f16)(v[e] / div);
  }
  *(uint4*)(out + p * (size_t)d.ld_out + ch) = o.u;
}

__global__ __launch_bounds__(NT) void global_avgpool_kernel(int n_img, int rows, int c, const f16* __restrict__ in, int64_t ld,
                                                            float* __restrict__ out, int64_t ldo) {
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  const int chunks = c >> 3;
  if (idx >= (size_t)n_img * chunks) return;
  const size_t img = idx / chunks;
  const int ch = (int)(idx - img * chunks) * 8;
  const f16* p = in + img * rows * (size_t)ld + ch;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.0f;
  for (int r = 0; r < rows; ++r) {
    Pack16 x;
    x.u = *(const uint4*)(p + (size_t)r * (size_t)ld);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = s[e] + (float)x.e[e];
  }
  const float div = (float)rows;
  float* o = out + img * (size_t)ldo + ch;
  *(f32x4*)o = f32x4{s[0] / div, s[1] / div, s[2] / div, s[3] / div};
  *(f32x4*)(o + 4) = f32x4{s[4] / div, s[5] / div, s[6] / div, s[7] / div};
}

// torch's area_pixel_compute_source_index (align_corners = False, not cubic): scale * (o + 0.5) - 0.5 as ONE fused
// multiply-add (what torch's CPU build evaluates: a product rounded on its own moves s by an ulp, 4e-6 at s = 48), negatives to 0
__device__ __forceinline__ void bilinear_axis(int o, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float s = __builtin_fmaf(scale, (float)o + 0.5f, -0.5f);
  if (s < 0.0f) s = 0.0f;
  i0 = min((int)s, in_size - 1);
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.0f - l1;
}

__global__ __launch_bounds__(NT) void bilinear_rows_kernel(rcdm_bilinear_desc d, const uint8_t* __restrict__ src,
                                                           f16* __restrict__ dst) {
#pragma clang fp contract(off)
  const size_t hw = (size_t)d.out_h * d.out_w;
  const size_t p = (size_t)blockIdx.x * NT + threadIdx.x;
  if (p >= hw * d.n) return;
  const size_t img = p / hw, rem = p - img * hw;
  const int oy = (int)(rem / d.out_w), ox = (int)(rem - (size_t)oy * d.out_w);
  int y0, y1, x0, x1;
  float wy0, wy1, wx0, wx1;
  bilinear_axis(oy, (float)d.in_h / (float)d.out_h, d.in_h, y0, y1, wy0, wy1);
  bilinear_axis(ox, (float)d.in_w / (float)d.out_w, d.in_w, x0, x1, wx0, wx1);
  const uint8_t* s = src + img * (size_t)d.src_stride;
  const uint8_t* r0 = s + (size_t)y0 * (size_t)d.src_pitch;
  const uint8_t* r1 = s + (size_t)y1 * (size_t)d.src_pitch;
  Pack16 v;
  v.u = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int sc = d.flip_channels ? 2 - ch : ch;
    const float v00 = (float)r0[3 * x0 + sc] / 255.0f, v01 = (float)r0[3 * x1 + sc] / 255.0f;
    const float v10 = (float)r1[3 * x0 + sc] / 255.0f, v11 = (float)r1[3 * x1 + sc] / 255.0f;
    const float top = wx0 * v00 + wx1 * v01, bot = wx0 * v10 + wx1 * v11;
    float t = wy0 * top + wy1 * bot;
    t = t * d.scale[ch];
    t = t + d.shift[ch];
    v.e[ch] = (f16)t;
  }
  uint4* row = (uint4*)(dst + p * (size_t)d.ld);
  row[0] = v.u;
  for (int j = 1; j < d.c_pad / 8; ++j) row[j] = make_uint4(0, 0, 0, 0);
}

int out_side(int in, int pad, int k, int stride) {
  const int span = in + 2 * pad - k;
  return span < 0 ? 0 : span / stride + 1;
}

// RCDM_OK and the output sides, or the status to return
int conv2d_check(const rcdm_conv2d_desc* d, int& h_out, int& w_out) {
  if (d->n_img <= 0 || d->h_in <= 0 || d->w_in <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->pad_h < 0 || d->pad_w < 0 || d->lda < d->c_in || d->ldc < d->c_out)
    return RCDM_EINVAL;
  if ((d->c_in & 7) || (d->c_out & 7) || (d->lda & 7) || (d->ldc & 7)) return RCDM_ESHAPE;
  if (d->kh > MAX_K || d->kw > MAX_K || d->pad_h >= d->kh || d->pad_w >= d->kw) return RCDM_ESHAPE;
  if ((d->stride_h != 1 && d->stride_h != 2) || (d->stride_w != 1 && d->stride_w != 2)) return RCDM_ESHAPE;
  if (d->epilogue & ~(RCDM_EPI_BIAS | RCDM_EPI_RELU)) return RCDM_ESHAPE;
  if (d->h_in > MAX_SIDE || d->w_in > MAX_SIDE) return RCDM_ESHAPE;
  h_out = out_side(d->h_in, d->pad_h, d->kh, d->stride_h);
  w_out = out_side(d->w_in, d->pad_w, d->kw, d->stride_w);
  if (h_out < 1 || w_out < 1) return RCDM_ESHAPE;
  // (row indices are 32-bit, a tile may reach BM - 1 rows past M; the offsets built from them are 64-bit)
  if ((int64_t)d->n_img * h_out * w_out > 0x7fffffff - BM || (int64_t)d->kh * d->kw * d->c_in > 0x7fffffff - BK) return RCDM_ESHAPE;
  return RCDM_OK;
}

int pool2d_check(const rcdm_pool2d_desc* d, int& h_out, int& w_out) {
  if (d->n_img <= 0 || d->h_in <= 0 || d->w_in <= 0 || d->c <= 0 || d->kh <= 0 || d->kw <= 0 || d->pad_h < 0 ||
      d->pad_w < 0 || d->ld_in < d->c || d->ld_out < d->c)
    return RCDM_EINVAL;
  if (d->mode != RCDM_POOL_MAX && d->mode != RCDM_POOL_AVG_INCLUDE_PAD && d->mode != RCDM_POOL_AVG_EXCLUDE_PAD) return RCDM_EINVAL;
  if ((d->c & 7) || (d->ld_in & 7) || (d->ld_out & 7)) return RCDM_ESHAPE;
  // pad <= k / 2 (torch's rule): every window then holds at least one in-image tap
  if (d->kh > 3 || d->kw > 3 || 2 * d->pad_h > d->kh || 2 * d->pad_w > d->kw) return RCDM_ESHAPE;
  if ((d->stride_h != 1 && d->stride_h != 2) || (d->stride_w != 1 && d->stride_w != 2)) return RCDM_ESHAPE;
  if (d->h_in > MAX_SIDE || d->w_in > MAX_SIDE) return RCDM_ESHAPE;
  h_out = out_side(d->h_in, d->pad_h, d->kh, d->stride_h);
  w_out = out_side(d->w_in, d->pad_w, d->kw, d->stride_w);
  if (h_out < 1 || w_out < 1) return RCDM_ESHAPE;
  return RCDM_OK;
}

}  // namespace

extern "C" {

int rcdm_conv2d(const rcdm_conv2d_desc* d, const void* in, const void* W, const float* bias, void* out, void* stream) {
  if (!d || !in || !W || !out) return RCDM_EINVAL;
  int h_out = 0, w_out = 0;
  const int rc = conv2d_check(d, h_out, w_out);
  if (rc != RCDM_OK) return rc;
  if ((d->epilogue & RCDM_EPI_BIAS) && !bias) return RCDM_EINVAL;
  if ((((uintptr_t)in | (uintptr_t)W | (uintptr_t)out) & 15) || ((uintptr_t)bias & 3)) return RCDM_EINVAL;
  const int M = d->n_img * h_out * w_out, K = d->kh * d->kw * d->c_in;
  const unsigned tiles_n = (unsigned)((d->c_out + BN - 1) / BN);
  if (tiles_n > 65535u) return RCDM_ESHAPE;
  const dim3 grid((unsigned)((M + BM - 1) / BM), tiles_n);
  hipLaunchKernelGGL(conv2d_kernel, grid, dim3(NT), 0, (hipStream_t)stream, *d, h_out, w_out, M, K, (const f16*)in,
                     (const f16*)W, bias, (f16*)out);
  return rcdm_check_launch();
}

int rcdm_pool2d(const rcdm_pool2d_desc* d, const void* in, void* out, void* stream) {
  if (!d || !in || !out) return RCDM_EINVAL;
  int h_out = 0, w_out = 0;
  const int rc = pool2d_check(d, h_out, w_out);
  if (rc != RCDM_OK) return rc;
  if (((uintptr_t)in | (uintptr_t)out) & 15) return RCDM_EINVAL;
  const size_t total = (size_t)d->n_img * h_out * w_out * (size_t)(d->c >> 3);
  const size_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffffu) return RCDM_ESHAPE;
  hipLaunchKernelGGL(pool2d_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *d, h_out, w_out, total,
                     (const f16*)in, (f16*)out);
  return rcdm_check_launch();
}

int rcdm_global_avgpool(int32_t n_img, int32_t rows_per_img, int32_t c, const void* in, int64_t ld, float* out_f32, int64_t ldo,
                        void* stream) {
  if (!in || !out_f32) return RCDM_EINVAL;
  if (n_img <= 0 || rows_per_img <= 0 || c <= 0 || ld < c || ldo < c) return RCDM_EINVAL;
  if ((c & 7) || (ld & 7) || (ldo & 3)) return RCDM_ESHAPE;
  if (((uintptr_t)in | (uintptr_t)out_f32) & 15) return RCDM_EINVAL;
  const size_t total = (size_t)n_img * (size_t)(c >> 3);
  const size_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffffu) return RCDM_ESHAPE;
  hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, n_img, rows_per_img, c,
                     (const f16*)in, ld, out_f32, ldo);
  return rcdm_check_launch();
}

int rcdm_image_bilinear_rows(const rcdm_bilinear_desc* d, const void* src_u8, void* dst, void* stream) {
  if (!d || !src_u8 || !dst) return RCDM_EINVAL;
  if (d->n <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->out_h <= 0 || d->out_w <= 0) return RCDM_EINVAL;
  if (d->src_pitch < 3 * (int64_t)d->in_w || d->src_stride < 0) return RCDM_EINVAL;
  if (d->c_pad < 8 || (d->c_pad & 7) || (d->ld & 7) || d->ld < d->c_pad || ((uintptr_t)dst & 15)) return RCDM_EINVAL;
  for (int ch = 0; ch < 3; ++ch)
    if (!(d->scale[ch] == d->scale[ch]) || !(d->shift[ch] == d->shift[ch])) return RCDM_EINVAL;
  if (d->channels != 3 || d->in_h > MAX_SIDE || d->in_w > MAX_SIDE || d->out_h > MAX_SIDE || d->out_w > MAX_SIDE) return RCDM_ESHAPE;
  const size_t total = (size_t)d->n * d->out_h * d->out_w;
  const size_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffffu) return RCDM_ESHAPE;
  hipLaunchKernelGGL(bilinear_rows_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, *d, (const uint8_t*)src_u8,
                     (f16*)dst);
  return rcdm_check_launch();
}

}  // extern "C"
