// guide.hip — guidance rescale (Lin et al. 2023 §3.4; diffusers `rescale_noise_cfg`) for the captured step: the per-story
// factor  k_s = phi * std(e_c) / std(e) + (1 - phi),  e = e_u + g (e_c - e_u),  over the 4 f H W elements of story s,
// from the f16 eps rows the UNet leaves behind.  The step kernels of misc.hip multiply e by k_s (rcdm_cfg_*_step_scaled).
//
// Replaces (reference): the `guidance_rescale` argument of stage2_batchtest_rcdms_model.py:352.
//
// Two launches, no atomics, no counters, bitwise reproducible:
//   1. cfg_rescale_partial_kernel — grid (ceil(f H W / 1024), S): block (b, s) walks rows [1024 b, 1024 b + 1024) of story s
//      in a fixed strided order and stores its four SHIFTED sums  sum(d), sum(d^2)  of the conditional half and of the
//      combined prediction, d = x - (the story's first element): raw sum(x), sum(x^2) loses k at |mean| / std >= 64
//      (the GroupNorm statistics learned the same).  Lanes by xor-shuffle, waves through LDS in wave order.
//   2. cfg_rescale_finalize_kernel — one thread per story adds the story's partials in block order in fp64 and writes k_s.
// Every partial a finalize reads was stored by launch 1 of the same call: nothing depends on the workspace's contents.
#include "common.h"

namespace {

constexpr int GUIDE_ROWS = 1024;   // rows of one story per block of launch 1: 4 rows (32 elements) per thread

__host__ __device__ inline int guide_blocks(size_t fhw) { return (int)((fhw + GUIDE_ROWS - 1) / GUIDE_ROWS); }

template <bool VEC>
__device__ __forceinline__ void load4(const f16* p, float (&v)[4]) {
  if (VEC) {
    const f16x4 u = *(const f16x4*)p;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (float)u[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (float)p[c];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_partial_kernel(const f16* __restrict__ eps, int ld, int S, size_t fhw,
                                                                  float gs, float* __restrict__ part) {
  __shared__ float red[4][4];
  const int s = blockIdx.y, b = blockIdx.x;
  const f16* eu = eps + (size_t)s * fhw * ld;
  const f16* ec = eps + ((size_t)S + s) * fhw * ld;
  // the shifts: channel 0 of the story's first row, the same for every block of the story
  const float u0 = (float)eu[0], c0 = (float)ec[0];
  const float e0 = u0 + gs * (c0 - u0);
  float sc = 0.f, qc = 0.f, se = 0.f, qe = 0.f;
  const size_t r0 = (size_t)b * GUIDE_ROWS;
  const size_t r1 = r0 + GUIDE_ROWS < fhw ? r0 + GUIDE_ROWS : fhw;
  for (size_t r = r0 + threadIdx.x; r < r1; r += 256) {
    float u[4], c[4];
    load4<VEC>(eu + r * ld, u);
    load4<VEC>(ec + r * ld, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = u[k] + gs * (c[k] - u[k]);
      const float dc = c[k] - c0, de = e - e0;
      sc += dc;
      qc = fmaf(dc, dc, qc);
      se += de;
      qe = fmaf(de, de, qe);
    }
  }
  sc = wave_sum(sc);
  qc = wave_sum(qc);
  se = wave_sum(se);
  qe = wave_sum(qe);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = sc;
    red[wave][1] = qc;
    red[wave][2] = se;
    red[wave][3] = qe;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    part[((size_t)s * gridDim.x + b) * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// k = 1 when std(e) == 0 (a constant prediction): diffusers divides and hands on inf / nan, here the step is left as it is.
__global__ void cfg_rescale_finalize_kernel(const float* __restrict__ part, int S, int nb, double n, float phi,
                                            float* __restrict__ factor) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double sc = 0.0, qc = 0.0, se = 0.0, qe = 0.0;
  const float* p = part + (size_t)s * nb * 4;
  for (int b = 0; b < nb; ++b) {
    sc += (double)p[4 * b + 0];
    qc += (double)p[4 * b + 1];
    se += (double)p[4 * b + 2];
    qe += (double)p[4 * b + 3];
  }
  double vc = (qc - sc * sc / n) / (n - 1.0), ve = (qe - se * se / n) / (n - 1.0);
  vc = vc > 0.0 ? vc : 0.0;
  float k = 1.f;
  if (ve > 0.0 || ve != ve) k = (float)((double)phi * sqrt(vc / ve) + (1.0 - (double)phi));
  factor[s] = k;
}

}  // namespace

extern "C" {

size_t rcdm_cfg_rescale_workspace_bytes(int32_t S, int32_t frames, int32_t H, int32_t W) {
  if (S <= 0 || frames <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)S * guide_blocks((size_t)frames * H * W) * 4 * sizeof(float);
}

int rcdm_cfg_rescale_factor(const void* eps, int32_t ld, int32_t S, int32_t frames, int32_t H, int32_t W,
                            float guidance_scale, float guidance_rescale, void* workspace, size_t workspace_bytes,
                            float* factor, void* stream) {
  if (!eps || !workspace || !factor) return RCDM_EINVAL;
  if (S <= 0 || frames <= 0 || H <= 0 || W <= 0 || ld < 4) return RCDM_EINVAL;
  if (((uintptr_t)workspace & 3) || ((uintptr_t)eps & 1)) return RCDM_EINVAL;
  if (S > 65535) return RCDM_ESHAPE;   // gridDim.y
  if (workspace_bytes < rcdm_cfg_rescale_workspace_bytes(S, frames, H, W)) return RCDM_EWORKSPACE;
  const size_t fhw = (size_t)frames * H * W;
  const int nb = guide_blocks(fhw);
  const bool vec = (ld & 3) == 0 && ((uintptr_t)eps & 7) == 0;
  if (vec)
    hipLaunchKernelGGL(cfg_rescale_partial_kernel<true>, dim3(nb, S), dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld,
                       S, fhw, guidance_scale, (float*)workspace);
  else
    hipLaunchKernelGGL(cfg_rescale_partial_kernel<false>, dim3(nb, S), dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld,
                       S, fhw, guidance_scale, (float*)workspace);
  const int rc = rcdm_check_launch();
  if (rc != RCDM_OK) return rc;
  hipLaunchKernelGGL(cfg_rescale_finalize_kernel, dim3((S + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     (const float*)workspace, S, nb, (double)(4 * fhw), guidance_rescale, factor);
  return rcdm_check_launch();
}

}  // extern "C"
