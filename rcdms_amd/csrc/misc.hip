// misc.hip — the small kernels around the UNet body: timestep embedding, tiny-M linears, input
// assembly / layout conversion, fused CFG + DDIM / PNDM / sigma-table updates, weight repacking.
//
// Replaces (reference): diffusers Timesteps/TimestepEmbedding via src/models/unet.py:100-103,383-389;
// ResnetBlock3D.time_emb_proj src/models/resnet.py:191; the per-step torch.cat / chunk / scheduler.step
// sequence of src/pipelines/RCDMs_pipeline.py:482-497; einops "b c f h w -> (b f) c h w" resnet.py:14-16.
#include "common.h"

namespace {

__global__ void timestep_embed_kernel(const float* __restrict__ t, int rows, int dim, float* __restrict__ out) {
  const int half = dim / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * half) return;
  const int r = idx / half, i = idx - r * half;
  // exponent = -ln(10000) * i / (half - freq_shift), freq_shift = 0; flip_sin_to_cos -> [cos | sin]
  const float w = expf(-9.210340371976184f * (float)i / (float)half);
  const float a = t[r] * w;
  out[(size_t)r * dim + i] = cosf(a);
  out[(size_t)r * dim + half + i] = sinf(a);
}

// one wave per output column n; rows <= 8 kept as static-indexed accumulators.  The (optionally SiLU'd) input rows
// are staged once per block in LDS (rows*K floats) and read back as float4, the weight row streams as 16-byte loads.
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ x, int rows, int K,
                                                           const f16* __restrict__ W, const float* __restrict__ bias,
                                                           int N, int silu_in, int silu_out, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sx = (float*)smem;  // [rows][K]
  for (int i = threadIdx.x; i < rows * K; i += 256) {
    float v = x[i];
    if (silu_in) v = silu_f(v);
    sx[i] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < 4; ++j) {  // 16 output columns per block: the staged input is reused 16 times
  const int n = blockIdx.x * 16 + (threadIdx.x >> 6) * 4 + j;
  if (n >= N) return;
  float acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    Pack16 w;
    w.u = *(const uint4*)(W + (size_t)n * K + k);
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wf[e] = (float)w.e[e];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (r < rows) {
        const f32x4 x0 = *(const f32x4*)(sx + r * K + k), x1 = *(const f32x4*)(sx + r * K + k + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[r] = fmaf(x0[e], wf[e], acc[r]);
          acc[r] = fmaf(x1[e], wf[4 + e], acc[r]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    if (r < rows) {
      float v = wave_sum(acc[r]);
      if (lane == 0) {
        if (bias) v += bias[n];
        if (silu_out) v = silu_f(v);
        out[(size_t)r * N + n] = v;
      }
    }
  }
  }
}

// thread per output row (sample', frame, y, x): 9 gathered channels + zero pad.
__global__ void assemble_input_kernel(const float* __restrict__ lat, const float* __restrict__ mask,
                                      const float* __restrict__ masked, int S, int reps, int F, int H, int W, f16* out,
                                      int ld, int c_pad) {
  const size_t hw = (size_t)H * W, fhw = hw * F;
  const size_t total = (size_t)reps * S * fhw;
  const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= total) return;
  const int sp = (int)(m / fhw);
  const size_t rem = m - (size_t)sp * fhw;  // f*hw + y*W + x
  const int s = sp % S;
  f16* o = out + m * ld;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (f16)lat[((size_t)s * 4 + c) * fhw + rem];
  o[4] = (f16)mask[(size_t)sp * fhw + rem];
#pragma unroll
  for (int c = 0; c < 4; ++c) o[5 + c] = (f16)masked[((size_t)sp * 4 + c) * fhw + rem];
  for (int c = 9; c < c_pad; ++c) o[c] = (f16)0.f;
}

__global__ void ncfhw_to_rows_kernel(const float* __restrict__ x, int b, int C, int F, int H, int W, f16* out, int ld,
                                     int c_pad) {
  const size_t hw = (size_t)H * W, fhw = hw * F;
  const size_t total = (size_t)b * fhw;
  const size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= total) return;
  const int s = (int)(m / fhw);
  const size_t rem = m - (size_t)s * fhw;
  f16* o = out + m * ld;
  for (int c = 0; c < C; ++c) o[c] = (f16)x[((size_t)s * C + c) * fhw + rem];
  for (int c = C; c < c_pad; ++c) o[c] = (f16)0.f;
}

__global__ void rows_to_ncfhw_kernel(const f16* __restrict__ rows, int ld, int b, int C, int F, int H, int W,
                                     float* __restrict__ out) {
  const size_t hw = (size_t)H * W, fhw = hw * F;
  const size_t total = (size_t)b * C * fhw;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t rem = idx % fhw;
  const size_t sc = idx / fhw;
  const int c = (int)(sc % C), s = (int)(sc / C);
  out[idx] = (float)rows[((size_t)s * fhw + rem) * ld + c];
}

// thread per latent element (s, c, f, y, x).  SCALED (all three step kernels): the combined prediction of story s is multiplied
// by factor[s] (guidance rescale, guide.hip) before anything else reads it; the unscaled instantiation is the kernel as it was.
template <bool SCALED>
__global__ void cfg_ddim_kernel(const f16* __restrict__ eps, int ld, float* lat, int S, int reps, int F, int H, int W,
                                float gs, const float* __restrict__ coef, const int* __restrict__ step,
                                const float* __restrict__ factor) {
  const size_t hw = (size_t)H * W, fhw = hw * F;
  const size_t total = (size_t)S * 4 * fhw;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t rem = idx % fhw;
  const size_t sc = idx / fhw;
  const int c = (int)(sc & 3), s = (int)(sc >> 2);
  float e = (float)eps[((size_t)s * fhw + rem) * ld + c];
  if (reps == 2) {
    const float ec = (float)eps[((size_t)(S + s) * fhw + rem) * ld + c];
    e = e + gs * (ec - e);
  }
  if (SCALED) e *= factor[s];
  const float* k = coef + (size_t)(*step) * 4;
  const float x = lat[idx];
  const float x0 = (x - k[1] * e) / k[0];
  lat[idx] = k[2] * x0 + k[3] * e;
}

// Classifier-free guidance + one PLMS step of diffusers 0.24.0 PNDMScheduler (skip_prk_steps; step_plms + _get_prev_sample),
// in place on lat; thread per latent element.  Row (*step) of `tab` (rcdms_amd/scheduler.py PNDMScheduler.plms_table):
// (a, b, w_now, w1, w2, w3, slot_now, s1, s2, s3, mode, -):  e' = w_now e + w1 hist[s1] + w2 hist[s2] + w3 hist[s3];
// x' = a x_src + b e' with x_src = the saved first sample in mode 2 (the repeated second call), x otherwise; mode 1 saves x;
// slot_now >= 0 stores e.  hist: fp32 [5][total] — four prediction slots + the saved sample.
template <bool SCALED>
__global__ void cfg_pndm_kernel(const f16* __restrict__ eps, int ld, float* lat, float* __restrict__ hist, int S, int reps, int F,
                                int H, int W, float gs, const float* __restrict__ tab, const int* __restrict__ step,
                                const float* __restrict__ factor) {
  const size_t hw = (size_t)H * W, fhw = hw * F;
  const size_t total = (size_t)S * 4 * fhw;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t rem = idx % fhw;
  const size_t sc = idx / fhw;
  const int c = (int)(sc & 3), s = (int)(sc >> 2);
  float e = (float)eps[((size_t)s * fhw + rem) * ld + c];
  if (reps == 2) {
    const float ec = (float)eps[((size_t)(S + s) * fhw + rem) * ld + c];
    e = e + gs * (ec - e);
  }
  if (SCALED) e *= factor[s];
  const float* k = tab + (size_t)(*step) * 12;
  const int slot = (int)k[6], mode = (int)k[10];
  float mo = k[2] * e;
  if (k[3] != 0.f) mo += k[3] * hist[(size_t)(int)k[7] * total + idx];
  if (k[4] != 0.f) mo += k[4] * hist[(size_t)(int)k[8] * total + idx];
  if (k[5] != 0.f) mo += k[5] * hist[(size_t)(int)k[9] * total + idx];
  float x = lat[idx];
  if (mode == 1) hist[4 * total + idx] = x;
  if (mode == 2) x = hist[4 * total + idx];
  if (slot >= 0) hist[(size_t)slot * total + idx] = e;
  lat[idx] = k[0] * x + k[1] * mo;
}

// Classifier-free guidance + one step of the table-driven sigma-space / DPM-Solver update (rcdms_amd/scheduler.py
// EulerDiscrete / EulerAncestralDiscrete / LMSDiscrete / DPMSolverMultistep .sigma_table(); row layout in rcdm.h).
// Thread per spatial position (s, f, y, x): its 4 contiguous channels of each eps row are read once (one 8-byte load
// when VEC), the CFG combine is done once, then the 4 channel planes of latents / history / noise / model_in are walked
// (consecutive threads -> consecutive addresses in every plane).  A history slot is read only under a non-zero weight
// and a noise row only under a non-zero c, so neither needs initialisation; slot indices outside 0..2 are ignored.
template <bool VEC, bool SCALED>
__global__ __launch_bounds__(256) void cfg_sigma_kernel(const f16* __restrict__ eps, int ld, float* __restrict__ lat,
                                                        float* __restrict__ model_in, float* __restrict__ hist,
                                                        const float* __restrict__ noise, int S, int reps, size_t fhw,
                                                        float gs, const float* __restrict__ tab,
                                                        const int* __restrict__ step, const float* __restrict__ factor) {
  const size_t total = (size_t)S * 4 * fhw;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)S * fhw) return;
  const int s = (int)(p / fhw);
  const size_t rem = p - (size_t)s * fhw;
  float e[4];
  const f16* eu = eps + p * ld;
  if (VEC) {
    const f16x4 u = *(const f16x4*)eu;
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = (float)u[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = (float)eu[c];
  }
  if (reps == 2) {
    const f16* ec = eps + ((size_t)S * fhw + p) * ld;
    float v[4];
    if (VEC) {
      const f16x4 u = *(const f16x4*)ec;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = (float)u[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = (float)ec[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = e[c] + gs * (v[c] - e[c]);
  }
  if (SCALED) {
    const float fs = factor[s];
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] *= fs;
  }
  const int st = *step;
  const float* k = tab + (size_t)st * 16;
  const float px = k[0], pe = k[1], a = k[2], b = k[3], w1 = k[4], w2 = k[5], w3 = k[6], cn = k[7], cin = k[8];
  const int slot = (int)k[9], s1 = (int)k[10], s2 = (int)k[11], s3 = (int)k[12];
  const bool r1 = w1 != 0.f && s1 >= 0 && s1 < 3, r2 = w2 != 0.f && s2 >= 0 && s2 < 3, r3 = w3 != 0.f && s3 >= 0 && s3 < 3;
  const bool rn = cn != 0.f && noise != nullptr, wr = slot >= 0 && slot < 3;
  const float* nz = rn ? noise + (size_t)st * total : noise;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const size_t idx = ((size_t)s * 4 + c) * fhw + rem;
    const float x = lat[idx];
    const float d = px * x + pe * e[c];
    float y = a * x + b * d;
    if (r1) y += w1 * hist[(size_t)s1 * total + idx];
    if (r2) y += w2 * hist[(size_t)s2 * total + idx];
    if (r3) y += w3 * hist[(size_t)s3 * total + idx];
    if (rn) y += cn * nz[idx];
    if (wr) hist[(size_t)slot * total + idx] = d;
    lat[idx] = y;
    model_in[idx] = cin * y;
  }
}

// Stage-1 prior, per-step sequence assembly.  tok rows (b, l) <- the step-independent rows of `base`, except row
// l == time_row of every sample, which takes the time embedding (one fp32 row, shared by the batch); x16 rows <-
// the noisy embeddings in f16, sample b reading latent row b % n_lat (classifier-free guidance feeds the same 5
// latents to both halves: torch.cat([latents] * 2), prior_pipeline.py:314).
__global__ void prior_assemble_kernel(const f16* __restrict__ base, const float* __restrict__ temb,
                                      const float* __restrict__ lat, int n_lat, f16* __restrict__ tok,
                                      f16* __restrict__ x16, int B, int L, int C, int E, int time_row) {
  const size_t chunks = (size_t)B * L * (C / 8);
  const size_t nx = (size_t)B * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks + nx; i += (size_t)gridDim.x * blockDim.x) {
    if (i < chunks) {
      const int c8 = (int)(i % (C / 8));
      const size_t row = i / (C / 8);
      const int l = (int)(row % L);
      Pack16 v;
      if (l == time_row) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v.e[e] = (f16)temb[c8 * 8 + e];
      } else {
        v.u = *(const uint4*)(base + row * C + c8 * 8);
      }
      *(uint4*)(tok + row * C + c8 * 8) = v.u;
    } else {
      const size_t j = i - chunks;
      const int b = (int)(j / E), e = (int)(j - (size_t)b * E);
      x16[j] = (f16)lat[(size_t)(b % n_lat) * E + e];
    }
  }
}

// CLIP text embeddings (transformers CLIPTextEmbeddings.forward): row r <- f16(token_embedding[ids[r]] + position_embedding[r % L]),
// one 16-byte store per thread.  The ids are trusted (the caller range-checks them on the host).
__global__ void embed_tokens_kernel(const int* __restrict__ ids, int n_rows, int L, const float* __restrict__ table,
                                    const float* __restrict__ pos, int C, f16* __restrict__ out, int ldo) {
  const int cpr = C / 8;
  const size_t chunks = (size_t)n_rows * cpr;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % cpr);
    const size_t r = i / cpr;
    const float* t = table + (size_t)ids[r] * C + c8 * 8;
    const float* q = pos + (size_t)(r % L) * C + c8 * 8;
    const f32x4 t0 = *(const f32x4*)t, t1 = *(const f32x4*)(t + 4), q0 = *(const f32x4*)q, q1 = *(const f32x4*)(q + 4);
    Pack16 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v.e[e] = (f16)(t0[e] + q0[e]);
      v.e[4 + e] = (f16)(t1[e] + q1[e]);
    }
    *(uint4*)(out + r * ldo + c8 * 8) = v.u;
  }
}

// CLIP vision patch embedding as GEMM rows (transformers CLIPVisionEmbeddings.forward: Conv2d(3, C, patch, stride patch,
// bias=False) then the class token in front): image b gives Ph Pw + 1 rows of ldk halfs — row 0 all zero (the class-token slot:
// the GEMM leaves its residual operand there), row 1 + p the pixels of patch p in the weight's (c, ky, kx) order, columns
// 3 patch^2 .. ldk zero.
__global__ void patch_rows_kernel(const float* __restrict__ px, int B, int H, int W, int patch, f16* __restrict__ out, int ldk) {
  const int Pw = W / patch, T = (H / patch) * Pw + 1, cpr = ldk / 8, pp = patch * patch, K = 3 * pp;
  const size_t chunks = (size_t)B * T * cpr;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
    const int c8 = (int)(i % cpr);
    const size_t row = i / cpr;
    const int b = (int)(row / T), j = (int)(row % T);
    Pack16 v;
    v.u = make_uint4(0, 0, 0, 0);
    if (j > 0) {
      const int py = (j - 1) / Pw, pxx = (j - 1) % Pw;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = c8 * 8 + e;
        if (col < K) {
          const int c = col / pp, k = col - c * pp, ky = k / patch, kx = k - ky * patch;
          v.e[e] = (f16)px[(((size_t)b * 3 + c) * H + py * patch + ky) * W + pxx * patch + kx];
        }
      }
    }
    *(uint4*)(out + row * ldk + c8 * 8) = v.u;
  }
}

// Stage-1 prior, CFG combine + UnCLIPScheduler.step (prediction_type "sample", variance_type "fixed_small_log"),
// prior_pipeline.py:328-344 + diffusers 0.24.0 UnCLIPScheduler.step: x0 = clamp(u + s (c - u), +-clip);
// lat = k0 x0 + k1 lat + k2 noise, with (k0, k1, k2) = coef[*step] (k2 = 0 on the last step).
__global__ void cfg_unclip_kernel(const f16* __restrict__ pred, int ld, float* lat, int n, int reps, int E, float gs,
                                  float clip, const float* __restrict__ coef, const float* __restrict__ noise,
                                  const int* __restrict__ step) {
  const size_t total = (size_t)n * E;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int r = (int)(idx / E), e = (int)(idx - (size_t)r * E);
  float x0 = (float)pred[(size_t)r * ld + e];
  if (reps == 2) {
    const float xc = (float)pred[(size_t)(n + r) * ld + e];
    x0 = x0 + gs * (xc - x0);
  }
  if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
  const int st = *step;
  const float* k = coef + (size_t)st * 3;
  float v = k[0] * x0 + k[1] * lat[idx];
  if (noise) v += k[2] * noise[(size_t)st * total + idx];
  lat[idx] = v;
}

__global__ void load_timestep_kernel(const float* __restrict__ ts, const int* __restrict__ step, float* t_out, int rows) {
  const int i = threadIdx.x;
  if (i < rows) t_out[i] = ts[*step];
}
__global__ void load_table_row_kernel(const float* __restrict__ table, const int* __restrict__ step, float* __restrict__ dst,
                                      size_t row_floats) {
  const f32x4* src = (const f32x4*)(table + (size_t)(*step) * row_floats);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < row_floats / 4; i += (size_t)gridDim.x * blockDim.x)
    ((f32x4*)dst)[i] = src[i];
}
__global__ void advance_step_kernel(int* step) {
  if (threadIdx.x == 0) *step = *step + 1;
}

__global__ void pack_f16_kernel(const float* __restrict__ src, f16* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = (f16)src[i];
}
// Mish (reference resnet.py:215-217): x * tanh(softplus(x)), fp32 elementwise; softplus with torch's threshold of 20
__global__ void mish_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    const float sp = v > 20.f ? v : log1pf(__expf(v));
    y[i] = v * tanhf(sp);
  }
}
// dst[co][tap*cin_pad + ci] = w[co][ci][ky][kx], tap = ky*3+kx
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, int c_out, int c_in, int cin_pad, f16* __restrict__ dst) {
  const size_t total = (size_t)c_out * 9 * cin_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin_pad);
    const size_t r = i / cin_pad;
    const int tap = (int)(r % 9), co = (int)(r / 9);
    dst[i] = ci < c_in ? (f16)w[((size_t)co * c_in + ci) * 9 + tap] : (f16)0.f;
  }
}
// phase weights of nearest-2x upsample + conv3x3 (rcdm_conv3x3, upsample = 2): dst[phase][co][tap2 * c_in + ci], phase = 2a + b,
// tap2 = 2r + c = the 2x2 source pixel (y + a - 1 + r, x + b - 1 + c) of output pixel (2y + a, 2x + b); its weight is the
// fp32 SUM of the 3x3 taps (ky, kx) with (a + ky - 1) >> 1 == a - 1 + r and (b + kx - 1) >> 1 == b - 1 + c:
// a = 0: r = 0 <- {ky 0}, r = 1 <- {1, 2};   a = 1: r = 0 <- {0, 1}, r = 1 <- {2}   (same for columns)
__global__ void pack_conv3x3_up2_kernel(const float* __restrict__ w, int c_out, int c_in, f16* __restrict__ dst) {
  const size_t total = (size_t)4 * c_out * 4 * c_in;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % c_in);
    size_t q = i / c_in;
    const int tap2 = (int)(q & 3);
    q >>= 2;
    const int co = (int)(q % c_out), phase = (int)(q / c_out);
    const int a = phase >> 1, b = phase & 1, r = tap2 >> 1, c = tap2 & 1;
    const float* src = w + ((size_t)co * c_in + ci) * 9;
    float acc = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
      if (((a + ky + 1) >> 1) - 1 != a - 1 + r) continue;   // ((a + ky - 1) >> 1 with the argument kept non-negative)
      for (int kx = 0; kx < 3; ++kx)
        if (((b + kx + 1) >> 1) - 1 == b - 1 + c) acc += src[ky * 3 + kx];
    }
    dst[i] = (f16)acc;
  }
}
// C[n][m] = A[n][k] B[k][m], all fp32 row-major: weight COMPOSITION at pack time (two linear maps in a row folded into one
// matrix before it is rounded to f16 — Packer.ffz, the context stacks); 32x32 tiles through LDS, fixed summation order.
// Not a hot-path kernel: a few GFLOP once per model load.
__global__ __launch_bounds__(256) void matmul_f32_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                         float* __restrict__ C, int n, int k, int m) {
  __shared__ float sa[32][33], sb[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads, 4 output rows each
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < k; k0 += 32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = ty + 8 * i;
      sa[r][tx] = (r0 + r < n && k0 + tx < k) ? A[(size_t)(r0 + r) * k + k0 + tx] : 0.f;
      sb[r][tx] = (k0 + r < k && c0 + tx < m) ? B[(size_t)(k0 + r) * m + c0 + tx] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < 32; ++kk) {
      const float b = sb[kk][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(sa[ty + 8 * i][kk], b, acc[i]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (r0 + ty + 8 * i < n && c0 + tx < m) C[(size_t)(r0 + ty + 8 * i) * m + c0 + tx] = acc[i];
}
// packed row p: grp = p/32, j = p%32; source row = j<16 ? grp*16+j (hidden) : n_out/2 + grp*16 + (j-16) (gate)
__global__ void pack_geglu_kernel(const float* __restrict__ w, const float* __restrict__ bias, int n_out, int K,
                                  f16* __restrict__ wd, float* __restrict__ bd) {
  const size_t total = (size_t)n_out * K;
  const int half = n_out / 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K), prow = (int)(i / K);
    const int grp = prow >> 5, j = prow & 31;
    const int src = j < 16 ? grp * 16 + j : half + grp * 16 + (j - 16);
    wd[i] = (f16)w[(size_t)src * K + k];
    if (k == 0 && bias && bd) bd[prow] = bias[src];
  }
}

inline int grid_for(size_t n, int block = 256, int cap = 8192) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" {

int rcdm_timestep_embed(const float* t, int32_t rows, int32_t dim, float* out, void* stream) {
  if (!t || !out || rows <= 0 || dim <= 0 || (dim & 1)) return RCDM_EINVAL;
  const int n = rows * (dim / 2);
  hipLaunchKernelGGL(timestep_embed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, rows, dim, out);
  return rcdm_check_launch();
}

int rcdm_small_linear(const float* x, int32_t rows, int32_t K, const void* W, const float* bias, int32_t N,
                      int32_t silu_in, int32_t silu_out, float* out, void* stream) {
  if (!x || !W || !out || rows <= 0 || K <= 0 || N <= 0) return RCDM_EINVAL;
  if (rows > 8 || (K & 7) || (size_t)rows * K * sizeof(float) > 64 * 1024) return RCDM_ESHAPE;
  hipLaunchKernelGGL(small_linear_kernel, dim3((N + 15) / 16), dim3(256), (size_t)rows * K * sizeof(float),
                     (hipStream_t)stream, x, rows, K,
                     (const f16*)W, bias, N, silu_in, silu_out, out);
  return rcdm_check_launch();
}

int rcdm_assemble_input(const float* latents, const float* mask, const float* masked, int32_t S, int32_t reps,
                        int32_t frames, int32_t H, int32_t W, void* out, int32_t ld, int32_t c_pad, void* stream) {
  if (!latents || !mask || !masked || !out) return RCDM_EINVAL;
  if (S <= 0 || (reps != 1 && reps != 2) || frames <= 0 || H <= 0 || W <= 0 || c_pad < 9 || ld < c_pad) return RCDM_EINVAL;
  const size_t total = (size_t)reps * S * frames * H * W;
  hipLaunchKernelGGL(assemble_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     latents, mask, masked, S, reps, frames, H, W, (f16*)out, ld, c_pad);
  return rcdm_check_launch();
}

int rcdm_ncfhw_to_rows(const float* x, int32_t b, int32_t C, int32_t frames, int32_t H, int32_t W, void* out, int32_t ld,
                       int32_t c_pad, void* stream) {
  if (!x || !out || b <= 0 || C <= 0 || frames <= 0 || H <= 0 || W <= 0 || c_pad < C || ld < c_pad) return RCDM_EINVAL;
  const size_t total = (size_t)b * frames * H * W;
  hipLaunchKernelGGL(ncfhw_to_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     b, C, frames, H, W, (f16*)out, ld, c_pad);
  return rcdm_check_launch();
}

int rcdm_rows_to_ncfhw(const void* rows, int32_t ld, int32_t b, int32_t C, int32_t frames, int32_t H, int32_t W,
                       float* out, void* stream) {
  if (!rows || !out || b <= 0 || C <= 0 || frames <= 0 || H <= 0 || W <= 0 || ld < C) return RCDM_EINVAL;
  const size_t total = (size_t)b * C * frames * H * W;
  hipLaunchKernelGGL(rows_to_ncfhw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f16*)rows, ld, b, C, frames, H, W, out);
  return rcdm_check_launch();
}

int rcdm_cfg_ddim_step_scaled(const void* eps, int32_t ld, float* latents, int32_t S, int32_t reps, int32_t frames, int32_t H,
                              int32_t W, float guidance_scale, const float* coef, const int32_t* step_counter,
                              const float* factor, void* stream) {
  if (!eps || !latents || !coef || !step_counter) return RCDM_EINVAL;
  if (S <= 0 || (reps != 1 && reps != 2) || frames <= 0 || H <= 0 || W <= 0 || ld < 4) return RCDM_EINVAL;
  const size_t total = (size_t)S * 4 * frames * H * W;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (factor)
    hipLaunchKernelGGL(cfg_ddim_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld, latents, S, reps,
                       frames, H, W, guidance_scale, coef, step_counter, factor);
  else
    hipLaunchKernelGGL(cfg_ddim_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld, latents, S, reps,
                       frames, H, W, guidance_scale, coef, step_counter, factor);
  return rcdm_check_launch();
}

int rcdm_cfg_ddim_step(const void* eps, int32_t ld, float* latents, int32_t S, int32_t reps, int32_t frames, int32_t H,
                       int32_t W, float guidance_scale, const float* coef, const int32_t* step_counter, void* stream) {
  return rcdm_cfg_ddim_step_scaled(eps, ld, latents, S, reps, frames, H, W, guidance_scale, coef, step_counter, nullptr, stream);
}

int rcdm_cfg_pndm_step_scaled(const void* eps, int32_t ld, float* latents, float* history, int32_t S, int32_t reps,
                              int32_t frames, int32_t H, int32_t W, float guidance_scale, const float* table,
                              const int32_t* step_counter, const float* factor, void* stream) {
  if (!eps || !latents || !history || !table || !step_counter) return RCDM_EINVAL;
  if (S <= 0 || (reps != 1 && reps != 2) || frames <= 0 || H <= 0 || W <= 0 || ld < 4) return RCDM_EINVAL;
  const size_t total = (size_t)S * 4 * frames * H * W;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (factor)
    hipLaunchKernelGGL(cfg_pndm_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld, latents, history, S,
                       reps, frames, H, W, guidance_scale, table, step_counter, factor);
  else
    hipLaunchKernelGGL(cfg_pndm_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld, latents, history, S,
                       reps, frames, H, W, guidance_scale, table, step_counter, factor);
  return rcdm_check_launch();
}

int rcdm_cfg_pndm_step(const void* eps, int32_t ld, float* latents, float* history, int32_t S, int32_t reps, int32_t frames,
                       int32_t H, int32_t W, float guidance_scale, const float* table, const int32_t* step_counter, void* stream) {
  return rcdm_cfg_pndm_step_scaled(eps, ld, latents, history, S, reps, frames, H, W, guidance_scale, table, step_counter,
                                   nullptr, stream);
}

int rcdm_cfg_sigma_step_scaled(const void* eps, int32_t ld, float* latents, float* model_in, float* history, const float* noise,
                               int32_t S, int32_t reps, int32_t frames, int32_t H, int32_t W, float guidance_scale,
                               const float* table, const int32_t* step_counter, const float* factor, void* stream) {
  if (!eps || !latents || !model_in || !history || !table || !step_counter) return RCDM_EINVAL;
  if (S <= 0 || (reps != 1 && reps != 2) || frames <= 0 || H <= 0 || W <= 0 || ld < 4) return RCDM_EINVAL;
  const size_t fhw = (size_t)frames * H * W;
  const size_t n = (size_t)S * fhw;
  const bool vec = (ld & 3) == 0 && ((uintptr_t)eps & 7) == 0;
  auto kernel = vec ? (factor ? cfg_sigma_kernel<true, true> : cfg_sigma_kernel<true, false>)
                    : (factor ? cfg_sigma_kernel<false, true> : cfg_sigma_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const f16*)eps, ld, latents,
                     model_in, history, noise, S, reps, fhw, guidance_scale, table, step_counter, factor);
  return rcdm_check_launch();
}

int rcdm_cfg_sigma_step(const void* eps, int32_t ld, float* latents, float* model_in, float* history, const float* noise,
                        int32_t S, int32_t reps, int32_t frames, int32_t H, int32_t W, float guidance_scale,
                        const float* table, const int32_t* step_counter, void* stream) {
  return rcdm_cfg_sigma_step_scaled(eps, ld, latents, model_in, history, noise, S, reps, frames, H, W, guidance_scale, table,
                                    step_counter, nullptr, stream);
}

int rcdm_prior_assemble(const void* base, const float* temb, const float* latents, int32_t n_lat, void* tok, void* x16,
                        int32_t B, int32_t L, int32_t C, int32_t E, int32_t time_row, void* stream) {
  if (!base || !temb || !latents || !tok || !x16) return RCDM_EINVAL;
  if (B <= 0 || L <= 0 || C <= 0 || E <= 0 || n_lat <= 0 || time_row < 0 || time_row >= L) return RCDM_EINVAL;
  if (C & 7) return RCDM_ESHAPE;
  const size_t n = (size_t)B * L * (C / 8) + (size_t)B * E;
  hipLaunchKernelGGL(prior_assemble_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const f16*)base, temb,
                     latents, n_lat, (f16*)tok, (f16*)x16, B, L, C, E, time_row);
  return rcdm_check_launch();
}

int rcdm_embed_tokens(const int32_t* ids, int32_t n_rows, int32_t L, const float* table, int32_t vocab, const float* pos,
                      int32_t C, void* out, int32_t ldo, void* stream) {
  if (!ids || !table || !pos || !out) return RCDM_EINVAL;
  if (n_rows <= 0 || L <= 0 || vocab <= 0 || C <= 0) return RCDM_EINVAL;
  if ((C & 7) || (ldo & 7) || ldo < C) return RCDM_ESHAPE;
  const size_t n = (size_t)n_rows * (C / 8);
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, ids, n_rows, L, table, pos, C,
                     (f16*)out, ldo);
  return rcdm_check_launch();
}

int rcdm_patch_rows(const float* pixels, int32_t B, int32_t H, int32_t W, int32_t patch, void* out, int32_t ldk, void* stream) {
  if (!pixels || !out || B <= 0 || H <= 0 || W <= 0 || patch <= 0) return RCDM_EINVAL;
  if ((H % patch) || (W % patch) || (ldk & 7) || ldk < 3 * patch * patch) return RCDM_ESHAPE;
  const size_t n = (size_t)B * ((H / patch) * (W / patch) + 1) * (ldk / 8);
  hipLaunchKernelGGL(patch_rows_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, pixels, B, H, W, patch, (f16*)out,
                     ldk);
  return rcdm_check_launch();
}

int rcdm_cfg_unclip_step(const void* pred, int32_t ld, float* latents, int32_t n, int32_t reps, int32_t E,
                         float guidance_scale, float clip_range, const float* coef, const float* noise,
                         const int32_t* step_counter, void* stream) {
  if (!pred || !latents || !coef || !step_counter) return RCDM_EINVAL;
  if (n <= 0 || (reps != 1 && reps != 2) || E <= 0 || ld < E) return RCDM_EINVAL;
  const size_t total = (size_t)n * E;
  hipLaunchKernelGGL(cfg_unclip_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f16*)pred, ld, latents, n, reps, E, guidance_scale, clip_range, coef, noise, step_counter);
  return rcdm_check_launch();
}

int rcdm_load_timestep(const float* timesteps, const int32_t* step_counter, float* t_out, int32_t rows, void* stream) {
  if (!timesteps || !step_counter || !t_out || rows <= 0 || rows > 64) return RCDM_EINVAL;
  hipLaunchKernelGGL(load_timestep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, timesteps, step_counter, t_out, rows);
  return rcdm_check_launch();
}

int rcdm_load_table_row(const float* table, const int32_t* step_counter, float* dst, size_t row_floats, void* stream) {
  if (!table || !step_counter || !dst || row_floats == 0 || (row_floats & 3)) return RCDM_EINVAL;
  if (((uintptr_t)table | (uintptr_t)dst) & 15) return RCDM_EINVAL;
  size_t blocks = (row_floats / 4 + 255) / 256;
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(load_table_row_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, step_counter,
                     dst, row_floats);
  return rcdm_check_launch();
}

int rcdm_advance_step(int32_t* step_counter, void* stream) {
  if (!step_counter) return RCDM_EINVAL;
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_counter);
  return rcdm_check_launch();
}

int rcdm_pack_f16(const float* src, void* dst, size_t n, void* stream) {
  if (!src || !dst) return RCDM_EINVAL;
  if (n == 0) return RCDM_OK;
  hipLaunchKernelGGL(pack_f16_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, src, (f16*)dst, n);
  return rcdm_check_launch();
}

int rcdm_mish(const float* x, float* y, size_t n, void* stream) {
  if (!x || !y) return RCDM_EINVAL;
  if (n == 0) return RCDM_OK;
  hipLaunchKernelGGL(mish_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return rcdm_check_launch();
}

int rcdm_pack_conv3x3(const float* w, int32_t c_out, int32_t c_in, int32_t cin_pad, void* dst, void* stream) {
  if (!w || !dst || c_out <= 0 || c_in <= 0 || cin_pad < c_in || (cin_pad & 7)) return RCDM_EINVAL;
  const size_t n = (size_t)c_out * 9 * cin_pad;
  hipLaunchKernelGGL(pack_conv3x3_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in, cin_pad,
                     (f16*)dst);
  return rcdm_check_launch();
}

int rcdm_matmul_f32(const float* A, const float* B, float* C, int32_t n, int32_t k, int32_t m, void* stream) {
  if (!A || !B || !C || n <= 0 || k <= 0 || m <= 0) return RCDM_EINVAL;
  hipLaunchKernelGGL(matmul_f32_kernel, dim3((m + 31) / 32, (n + 31) / 32), dim3(256), 0, (hipStream_t)stream, A, B, C, n, k, m);
  return rcdm_check_launch();
}

int rcdm_pack_conv3x3_up2(const float* w, int32_t c_out, int32_t c_in, void* dst, void* stream) {
  if (!w || !dst || c_out <= 0 || c_in <= 0 || (c_in & 7)) return RCDM_EINVAL;
  const size_t n = (size_t)16 * c_out * c_in;
  hipLaunchKernelGGL(pack_conv3x3_up2_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, w, c_out, c_in, (f16*)dst);
  return rcdm_check_launch();
}

int rcdm_pack_geglu_rows(const float* w, const float* bias, int32_t n_out, int32_t K, void* w_dst, float* bias_dst,
                         void* stream) {
  if (!w || !w_dst || n_out <= 0 || K <= 0) return RCDM_EINVAL;
  if (n_out % 32) return RCDM_ESHAPE;
  const size_t n = (size_t)n_out * K;
  hipLaunchKernelGGL(pack_geglu_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, w, bias, n_out, K,
                     (f16*)w_dst, bias_dst);
  return rcdm_check_launch();
}

}  // extern "C"
