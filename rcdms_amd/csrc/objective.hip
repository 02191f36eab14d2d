// objective.hip — the stage-2 denoising objective around the UNet (include/rcdm.h, "Denoising objective"; csrc/objective_core.h
// has every rule and the order of every sum).
//   rcdm_diffuse_assemble   one launch: forward diffusion at one timestep per story, read from the device, and the 9-channel f16
//     diffuse_assemble_kernel   input rows.  A thread per (row, group of 8 channels): consecutive lanes store consecutive 16
//                               bytes of a row.  Group 0 holds the four noised latents, the mask and three masked latents,
//                               group 1 the fourth and zeros, every later group zeros.
//   rcdm_eps_sqerr          out[B][f], two launches:
//     eps_sqerr_chunk_kernel    a block walks chunks of 256 pixels of one frame (chunk j, j + gridDim.x, ...): a thread per
//                               pixel, one 8-byte load of the four f16 predictions, ob::pixel_sqerr, then ob::chunk_tree's
//                               order through LDS.  The chunk's sum goes to the workspace.
//     eps_sqerr_fold_kernel     a thread per frame: its chunk sums in ascending order.
// Every offset is formed in int64.  No atomics, no memset; no scratch (profiles/objective_kernel_resources.txt).
#include "common.h"
#include "objective_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = ob::THREADS;
static_assert(NT == ob::CHUNK, "a thread per slot of the chunk tree");

struct diffuse_args {
  const float *x0, *noise, *offs, *table, *mask, *masked;
  const int64_t* t;
  float offs_scale;
  int T, F, groups;
  int64_t hw, rows, ld;
  f16* out;
};

__global__ __launch_bounds__(NT) void diffuse_assemble_kernel(const diffuse_args a) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t row = i / a.groups;
  const int g = (int)(i - row * a.groups);
  if (row >= a.rows) return;
  const int64_t fhw = a.hw * a.F;
  const int64_t b = row / fhw, rem = row - b * fhw;          // rem = f hw + pixel
  Pack16 o;
  o.u = make_uint4(0u, 0u, 0u, 0u);
  if (g == 0) {
    const int64_t t = a.t[b];
    const bool valid = ob::timestep_valid(t, a.T);
    const float sa = valid ? a.table[2 * t] : 0.0f, s1m = valid ? a.table[2 * t + 1] : 0.0f;
    const int64_t f = rem / a.hw;
#pragma unroll
    for (int c = 0; c < ob::LATENT_CHANNELS; ++c) {
      const int64_t e = (b * ob::LATENT_CHANNELS + c) * fhw + rem;
      float n = a.noise[e];
      if (a.offs) n = ob::target(n, a.offs_scale, a.offs[(b * ob::LATENT_CHANNELS + c) * a.F + f]);
      const f16 v = (f16)ob::add_noise(sa, a.x0[e], s1m, n);
      o.e[c] = valid ? v : __builtin_bit_cast(f16, ob::F16_NAN);
    }
    o.e[ob::MASK_CHANNEL] = (f16)a.mask[b * fhw + rem];
#pragma unroll
    for (int c = 0; c < 3; ++c) o.e[5 + c] = (f16)a.masked[(b * ob::LATENT_CHANNELS + c) * fhw + rem];
  } else if (g == 1) {
    o.e[0] = (f16)a.masked[(b * ob::LATENT_CHANNELS + 3) * fhw + rem];
  }
  *(uint4*)(a.out + row * a.ld + (int64_t)g * ob::GROUP) = o.u;
}

struct sqerr_args {
  const f16* eps;
  const float *noise, *offs;
  float offs_scale;
  int F;
  int64_t hw, ld, cpf, chunks, frames;      // cpf: chunks per frame; chunks = frames * cpf
  double* part;
  double* out;
};

__global__ __launch_bounds__(NT) void eps_sqerr_chunk_kernel(const sqerr_args a) {
  __shared__ double part[ob::CHUNK];
  const int tid = threadIdx.x;
  for (int64_t j = blockIdx.x; j < a.chunks; j += gridDim.x) {        // the whole block
    const int64_t bf = j / a.cpf;
    const int64_t p = (j - bf * a.cpf) * ob::CHUNK + tid;
    double q = 0.0;
    if (p < a.hw) {
      const int64_t b = bf / a.F, f = bf - b * a.F;
      const f16x4 u = *(const f16x4*)(a.eps + (bf * a.hw + p) * a.ld);
      float ev[4], nv[4];
#pragma unroll
      for (int c = 0; c < ob::LATENT_CHANNELS; ++c) {
        const int64_t bc = b * ob::LATENT_CHANNELS + c;
        float n = a.noise[(bc * a.F + f) * a.hw + p];
        if (a.offs) n = ob::target(n, a.offs_scale, a.offs[bc * a.F + f]);
        ev[c] = (float)u[c];
        nv[c] = n;
      }
      q = ob::pixel_sqerr(ev, nv);
    }
    part[tid] = q;
    __syncthreads();
#pragma unroll
    for (int s = ob::CHUNK / 2; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    if (tid == 0) a.part[j] = part[0];      // part[0] is this thread's own slot: the next pass may start
  }
}

__global__ __launch_bounds__(NT) void eps_sqerr_fold_kernel(const sqerr_args a) {
  const int64_t bf = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (bf >= a.frames) return;
  double s = 0.0;
  for (int64_t j = 0; j < a.cpf; ++j) s += a.part[bf * a.cpf + j];
  a.out[bf] = s;
}

// RCDM_OK, or what is wrong with the geometry both entry points share
int geometry_check(int32_t B, int32_t frames, int32_t H, int32_t W) {
  if (B < 1 || frames < 1 || H < 1 || W < 1) return RCDM_EINVAL;
  const double rows = (double)B * frames * H * W;
  return rows >= (double)ob::MAX_ROWS ? RCDM_ESHAPE : RCDM_OK;
}

}  // namespace

extern "C" {

int rcdm_diffuse_assemble(const float* x0, const float* noise, const float* offs, float offs_scale, const int64_t* t,
                          const float* table, int32_t T, const float* mask, const float* masked, int32_t B, int32_t frames,
                          int32_t H, int32_t W, void* out, int32_t ld, int32_t c_pad, void* stream) {
  if (!x0 || !noise || !t || !table || !mask || !masked || !out || T < 1) return RCDM_EINVAL;
  const int rc = geometry_check(B, frames, H, W);
  if (rc != RCDM_OK) return rc;
  if (((uintptr_t)x0 & 3) || ((uintptr_t)noise & 3) || ((uintptr_t)offs & 3) || ((uintptr_t)table & 3) || ((uintptr_t)mask & 3) ||
      ((uintptr_t)masked & 3) || ((uintptr_t)t & 7) || ((uintptr_t)out & 15))
    return RCDM_EINVAL;
  // whole 16-byte groups: two of them hold the nine channels
  if (c_pad < 2 * ob::GROUP || c_pad > 1024 || (c_pad % ob::GROUP) || ld < c_pad || (ld % ob::GROUP)) return RCDM_ESHAPE;
  diffuse_args a;
  a.x0 = x0;
  a.noise = noise;
  a.offs = offs;
  a.table = table;
  a.mask = mask;
  a.masked = masked;
  a.t = t;
  a.offs_scale = offs_scale;
  a.T = T;
  a.F = frames;
  a.groups = c_pad / ob::GROUP;
  a.hw = (int64_t)H * W;
  a.rows = (int64_t)B * frames * a.hw;
  a.ld = ld;
  a.out = (f16*)out;
  const int64_t total = a.rows * a.groups;
  hipLaunchKernelGGL(diffuse_assemble_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, a);
  return rcdm_check_launch();
}

size_t rcdm_eps_sqerr_workspace_bytes(int32_t B, int32_t frames, int32_t H, int32_t W) {
  if (geometry_check(B, frames, H, W) != RCDM_OK) return 0;
  return (size_t)B * (size_t)frames * (size_t)ob::chunks_per_frame((int64_t)H * W) * sizeof(double);
}

int rcdm_eps_sqerr(const void* eps, int32_t ld, const float* noise, const float* offs, float offs_scale, int32_t B,
                   int32_t frames, int32_t H, int32_t W, int32_t blocks, double* out, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (!eps || !noise || !out || blocks < 0 || blocks > ob::MAX_BLOCKS) return RCDM_EINVAL;
  const int rc = geometry_check(B, frames, H, W);
  if (rc != RCDM_OK) return rc;
  if (((uintptr_t)eps & 7) || ((uintptr_t)noise & 3) || ((uintptr_t)offs & 3) || ((uintptr_t)out & 7) || ((uintptr_t)workspace & 7))
    return RCDM_EINVAL;
  if (ld < ob::LATENT_CHANNELS || (ld % 4)) return RCDM_ESHAPE;       // one 8-byte load per row
  if (!workspace || workspace_bytes < rcdm_eps_sqerr_workspace_bytes(B, frames, H, W)) return RCDM_EWORKSPACE;
  sqerr_args a;
  a.eps = (const f16*)eps;
  a.noise = noise;
  a.offs = offs;
  a.offs_scale = offs_scale;
  a.F = frames;
  a.hw = (int64_t)H * W;
  a.ld = ld;
  a.cpf = ob::chunks_per_frame(a.hw);
  a.frames = (int64_t)B * frames;
  a.chunks = a.frames * a.cpf;
  a.part = (double*)workspace;
  a.out = out;
  // the library's choice: a block per chunk, as far as the grid goes
  const int64_t grid = blocks > 0 ? blocks : (a.chunks < ob::MAX_BLOCKS ? a.chunks : ob::MAX_BLOCKS);
  hipLaunchKernelGGL(eps_sqerr_chunk_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, a);
  if (rcdm_check_launch() != RCDM_OK) return RCDM_ELAUNCH;
  hipLaunchKernelGGL(eps_sqerr_fold_kernel, dim3((unsigned)((a.frames + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, a);
  return rcdm_check_launch();
}

}  // extern "C"
