// objective_core.h — the lane-free rules of the stage-2 denoising objective (include/rcdm.h, "Denoising objective"): the
// forward-diffusion step that fills the UNet's input rows and the squared error of its epsilon prediction.  Plain C++:
// objective.hip runs it on the device and tools/objective_host.cpp runs the same functions on one CPU thread;
// tests/objective_oracle.py restates them in numpy.
//   target      n = noise + (offs_scale * offs[b][c][f])       two float32 roundings, the product first; without offs n = noise
//               (train_stage2.py:445-449: noise += noise_offset * randn(B, 4, f, 1, 1)).
//   input rows  channels 0..3 = f16_rn((sa * x0) + (s1m * n)), (sa, s1m) = table[t[b]]: three float32 roundings and the round
//               to nearest even into f16, what torch's mul, mul and add kernels followed by .half() give.  A story whose t lies
//               outside [0, T) reads no table row and gets the f16 quiet NaN 0x7E00 in channels 0..3.  Channel 4 = f16_rn(mask),
//               channels 5..8 = f16_rn(masked), channels 9..c_pad-1 = +0.  A row is written as c_pad / 8 groups of 8 halves.
//   squared error of frame (b, f): sum over the frame's 4 H W elements of (double(eps) - double(n))^2 in this fixed order:
//     pixel     d_c = double(eps_c) - double(n_c), c = 0..3;  q = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + d_3 d_3, every product and
//               every sum rounded to float64 on its own.
//     chunk     the frame's pixels in row-major order are cut into chunks of CHUNK = 256 from the frame's first pixel; a chunk
//               is 256 slots, slot i = q of pixel 256 j + i or +0.0 past the frame's end; then the binary tree
//               part[i] += part[i + s], s = 128, 64 .. 1 (chunk_tree).
//     frame     the chunk sums in ascending order, starting from +0.0 (the fold launch).
//   The longest chain of additions an element passes through is 3 + 8 + (chunks - 1): addition_chain().  Nothing above
//   depends on the launch geometry, there are no atomics and no memset: the same input gives the same bits.  NaN and inf
//   propagate through every step.
// No expression here may be contracted into an FMA.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OB_HD __host__ __device__ inline
#else
#define OB_HD inline
#endif
#if defined(__clang__)
#define OB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define OB_NO_CONTRACT
#endif

namespace ob {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;                       // pixels of one chunk = slots of the tree = threads of a block
constexpr int LATENT_CHANNELS = 4;
constexpr int MASK_CHANNEL = 4;                  // then the four masked-latent channels
constexpr int IN_CHANNELS = 9;
constexpr int GROUP = 8;                         // halves of one 16-byte store
constexpr uint16_t F16_NAN = 0x7E00;
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;   // B f H W below this
constexpr int MAX_BLOCKS = 65535;

OB_HD int64_t chunks_per_frame(int64_t hw) { return (hw + CHUNK - 1) / CHUNK; }
OB_HD int addition_chain(int64_t hw) { return 3 + 8 + (int)(chunks_per_frame(hw) - 1); }
OB_HD bool timestep_valid(int64_t t, int T) { return t >= 0 && t < (int64_t)T; }

// noise + offs_scale * offs, the product rounded first
OB_HD float target(float noise, float offs_scale, float offs) {
  OB_NO_CONTRACT
  const float p = offs_scale * offs;
  const float n = noise + p;
  return n;
}

// sa x0 + s1m n in three roundings
OB_HD float add_noise(float sa, float x0, float s1m, float n) {
  OB_NO_CONTRACT
  const float a = sa * x0;
  const float b = s1m * n;
  const float s = a + b;
  return s;
}

// one pixel: eps[c] already widened (exactly) from f16, n[c] the float32 targets
OB_HD double pixel_sqerr(const float (&eps)[4], const float (&n)[4]) {
  OB_NO_CONTRACT
  const double d0 = (double)eps[0] - (double)n[0];
  const double d1 = (double)eps[1] - (double)n[1];
  const double d2 = (double)eps[2] - (double)n[2];
  const double d3 = (double)eps[3] - (double)n[3];
  const double p0 = d0 * d0;
  const double p1 = d1 * d1;
  const double p2 = d2 * d2;
  const double p3 = d3 * d3;
  double q = p0 + p1;
  q = q + p2;
  q = q + p3;
  return q;
}

inline double chunk_tree(double* part) {
  for (int s = CHUNK / 2; s > 0; s >>= 1)
    for (int i = 0; i < s; ++i) part[i] += part[i + s];
  return part[0];
}

}  // namespace ob
