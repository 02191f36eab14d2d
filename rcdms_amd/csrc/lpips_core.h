// lpips_core.h — the lane-free arithmetic of the LPIPS distance head (include/rcdm.h, "LPIPS"): the learned perceptual distance
// of Zhang et al., The Unreasonable Effectiveness of Deep Features as a Perceptual Metric (2018), for one tap of a feature tower.
// Plain C++: lpips.hip runs it on the device and tools/lpips_host.cpp runs the same functions on one CPU thread;
// tests/lpips_oracle.py restates them in numpy.
//   pixel       a[0 .. C), b[0 .. C): the f16 features of the two frames at one position, widened exactly to fp32.
//                 na = sqrt(sum_c a_c^2) + 1e-10 (the epsilon AFTER the root, as the lpips package's normalize_tensor), nb likewise;
//                 v  = sum_c lin_c (a_c / na - b_c / nb)^2,   all in fp32, true divisions (a_c / na with a = s e_i is exactly 1
//                 for s >= 2^-9, where 1e-10 is below half an ulp of s: a reciprocal multiply would not give that).
//   lanes       the C channels are cut into chunks of 8 (one 16-byte load); chunk k belongs to lane k of the pixel's group of
//               L = lanes(C) lanes, the smallest power of two >= C / 8 (C <= 512: L <= 64, a wave).  Lanes k >= C / 8 hold +0.0.
//                 1. a lane adds its 8 squares (sumsq8) or its 8 terms lin (d d) (term8) in channel order from +0.0;
//                 2. the L lane sums go through the binary tree part[t] += part[t + s], s = L / 2 .. 1 (group_tree; the device's
//                    xor butterfly leaves the tree's part[0] in every lane, since fp32 addition commutes).
//   tile        the h w pixels of a pair are cut into tiles of TILE = 64 consecutive pixels (one workgroup's job: small enough
//               that the 32 x 32 tap of a few pairs still fills the chip).  The pixel values of a tile are widened to float64
//               (exact), positions past h w are +0.0, and the 64 values go through the same binary tree (tile_tree).  One tile
//               partial per (pair, tile) is written to the workspace.
//   pair        the tiles(h w) partials of a pair go through fr's fixed sum (lane t of 256 adds partials t, t + 256, ... in
//               ascending order from +0.0, then the tree) and are divided once by (double)(h w) (pair_mean).
//               Which workgroup computes which tile is the host's choice and changes nothing: no atomics, no memset, the same
//               input gives the same bits for every grid size.
// No expression here may be contracted into an FMA: the model in numpy has none, and the three agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frechet_core.h"

namespace lp {

constexpr int MAX_C = 512;                // channels of one tap: one 16-byte chunk per lane of a wave
constexpr int CHUNK = 8;
constexpr int TILE = 64;                  // pixels behind one float64 partial
constexpr int MAX_PAIRS = 65535;
constexpr float EPS = 1e-10f;

FR_HD int lanes(int c) {
  int l = 1;
  while (l * CHUNK < c) l <<= 1;
  return l;
}

FR_HD int64_t tiles(int64_t hw) { return (hw + TILE - 1) / TILE; }

FR_HD float sumsq8(const float* v) {
  FR_NO_CONTRACT
  float s = 0.0f;
  for (int e = 0; e < CHUNK; ++e) s += v[e] * v[e];
  return s;
}

FR_HD float norm(float sumsq) {
  FR_NO_CONTRACT
  return sqrtf(sumsq) + EPS;
}

FR_HD float term8(const float* a, const float* b, float na, float nb, const float* lin) {
  FR_NO_CONTRACT
  float s = 0.0f;
  for (int e = 0; e < CHUNK; ++e) {
    const float d = a[e] / na - b[e] / nb;
    s += lin[e] * (d * d);
  }
  return s;
}

// the binary tree over the L lane sums of one pixel, in place (what the device's xor butterfly leaves in every lane)
inline float group_tree(float* part, int L) {
  for (int s = L / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) part[t] += part[t + s];
  return part[0];
}

// the binary tree over the TILE pixel values of a tile, in place
inline double tile_tree(double* v) {
  for (int s = TILE / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) v[t] += v[t + s];
  return v[0];
}

FR_HD double pair_mean(double sum, int64_t hw) { return sum / (double)hw; }

// the longest chain of float64 additions behind one pair: 6 levels of the tile's tree, the strided partial sums over the
// tiles and the 8 levels of their tree
FR_HD int64_t chain(int64_t hw) { return 6 + (tiles(hw) + fr::LANES - 1) / fr::LANES + 8; }

}  // namespace lp
