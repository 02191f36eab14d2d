// wino_loader.h — launch arguments of the Winograd conv3x3 (wino.hip) and the work dealing and operand addressing of its
// batched GEMM (wino_gemm_kernel): which (entry, split-K slice, tile) a block computes, and the byte offset (or kIgemmOOB) of
// every 16-byte piece of its two operands.  __host__ __device__ like igemm_loader.h, whose swizzle, out-of-bounds mark and
// XCD dealing it uses: tools/igemm_loader_host.cpp runs it on the CPU for tests/test_gemm_exact_host.py.
#pragma once
#include "igemm_loader.h"

struct WinoArgs {
  // conv geometry
  const f16* in;
  const f16* in2;
  const f16* U;      // f16 [16][N][K]   (rcdm_pack_conv3x3_wino)
  const f16* W2;     // f16 [N][K2]      (1x1 weight of the second input) or null
  const float* bias;
  const float* rowvec;
  const f16* res;
  f16* out;
  f16* V;            // workspace: f16 [16][T][K]
  float* slab;       // workspace: fp32 (or, slab16 != 0, f16) [E][splits][T][N]
  int slab16;
  int n_img, H, W, th, tw, T, N, K, K2;
  int lda, lda2, ldc, ldr, ldt, rows_per_sample;
  int epi;
  float out_scale;
  int E, splits, nk, nk2, nkps, nkps2, tilesM, tilesN;
  // GroupNorm (+ SiLU) applied to `in` by the input transform (null: `in` is used as it is)
  const float* gn_stat;   // [samples][G][2] = (mean, rstd)
  const float* gn_gamma;
  const float* gn_beta;
  int gn_cg, gn_G, gn_rps, gn_silu;
  // partial statistics of the GroupNorm that reads `out` NEXT, left by the output transform (null: none): one partial
  // (count, mean, M2) per (sample, group, tile of the sample), the layout gn_finalize_kernel reads with splits = tiles per sample
  float* go_partial;
  int go_G, go_cg, go_rps, go_splits;
};

constexpr int kWinoTile = 160;   // the GEMM's tile, rows and columns

// Work item of block lin = (entry, split-K slice, tile), ordered entry-major with the second input's four entries first (their
// K is the other tensor's width, usually the longer loop).  Every XCD gets a CONTIGUOUS run of items (xcd_run_index): whole
// entries per XCD (two positions each at E = 16), i.e. every byte of U and V is fetched into exactly one L2.  (Tiles of one
// entry spread over all XCDs — the first version — pulled each V[pos] into all eight L2s: 260 MB through the fabric instead
// of 78 MB at the 16x16 level, 45 us instead of 36.)
struct WinoItem {
  int entry, split, m0, n0;
};
__host__ __device__ __forceinline__ WinoItem wino_item(const WinoArgs& p, int lin) {
  const int ntile = p.tilesM * p.tilesN, W = p.E * p.splits * ntile;
  const int n_extra = p.E - 16;
  const int WX = n_extra * p.splits * ntile, WM = W - WX;   // items of the second input's entries (first in item order) / of the 16 positions
  int item;
  if (((WX | WM) & 7) == 0) {
    // every XCD takes its share of the long entries first, then its run of positions
    const int xcd = lin & 7, j = lin >> 3;
    const int xq = WX >> 3, mq = WM >> 3;
    item = j < xq ? xcd * xq + j : WX + xcd * mq + (j - xq);
  } else {
    item = xcd_run_index(lin, W);
  }
  const int yes = item / ntile, tl = item - yes * ntile;
  const int ye = yes / p.splits, split = yes - ye * p.splits;
  const int tn = tl / p.tilesM, tm = tl - tn * p.tilesM;
  return {ye < n_extra ? 16 + ye : ye - n_extra, split, tm * kWinoTile, tn * kWinoTile};
}

// entry e < 16 is V[e] (T x K) against U[e] (N x K); entries 16 + 2a + b are the pixels (2ty + a, 2tx + b) of in2 against W2
__host__ __device__ __forceinline__ int wino_kd(const WinoArgs& p, int entry) { return entry >= 16 ? p.K2 : p.K; }   // contraction width = W row length

// Byte offset of tile row m of the entry's A operand (from V + entry T K, or from in2), or kIgemmOOB past T
__host__ __device__ __forceinline__ unsigned wino_a_row(const WinoArgs& p, int entry, int m) {
  if (m >= p.T) return kIgemmOOB;
  if (entry < 16) return (unsigned)m * (unsigned)p.K * 2u;
  // tile m -> pixel (2ty + a, 2tx + b) of in2
  const int tpi = p.th * p.tw;
  const int img = m / tpi, rem = m - img * tpi;
  const int ty = rem / p.tw, tx = rem - ty * p.tw;
  const int ab = entry - 16;
  const int prow = img * p.H * p.W + (2 * ty + (ab >> 1)) * p.W + 2 * tx + (ab & 1);
  return (unsigned)prow * (unsigned)p.lda2 * 2u;
}
// ... of row n of its weight operand (from U + entry N K, or from W2), or kIgemmOOB past N
__host__ __device__ __forceinline__ unsigned wino_w_row(const WinoArgs& p, int entry, int n) {
  return n < p.N ? (unsigned)n * (unsigned)wino_kd(p, entry) * 2u : kIgemmOOB;
}
// ... and of channels [c, c + 8) of either row at a k-step (c = the step's first channel + igemm_swizzle_chunk)
__host__ __device__ __forceinline__ unsigned wino_piece_offset(unsigned row_off, int c, int Kd) {
  return (c < Kd && row_off != kIgemmOOB) ? row_off + (unsigned)c * 2u : kIgemmOOB;
}
