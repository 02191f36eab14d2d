// igemm_loader.h — operand addressing of the three implicit-GEMM tile kernels (igemm.hip igemm_dma_kernel, igemm8.hip
// igemm_pp_kernel, igemm16.hip igemm16_kernel): which tile a block computes, what a k-step of 64 reads, and the byte offset
// (or kIgemmOOB) of every 16-byte piece of the activation and weight tiles.  The arithmetic that has to agree between the
// kernels exists here once; ring layout, which wave fills what, when the DMA is issued and the aux bits stay in the kernels.
// Everything is __host__ __device__: tools/igemm_loader_host.cpp runs the same functions on the CPU, where
// tests/test_gemm_exact_host.py gathers the operands through them and compares with the numpy model of tests/gemm_exact.py.
#pragma once
#include "igemm_args.h"

// voffset of a piece that does not exist (a row past M / N, a tap outside the image, a channel chunk past Cin): at or
// beyond num_records of the kernels' buffer resources, so the hardware writes zeros and the loaders have no branches
constexpr unsigned kIgemmOOB = 0x80000000u;

// Contiguous-run-per-XCD dealing: the hardware deals workgroups to the 8 XCDs round-robin by linear id, so block lin runs
// on XCD lin & 7 as that XCD's (lin >> 3)-th block.  Returns the index in a sequence of n work items that gives every XCD
// one contiguous run of it (the first n & 7 runs one item longer): a bijection of [0, n).
__host__ __device__ __forceinline__ int xcd_run_index(int lin, int n) {
  const int xcd = lin & 7, q = n >> 3, r = n & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
}

// XCD-aware, L2-blocked tile order: linear tile index lin -> the tile's first row and column.  Block b runs on XCD b%8, so
// each XCD is given a contiguous run of the tile sequence (xcd_run_index); the sequence itself walks super-rows of GM row panels column by
// column (n outer, m inner inside the super-row), so the ~64 tiles an XCD has in flight form a GM x (64/GM) patch: every
// activation panel is shared by 64/GM tiles and every weight panel by GM tiles *at the same time*.  With plain n-fastest
// order a wide N (GEGLU: 40-80 column tiles) streams the whole weight matrix through the 4 MB L2 once per row panel:
// rocprofv3 FETCH_SIZE showed 16-19x the operand bytes (0.4-0.5 GB per launch, HBM-bound) on the 32x32 / 16x16 levels.
template <int BM, int BN>
__host__ __device__ __forceinline__ void igemm_tile_origin(const IgemmArgs& p, int lin, int& m0, int& n0) {
  constexpr int GM = 8;
  const int tl = xcd_run_index(lin, p.tilesM * p.tilesN);
  const int per_group = GM * p.tilesN;
  const int grp = tl / per_group, rem = tl - grp * per_group;
  const int left = p.tilesM - grp * GM;
  const int gm = left < GM ? left : GM;  // rows in this (possibly last, short) super-row
  const int tn = rem / gm, tm = grp * GM + (rem - tn * gm);
  m0 = tm * BM;
  n0 = tn * BN;
}

// What k-step ks reads: channels [c0, c0 + 64) of tap `tap` at (dy, dx) from the padded origin of the output pixel.
struct IgemmKStep {
  int c0, tap, dy, dx;
  int cin;        // channel count of the input this step reads
  unsigned lda;   // ... and its row stride
  bool s2;        // the second input (wave-uniform)
};
// TAPS = 1 (Linear / 1x1), 9 (conv3x3) or 4 (one 2x2 phase of an upsampling conv).  Channel chunk outer, tap inner: the
// shifted windows of one 64-channel slab are read back to back, so the re-reads hit L2 (one slab of all tiles in flight on
// an XCD is ~2 MB).  Tap-outer order re-read the whole Cin-deep panel (16 MB in flight at Cin = 960) per tap: FETCH_SIZE
// was 10x the input bytes.
// Second input (IgemmArgs::A2, conv launches only): the k-steps from nk1 on are a tenth "tap" — the output pixel itself
// (dy = dx = 1 from the padded origin) in another tensor with its own row stride and channel count, against W columns
// 9 Cin + c.
template <int TAPS>
__host__ __device__ __forceinline__ IgemmKStep igemm_kstep(const IgemmArgs& p, int ks) {
  static_assert(TAPS == 1 || TAPS == 9 || TAPS == 4, "taps");
  IgemmKStep k;
  k.s2 = TAPS == 9 && ks >= p.nk1;
  k.tap = 0;
  int kci = ks;
  if (TAPS != 1) {
    kci = ks / TAPS;
    k.tap = ks - kci * TAPS;
    if (k.s2) {
      kci = ks - p.nk1;
      k.tap = 9;
    }
  }
  k.c0 = kci * BK;
  k.dy = k.s2 ? 1 : TAPS == 4 ? k.tap >> 1 : k.tap / 3;
  k.dx = k.s2 ? 1 : TAPS == 4 ? k.tap & 1 : k.tap - k.dy * 3;
  k.cin = k.s2 ? p.Cin2 : p.Cin;
  k.lda = (unsigned)(k.s2 ? p.lda2 : p.lda);
  return k;
}

// Output row m of the activation operand.  TAPS == 1: `off` is the row's byte offset (kIgemmOOB: dead).  Otherwise img is
// the first pixel row of its image and (iy, ix) the padded origin of its window in the (virtually upsampled) input; a dead
// row carries iy = -(1 << 20), which no tap brings back inside the image — the mark is iy alone: img and ix of a dead row
// are decoded like any other's (selecting all three cost the LDS-DMA conv kernels 3 VGPRs; no address is formed from them
// without igemm_pixel_offset's select).  img holds img * Hi * Wi, not the image number: the offsets are formed in unsigned,
// so (img * Hi + sy) * Wi + sx and img * Hi * Wi + sy * Wi + sx are the same 32-bit value.
struct IgemmPixelRow {
  unsigned off;
  int img, iy, ix;
};
// live: the row exists (inside the tile's pieces and m < p.M); phase: the output parity 2a + b of a phase launch's tile
template <int TAPS>
__host__ __device__ __forceinline__ IgemmPixelRow igemm_pixel_row(const IgemmArgs& p, int m, bool live, int phase = 0) {
  IgemmPixelRow r = {kIgemmOOB, 0, -(1 << 20), 0};
  if (TAPS == 1) {
    if (live) r.off = (unsigned)m * (unsigned)p.lda * 2u;
  } else {
    const int hw = p.Ho * p.Wo;
    const int pm = TAPS == 4 ? m - phase * p.ph_rows : m;   // (phase launch: the source pixel of this virtual row)
    const int img = pm / hw, rem = pm - img * hw;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    r.img = img * p.Hi * p.Wi;
    if (live) r.iy = oy * p.stride - p.pad + (TAPS == 4 ? phase >> 1 : 0);
    r.ix = ox * p.stride - p.pad + (TAPS == 4 ? phase & 1 : 0);
  }
  return r;
}

// Byte offset of channels [c, c + 8) of `row` at k-step k, or kIgemmOOB: the border test against the virtual image
// (Hv, Wv) = (Hi, Wi) << up, the nearest-2x upsample folded in as >> up.  Computed unconditionally and selected (a select,
// not a branch: no address is dereferenced here).
template <int TAPS>
__host__ __device__ __forceinline__ unsigned igemm_pixel_offset(const IgemmArgs& p, const IgemmKStep& k, const IgemmPixelRow& row,
                                                                int c, int Hv, int Wv) {
  if (TAPS == 1) return (c < p.Cin && row.off != kIgemmOOB) ? row.off + (unsigned)c * 2u : kIgemmOOB;
  const int iy = row.iy + k.dy, ix = row.ix + k.dx;
  const bool ok = (c < k.cin) && ((unsigned)iy < (unsigned)Hv) && ((unsigned)ix < (unsigned)Wv);
  const int sy = iy >> p.up, sx = ix >> p.up;
  const unsigned off = ((unsigned)(row.img + sy * p.Wi + sx) * k.lda + (unsigned)c) * 2u;
  return ok ? off : kIgemmOOB;
}

// Byte offset of weight row n (phase launches: of that phase's block of N rows), or kIgemmOOB past N ...
__host__ __device__ __forceinline__ unsigned igemm_weight_row(const IgemmArgs& p, int n, int phase = 0) {
  return n < p.N ? (unsigned)(phase * p.N + n) * (unsigned)p.Ktot * 2u : kIgemmOOB;
}
// ... and of its columns tap * Cin + [c, c + 8) at k-step k (two selects, not one on the and of the conditions: hipcc then
// keeps the per-piece selects on the VALU instead of an s_and_b64 between the DMA issues — 160x160 GEMM, N = 6144: -0.7 us)
__host__ __device__ __forceinline__ unsigned igemm_weight_offset(const IgemmArgs& p, const IgemmKStep& k, unsigned w_off, int c) {
  const unsigned off = w_off == kIgemmOOB ? kIgemmOOB : w_off + ((unsigned)k.tap * (unsigned)p.Cin + (unsigned)c) * 2u;
  return c < k.cin ? off : kIgemmOOB;
}

// Source-side XOR swizzle: the first channel (of the k-step's 64) that the DMA lane with 16-byte chunk index lch brings to
// tile row `row` — LDS slot (row, lch) holds global chunk lch ^ ((row >> 1) & 7).  The read side of the 16x16x32 kernels is
// frag16_lanes (igemm_frag16.h).
__host__ __device__ __forceinline__ int igemm_swizzle_chunk(int row, int lch) { return (lch ^ ((row >> 1) & 7)) * 8; }
