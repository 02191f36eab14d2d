// igemm_plan.h — the host-side planner of the implicit-GEMM launches (igemm_plan.hip; no kernels): which tile variant runs a
// GEMM / conv3x3 and how it is split along K.  Every query entry point of the C ABI (workspace bytes, statistics slot counts,
// plan queries, *_ok) and every launch entry of igemm.hip gets its plan from plan_gemm / plan_conv, so a query answers the
// way the launch itself decides by construction.
#pragma once
#include <stddef.h>
#include "igemm_args.h"

// Tile variants (rcdm_set_igemm_variant, RCDM_SHAPE_RULES, plan queries: the numbers are part of the C ABI).
enum Variant : int {
  kVar128 = 1,        // 128x128, two blocks per CU: the default tile
  kVar256 = 2,        // 256x256, 8 waves, one block per CU
  kVar64 = 3,         // 64x64, two-slot ring, four blocks per CU
  kVar64Deep = 4,     // 64x64, four-slot ring (three steps in flight), two blocks per CU
  kVar128x64 = 5,     // 128x64, three blocks per CU
  kVarPP = 6,         // 6 / 7 / 8: the ping-pong kernel of igemm8.hip at 160x320 / 160x256 / 256x256 (kVarPP + shape index)
  kVarPP256 = 8,
  kVar160 = 9,        // igemm16.hip: 160x160, two blocks per CU
  // 10: the igemm_dma loop at 128x64 with a THREE-slot LDS ring, two blocks per CU (GEMMs only; a conv runs as 5).  Measured
  // in the replayed graph (profiles/r4_shape_rules_ab.txt): -0.09 ms per step on the thirty-five N = C = K = 1280 projections of
  // the 16x16 level, worse everywhere else — as were a four-slot 128x64 ring and a three-slot 128x128 ring (one block per CU
  // each; built, tested, removed): one more stage in flight pays only where it does not cost the third co-resident block
  // more than the latency it hides.
  kVar128x64Deep = 10,
  kNumVariants = 11,
};
enum Family { kFamDma, kFamPP, kFam160 };   // igemm.hip (igemm_dma_kernel) / igemm8.hip / igemm16.hip
// what a variant has no kernel instantiation for
enum : int { kNoStats = 1, kNoConsumer = 2, kNoConv = 4, kNoQuickGelu = 8 };

constexpr int kLnxTabBytes = 3328;   // behind the ring of an LDS-DMA tile, deferred LayerNorm: [BM][2] floats (rstd, mean rstd) + 4 [BN] floats (S, bias, two row vectors) + the slot widths
struct VariantRow {
  int bm, bn, wm, wn, ring;   // tile, wave grid, LDS ring depth
  int blocks_per_cu;
  Family family;
  int cannot;                 // kNo* bits
  int instead;                // the variant that runs such a launch in its place (0: none — the planner never sends one here)
  constexpr int threads() const { return wm * wn * 64; }
  constexpr int lds_bytes() const {   // dynamic LDS of a block
    return family == kFamDma ? ring * (bm + bn) * 128 + kLnxTabBytes : family == kFamPP ? (2 * bm + 3 * bn) * 128 : ring * (bm + bn) * 128;
  }
};
// Row 0 (rcdm_set_igemm_variant(0)) runs as variant 1.
// The 256x256 LDS-DMA tile is at the 256-register cap: its statistics / deferred-LayerNorm instantiations spilled (12 /
// 200 B of scratch) and are not built — such launches take the 128x128 tile, also when variant 2 is forced
// (so did its quick-GELU instantiation, 8 B: the same rule).  Row statistics come out of the igemm_dma epilogue only; the
// 256x256 ping-pong tile has no consumer epilogue (register cap).
inline constexpr VariantRow kVariants[kNumVariants] = {
    {128, 128, 2, 2, 2, 2, kFamDma, 0, 0},
    {128, 128, 2, 2, 2, 2, kFamDma, 0, 0},                                          // 64 KB
    {256, 256, 2, 4, 2, 1, kFamDma, kNoStats | kNoConsumer | kNoQuickGelu, kVar128},  // 128 KB
    {64, 64, 2, 2, 2, 4, kFamDma, 0, 0},                                            // 32 KB
    {64, 64, 2, 2, 4, 2, kFamDma, 0, 0},                                            // 64 KB
    {128, 64, 2, 2, 2, 3, kFamDma, 0, 0},                                           // 48 KB
    {160, 320, 2, 4, 2, 1, kFamPP, kNoStats, 0},                                    // 160 KB
    {160, 256, 2, 4, 2, 1, kFamPP, kNoStats, 0},
    {256, 256, 2, 4, 2, 1, kFamPP, kNoStats | kNoConsumer, 0},                      // 160 KB
    {160, 160, 2, 2, 2, 2, kFam160, kNoStats, 0},                                   // 80 KB
    {128, 64, 2, 2, 3, 2, kFamDma, kNoConv, kVar128x64},                            // 72 KB
};
inline bool is_pp(int v) { return kVariants[v].family == kFamPP; }
inline bool is_dma(int v) { return kVariants[v].family == kFamDma; }

// what steers a plan besides the descriptor: whether the launch leaves row statistics (producer of a deferred LayerNorm),
// whether it consumes them, and — a producer whose caller fixes the slot count of the statistics buffer — that count (0: the
// shape's own)
struct PlanFlags {
  bool producer = false, consumer = false;
  int parts = 0;
};

// The plan of a GEMM / of a conv3x3 in any of its forms (plain, c_in2 > 0, upsample == 2: the phase form, variant =
// kVarPP + tile shape): fills the geometry fields of `a` (no pointers) and `variant`.  RCDM_OK or the error every entry
// point reports for such a descriptor.
int plan_gemm(const rcdm_gemm_desc* d, PlanFlags f, IgemmArgs& a, int& variant);
int plan_conv(const rcdm_conv3x3_desc* d, IgemmArgs& a, int& variant);
void from_gemm(const rcdm_gemm_desc* d, IgemmArgs& a);   // the shape fields alone (rcdm_gemm_ln plans its one tile itself)
int variant_for_parts(const IgemmArgs& a, int parts);
inline size_t slab_bytes(const IgemmArgs& a) {   // split-K workspace of a planned launch
  return a.splits > 1 ? (size_t)a.splits * a.M * a.N * sizeof(float) : 0;
}
int check_common(const IgemmArgs& a);
int attach_gnstat(IgemmArgs& a, const rcdm_groupnorm_desc* gn, void* gn_ws, size_t gn_ws_bytes, bool need_ws);
int slab16_mode();
