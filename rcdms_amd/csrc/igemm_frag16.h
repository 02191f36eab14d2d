// igemm_frag16.h — the v_mfma_f32_16x16x32_f16 fragment machinery of the tile kernels that read their operands from
// [rows][128 B] LDS tiles (one 64-deep k-step of f16 per row, XOR-swizzled in 16-byte chunks): igemm16.hip igemm16_kernel and
// wino.hip wino_gemm_kernel run the whole 2-stage ring loop below (ring2_tile_loop), igemm8.hip igemm_pp_kernel keeps its
// own ping-pong tick schedule and calls the fragment read and the MFMA run.  Device only.
// Weights are the MFMA A operand, pixels / tile rows the B operand -> D[channel][pixel]: acc[i][j] is the 16x16 fragment of
// weight rows 16 i .. and pixel rows 16 j .. of the wave's tile (accumulator layout: igemm_epilogue.h).
//
// A/B switches that reach this header:
//   RCDM_PRIO_LOADS (igemm_args.h; -DRCDM_PRIO_LOADS=0 drops the priority flips) governs EVERY user of frag16_mfma and
//   ring2_tile_loop — the Winograd GEMM included, whose copy of the loop used to flip unconditionally;
//   ring2_tile_loop's ABLATE argument: igemm16.hip passes its RCDM_I16_ABLATE & 8, wino.hip passes 0 (tools/run_i16_ablate.sh
//   measures the 160x160 GEMM / conv kernel only).
#pragma once
#include "igemm_args.h"
#include "pp_sync.h"

// Lane map of one fragment read.  Lane l holds row l15 of a 16-row fragment and, per 32-deep half k-step, the 8 halfs of
// k group kg: 16-byte chunk kg of the row for the first half, 4 + kg for the second.  The tile is stored swizzled — LDS slot
// (row, lch) holds source chunk lch ^ ((row >> 1) & 7), the source side of which is igemm_swizzle_chunk (igemm_loader.h) —
// so the chunk is found at slot chunk ^ sw, sw = (row >> 1) & 7 of this lane's fragment rows: fragment bases are multiples
// of 16, so that is (l15 >> 1) & 7 = (lane >> 1) & 7 for every fragment of the lane.  koff0 / koff1: the byte offsets inside
// the row of the two half k-steps.
struct Frag16Lanes {
  int l15, kg, koff0, koff1;
};
__device__ __forceinline__ Frag16Lanes frag16_lanes(int lane) {
  const int l15 = lane & 15, kg = lane >> 4;
  const int sw = (lane >> 1) & 7;
  const int koff0 = ((kg ^ sw) << 4);
  const int koff1 = (((4 + kg) ^ sw) << 4);
  return {l15, kg, koff0, koff1};
}

template <int FN, int FM>
__device__ __forceinline__ void frag16_zero(f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The fragments of one 32-deep half k-step: sb / sa point at this lane's row of the first weight / pixel fragment, koff is
// the half k-step's offset inside the row (koff0 / koff1); the next fragment is 16 rows = 2048 bytes on.  koff is added LAST,
// per read: with it folded into sa / sb by the caller hipcc orders the 160x160 loop's reads so that the first MFMA's weight
// fragment arrives last (+1.3 % on the 8192^3 GEMM, measured).
template <int FN, int FM>
__device__ __forceinline__ void frag16_load(const char* sa, const char* sb, int koff, f16x8 (&wf)[FN], f16x8 (&xf)[FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i) wf[i] = *(const f16x8*)(sb + i * 2048 + koff);
#pragma unroll
  for (int j = 0; j < FM; ++j) xf[j] = *(const f16x8*)(sa + j * 2048 + koff);
}

// The FN x FM MFMA run at LOW priority, everything else of the wave (address arithmetic, ds_read, DMA issue) at high
// priority.  The SIMD issues oldest-first among equal priorities, and a wave whose next MFMA waits for the matrix pipe keeps
// the other wave's VALU instructions from issuing (tools/ubench/pipe_overlap.hip: a VALU wave beside two MFMA-streaming
// waves gets one instruction per 23 clocks at equal priority, one per 6.4 at s_setprio 3, with the MFMA rate unchanged).
// RCDM_PRIO_LOADS == 0: no flips; PRIO1 (the ping-pong kernel only): its round-2 form instead, the MFMA run at priority 1
// and nothing else raised (-0.05 ms per step against the current form).
template <int FN, int FM, bool PRIO1 = false>
__device__ __forceinline__ void frag16_mfma(const f16x8 (&wf)[FN], const f16x8 (&xf)[FM], f32x4 (&acc)[FN][FM]) {
  constexpr int kRun = RCDM_PRIO_LOADS ? 0 : 1, kRest = RCDM_PRIO_LOADS ? 3 : 0;
  if constexpr (RCDM_PRIO_LOADS || PRIO1) __builtin_amdgcn_s_setprio(kRun);
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
  if constexpr (RCDM_PRIO_LOADS || PRIO1) __builtin_amdgcn_s_setprio(kRest);
}

// The k-loop of a block of 4 waves (2 x 2, wave (wm, wn) computes the (BM/2) x (BN/2) quarter) over a 2-stage ring of
// [BM pixel rows | BN weight rows] x 128 B stages at smem, filled by the caller's LDS-DMA functor issue(g, stage) (k-step g
// of this block's nkl into ring stage `stage`).  The caller has issued step 0 into stage 0; one s_barrier per 64-deep k-step.
// ABLATE (debug builds): no DMA after the caller's first stage.
template <int BM, int BN, int FM, int FN, bool ABLATE, class Issue>
__device__ __forceinline__ void ring2_tile_loop(const char* smem, int nkl, int wm, int wn, int lane, Issue&& issue, f32x4 (&acc)[FN][FM]) {
  constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
  const Frag16Lanes fl = frag16_lanes(lane);
  const int rowA = (wm * (BM / 2) + fl.l15) * 128, rowB = A_BYTES + (wn * (BN / 2) + fl.l15) * 128;
  for (int g = 0; g < nkl; ++g) {
    // this wave's pieces of step g have landed (nothing newer is in flight); the barrier makes everybody's visible and
    // says everybody is done reading the stage of step g-1, which the issue below refills
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if constexpr (!ABLATE)
      if (g + 1 < nkl) issue(g + 1, (g + 1) & 1);
    const char* sb = smem + (g & 1) * STAGE;
#if RCDM_PRIO_LOADS   // everything but the MFMA runs of a k-step at raised priority (frag16_mfma)
    __builtin_amdgcn_s_setprio(3);
#endif
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int koff = kk ? fl.koff1 : fl.koff0;
      f16x8 wf[FN], xf[FM];
      frag16_load<FN, FM>(sb + rowA, sb + rowB, koff, wf, xf);
      frag16_mfma<FN, FM>(wf, xf, acc);
    }
  }
}
