// rowff.hip — ROW-STATIONARY fused token-matrix chains for gfx950 (the C = 320 level of the 512x512 UNet).
//
//   rcdm_ff_fused :  out = x + FeedForward_geglu(LayerNorm(x))                                      (one launch)
//   rcdm_rowchain :  tok = a W_a^T + b_a (+ res);  y = LayerNorm(tok) (+ pe);  then one of
//                      out = y W_t^T                      (N = C: cross-attention query, N = 3C: fused q | k | v)
//                      out = tok + FeedForward_geglu(y)   (y computed with the feed-forward's own LayerNorm)
//                      out = z_res + (tok + FeedForward_geglu(y)) W_z^T + b_z     (tail 2: the block's proj_out rides too)
//                      out = temporal self-attention of q | k | v = y W_t^T       (tail 4: q, k, v never leave the CU)
// Replace, per launch, the chains the library otherwise runs as 3-5 launches with every intermediate tensor in HBM:
//   * nn.LayerNorm -> diffusers FeedForward(dim, activation_fn="geglu") -> + hidden_states
//     (BasicTransformerBlock.forward src/models/attention.py:514, TemporalTransformerBlock.forward motion_module.py:243);
//   * proj_in / to_out[0] (+ residual) -> norm1 / norm2 / norms[i] (+ PositionalEncoding) -> to_q | to_k | to_v
//     (attention.py:330,482-499,121,139-141; motion_module.py:166,236-241,299-302);
//   * to_out[0] + residual -> norm3 / ff_norm -> ff -> + residual (attention.py:164,514; motion_module.py:243);
//   * the q | k | v chain of a motion module and the attention over the frames behind it (motion_module.py:299-302).
//
// Decomposition (round 3): the implicit-GEMM kernels tile BOTH dimensions, so their operands
// stream L2 -> LDS for every tile and every intermediate tensor round-trips HBM.  Here a WAVE owns 16 token rows for the
// whole chain and only the weights move:
//   * the wave's current activation rows live in registers as the B operands of v_mfma_f32_16x16x32_f16 (C / 32
//     fragments: lane (row l15, kg) holds channels 32 s + 8 kg .. + 7 of k-step s: 40 VGPRs at C = 320);
//   * a GEMM's fp32 accumulators land in the MFMA D layout, lane (row, kg) holding 4 output rows (channels) of each
//     16-channel fragment.  The weight ROWS are permuted in the pack ("P layout": fragment i, D row 4 kg + e <-> channel
//     32 (i >> 1) + 8 kg + 4 (i & 1) + e), so that fragments 2 s and 2 s + 1 together are exactly the B operand of
//     k-step s of the NEXT GEMM: activations chain from accumulator registers into operands with no data movement,
//     LayerNorm is a per-lane reduction + two cross-lane adds, and global loads / stores are 16 bytes per lane;
//   * the feed-forward's hidden units are processed in groups of 32: GEMM1 (K = C) for 16 hidden + 16 gate columns,
//     twice, gives the GEGLU inputs in the D layout, h = (a_h + b_h) * gelu(a_g + b_g) goes from accumulator registers
//     straight into GEMM2 (K = 32, C / 16 MFMAs into the resident output accumulator): the 4C-wide hidden tensor never
//     exists, not even in LDS;
//   * the only LDS traffic of the loops is the weight stream: all weights of a chain are packed FRAGMENT-MAJOR in
//     consumption order (rcdm_pack_*: every MFMA A operand is one contiguous 1-KiB block in lane order), so a
//     buffer_load ... lds piece is one fragment, LDS is written and read linearly (no swizzle, no bank conflicts), and
//     the whole LDS is one ring of R chunks of 20 fragments that all NW waves of the block consume in lock step (one
//     s_barrier per chunk, counted vmcnt).
// One LDS read per MFMA is the price (the activations cost none): at ten waves per CU the LDS pipe is as loaded as the
// matrix pipe (measured, feed-forward: reads alone 1000 clocks per chunk, MFMAs alone 1000, together 1450).  The variant
// with 48 rows per wave on four waves (one per SIMD, 512 registers, 0.4 x the LDS reads) was built and measured slower
// (147 vs 118 us): a single wave issues one instruction per ~4 clocks, and MFMAs + GEGLU arithmetic + reads do not fit.
//
// Block = NW = 10 waves = 160 rows (the 40960 / 10240 / 2560 / 640 token rows of the UNet are an exact number of blocks;
// 3 + 3 + 2 + 2 waves per SIMD at <= 168 registers).
#include "common.h"
#include "pp_sync.h"
#include <type_traits>

#ifndef RCDM_FF_ABLATE
#define RCDM_FF_ABLATE 0  // debug builds (wrong results, timing only): 1 no DMA after the prefill, 2 no MFMA, 4 no fragment
#endif                    // reads, 8 no barrier in the loop, 16 no epilogue, 32 no GEGLU arithmetic

namespace {

enum { TAIL_FF = 0, TAIL_N1 = 1, TAIL_FFP = 2, TAIL_N3 = 3, TAIL_ATT = 4 };   // FFP: feed-forward, then a C x C projection (+ bias
                                                                               // + residual); ATT: q | k | v, then the temporal attention

struct RowArgs {
  const f16* a_in;     // [M][lda]: stage-A input rows (HAS_A), else the rows the LayerNorm reads (and the FF residual)
  const f16* res;      // [M][ldr]: residual of stage A (A_RES)
  f16* tok;            // [M][ldt]: stage-A output rows (HAS_A); with TAIL_FF also the feed-forward's residual
  f16* out;            // [M][ldo]: tail output (may alias a_in / tok: a block reads and writes only its own rows)
  const f16* wstream;  // [stage-A fragments][tail fragments]
  const float* a_bias; // [C]   (HAS_A)
  const float* ln_g;   // [C]
  const float* ln_b;   // [C]
  const float* pe;     // [frames][C] (LN_PE)
  const float* b1p;    // [8C] packed (TAIL_FF): per (group, pair) 16 hidden biases then their 16 gate biases
  const float* b2;     // [C] (TAIL_FF)
  const f16* z_res;     // [M][ldz] residual of the trailing projection (TAIL_FFP)
  const float* z_bias;  // [C] (TAIL_FFP)
  const float* gn_stat; // [samples][gn_G][2] = (mean, rstd) of the GroupNorm whose apply runs in the prologue (HAS_A && !A_RES), or null
  const float* gn_g;    // [C] GroupNorm weight
  const float* gn_b;    // [C] GroupNorm bias
  int M, lda, ldr, ldt, ldo, ldz;
  int rows_per_frame, frames;
  int gn_G, gn_rows;    // groups; rows per GroupNorm sample (>= the block's rows: a block meets at most two samples)
  float eps;
  float att_scale;      // TAIL_ATT: d_head^-1/2
};

template <int C, int NW, int R, int PD, bool HAS_A, bool A_RES, bool LN_PE, int TAIL>
__global__ __launch_bounds__(NW * 64) void row_chain_kernel(const RowArgs p) {
  constexpr int NK = C / 32;        // k-steps of a K = C GEMM = register fragments of 16 activation rows
  constexpr int NOF = C / 16;       // output fragments (16 channels each) of an N = C GEMM
  constexpr int CHF = 2 * NK;       // fragments per chunk (== NOF)
  constexpr int CHB = CHF * 1024;   // chunk bytes
  constexpr int NG = C / 8;         // feed-forward: groups of 32 hidden units (4C / 32)
  constexpr int NCH_A = HAS_A ? NK : 0;                                   // stage A: NK * NOF fragments
  constexpr bool IS_FF = TAIL == TAIL_FF || TAIL == TAIL_FFP;
  // TAIL_ATT takes its rows FRAME-MAJOR (FM): wave w owns frame w % 5 of pixel group 2 * block + w / 5 (16 consecutive pixels of
  // one (sample, frame) image), so the five frames of a pixel sit in the same lane of five waves of ONE block
  constexpr bool FM = TAIL == TAIL_ATT;
  constexpr int NCH_T = IS_FF ? 3 * NG + (TAIL == TAIL_FFP ? NK : 0) : (FM ? 3 : TAIL) * NK;   // FF 3 chunks per group; GEMM NK per C columns
  constexpr int NCH = NCH_A + NCH_T;
  constexpr int NT = NW * 64;
  constexpr int PPW = CHF / NW;     // DMA pieces per wave and chunk
  static_assert(CHF % NW == 0, "chunk fragments must divide over the waves");
  static_assert(NOF == CHF && CHF % PD == 0 && CHF >= 20 && NOF % 2 == 0, "chunk geometry");
  constexpr int PAR0 = R * CHB;     // parameter region (floats): [a_bias C][gamma C][beta C][pe frames*C][b1p 8C][b2 C | z_bias C]
  constexpr int RS = 2 * C + 16;    // staged output row (bytes)
  static_assert(!IS_FF || NW * 16 * RS <= R * CHB, "epilogue staging exceeds the ring");
  // FM: behind [a_bias][gamma][beta] lies the exchange region X of the attention (one 160-column half of k or v of all NW
  // waves, XW bytes per wave); until the first k half is written there it holds the prologue's tables (pe, GroupNorm)
  constexpr int XOFF = PAR0 + 3 * C * 4, XW = (NK / 2) * 1024;
  static_assert(!FM || (HAS_A && NW == 10 && (5 * C + NW * 2 * C) * 4 <= NW * XW), "frame-major chain geometry");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l15 = lane & 15, kg = lane >> 4;
  int row0_ = blockIdx.x * (NW * 16) + wave * 16, fm_gps = 1, fm_ngrp = 0;
  bool fm_live = true;
  const int fm_f = wave % 5;
  if constexpr (FM) {   // every value here is wave-uniform
    fm_gps = p.rows_per_frame >> 4;                          // pixel groups per image
    fm_ngrp = (p.M / (5 * p.rows_per_frame)) * fm_gps;       // and in all
    const int grp = 2 * blockIdx.x + wave / 5;
    fm_live = grp < fm_ngrp;   // the last block may own one group only: its other five waves run on group 0's rows, store nothing
    const int g2 = fm_live ? grp : 0, b = g2 / fm_gps;
    row0_ = (b * 5 + fm_f) * p.rows_per_frame + 16 * (g2 - b * fm_gps);
  }
  const int row0 = row0_;
  const int row = row0 + l15;
  const bool live = FM ? fm_live : row < p.M;
  const int oG = HAS_A ? C : 0, oB = oG + C, oPE = oB + C, oT = oPE + (LN_PE ? p.frames * C : 0);
  const int oZ = oT + (IS_FF ? 8 * C : 0);              // [b2 C][z_bias C] (TAIL_FFP)
  const int oGN = oZ + (TAIL == TAIL_FFP ? 2 * C : 0);  // [2 samples][scale C | shift C] of the prologue GroupNorm
  const int npar = oGN;

  const __amdgpu_buffer_rsrc_t rsrcW =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.wstream, 0, (unsigned)NCH * CHB, 0x00020000);
  int dma_voff = lane * 16;
  auto issue_chunk = [&](int c, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int piece = wave * PPW + i;
      // per-lane part of the address in the (loop-invariant) voffset, the chunk / piece part in the scalar offset.  The
      // descriptor's range check sees the voffset only: past the end of the stream it is set out of range explicitly
      // (such a piece moves nothing and writes zeros)
      const unsigned voff = c < NCH ? (unsigned)dma_voff : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcW, (__attribute__((address_space(3))) void*)(smem + slot * CHB + piece * 1024),
                                               16, voff, c < NCH ? c * CHB + piece * 1024 : 0, 0, 0);
    }
  };

  // ---- prologue: plain loads first (they are waited for with the DMA prefill still in flight behind them)
  f16x8 xr[NK];    // the input rows; after stage A / the LayerNorm: the B operands of the tail
  f16x8 tk[NK];    // stage A: residual in, new token rows out (P layout = operand layout)
  auto ld16 = [](const f16* q) __attribute__((always_inline)) -> f16x8 { Pack16 t; t.u = *(const uint4*)q; return t.h; };
  auto st16 = [](f16* q, f16x8 v) __attribute__((always_inline)) { Pack16 t; t.h = v; *(uint4*)q = t.u; };
  {
    const f16* xp = p.a_in + (size_t)(live ? row : 0) * p.lda + 8 * kg;
#pragma unroll
    for (int s = 0; s < NK; ++s) xr[s] = ld16(xp + 32 * s);
    if (HAS_A && A_RES) {
      const f16* rp = p.res + (size_t)(live ? row : 0) * p.ldr + 8 * kg;
#pragma unroll
      for (int s = 0; s < NK; ++s) tk[s] = ld16(rp + 32 * s);
    } else {
#pragma unroll
      for (int s = 0; s < NK; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) tk[s][j] = (f16)0.f;
    }
  }
  constexpr int NB4_MAX = ((HAS_A ? C : 0) + 2 * C + (LN_PE ? 8 * C : 0) + (IS_FF ? 8 * C : 0) + (TAIL == TAIL_FFP ? 2 * C : 0)) / 4;  // <= 8 frames
  constexpr int NB4_PER = (NB4_MAX + NT - 1) / NT;
  f32x4 bq[NB4_PER];
#pragma unroll
  for (int i = 0; i < NB4_PER; ++i) {
    const int idx = min(i * NT + t, npar / 4 - 1) * 4;
    const float* src;
    if (HAS_A && idx < oG) src = p.a_bias + idx;
    else if (idx < oB) src = p.ln_g + (idx - oG);
    else if (idx < oPE) src = p.ln_b + (idx - oB);
    else if (LN_PE && idx < oT) src = p.pe + (idx - oPE);
    else if (idx < oZ) src = p.b1p + (idx - oT);
    else if (idx < oZ + C) src = p.b2 + (idx - oZ);
    else src = p.z_bias + (idx - oZ - C);
    bq[i] = *(const f32x4*)src;
  }
  // GroupNorm apply in the prologue (attention.py:328-330 / motion_module.py:162-166: norm, then proj_in): this block's
  // rows belong to at most two samples; thread (j, c) prepares scale / shift of channel c for the block's sample j
  float gn_sc = 0.f, gn_sh = 0.f;
  float fm_sc[FM ? 5 : 1], fm_sh[FM ? 5 : 1];
  constexpr bool CAN_GN = HAS_A && !A_RES;
  static_assert(NT == 2 * C, "one thread per (sample slot, channel)");
  if constexpr (FM && CAN_GN) {
    // frame-major: every wave has its own sample (gn_rows == rows_per_frame: one per image); slot = wave, five slots per thread
    if (p.gn_stat) {
      const int j0 = t >= C ? 1 : 0, ch = t - j0 * C;
      const float ga = p.gn_g[ch], be = p.gn_b[ch];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int j = 2 * i + j0;
        const int smp = (min(2 * (int)blockIdx.x + j / 5, fm_ngrp - 1) / fm_gps) * 5 + j % 5;
        const float* st = p.gn_stat + ((size_t)smp * p.gn_G + ch / (C / p.gn_G)) * 2;
        const float mean = st[0], rstd = st[1];
        fm_sc[i] = rstd * ga;
        fm_sh[i] = __builtin_fmaf(-(mean * rstd), ga, be);
      }
    }
  } else if (CAN_GN && p.gn_stat) {
    const int j = t >= C ? 1 : 0, ch = t - j * C;
    const int nsamp = (p.M + p.gn_rows - 1) / p.gn_rows;
    const int smp = min((int)(blockIdx.x * (NW * 16)) / p.gn_rows + j, nsamp - 1);
    const float* st = p.gn_stat + ((size_t)smp * p.gn_G + ch / (C / p.gn_G)) * 2;
    const float ga = p.gn_g[ch], be = p.gn_b[ch], mean = st[0], rstd = st[1];
    gn_sc = rstd * ga;                  // the same expressions as gn_apply_kernel (norm.hip): same roundings
    gn_sh = __builtin_fmaf(-(mean * rstd), ga, be);
  }
  int cslot = 0;  // slot of the chunk consumed next
#pragma unroll
  for (int c = 0; c < R - 1; ++c) issue_chunk(c, c);
#pragma unroll
  for (int i = 0; i < NB4_PER; ++i) {
    const int idx = i * NT + t;
    if (idx < npar / 4) *(f32x4*)(smem + PAR0 + 16 * idx) = bq[i];
  }
  const float* par = (const float*)(smem + PAR0);
  if constexpr (FM && CAN_GN) {
    if (p.gn_stat) {
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        float* gp = (float*)(smem + PAR0) + oGN + (2 * i + (t >= C ? 1 : 0)) * 2 * C + (t >= C ? t - C : t);
        gp[0] = fm_sc[i];
        gp[C] = fm_sh[i];
      }
    }
  } else if (CAN_GN && p.gn_stat) {
    float* gp = (float*)(smem + PAR0) + oGN + (t >= C ? 2 * C : 0) + (t >= C ? t - C : t);
    gp[0] = gn_sc;
    gp[C] = gn_sh;
  }
  wait_lgkm0();
  wait_vm<(R - 2) * PPW>();  // this wave's pieces of chunk 0 (the compiler's own wait for the plain loads came earlier)
  tick_barrier();            // the parameters and chunk 0 are in LDS

  if (CAN_GN && p.gn_stat) {
    // y = f16(x * scale + shift): the arithmetic of gn_apply_kernel (norm.hip), bit-identical to the separate launch
    const int j = FM ? wave : row0 / p.gn_rows - (int)(blockIdx.x * (NW * 16)) / p.gn_rows;   // wave-uniform: gn_rows % 16 == 0
    const float* gs = par + oGN + (FM ? j * 2 * C : j > 0 ? 2 * C : 0) + 8 * kg;
#pragma unroll
    for (int s = 0; s < NK; ++s) {
      const f32x4 c0 = *(const f32x4*)(gs + 32 * s), c1 = *(const f32x4*)(gs + 32 * s + 4);
      const f32x4 h0 = *(const f32x4*)(gs + C + 32 * s), h1 = *(const f32x4*)(gs + C + 32 * s + 4);
      f16x8 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // fp32 result first, then its f16 rounding, as the separate launch does: left alone, the compiler merges the two
        // into v_fma_mixlo_f16 (ONE rounding) and one element in ~20 000 comes out an ulp away from gn_apply's
        float f0 = __builtin_fmaf((float)xr[s][e], c0[e], h0[e]), f1 = __builtin_fmaf((float)xr[s][4 + e], c1[e], h1[e]);
        asm volatile("" : "+v"(f0), "+v"(f1));
        y[e] = (f16)f0;
        y[4 + e] = (f16)f1;
      }
      xr[s] = y;
    }
  }

  // ---- the weight stream is ONE software pipeline over all NCH * CHF fragments: the read of fragment f + PD is issued
  // with the MFMA of fragment f, across chunk boundaries (no drain at the barriers).  Chunk hand-over at the top of chunk
  // c: this wave's pieces of chunk c + 1 have landed (counted vmcnt: loads only — stores complete out of order with
  // loads, so every wait also covers the few stores issued since the previous one, which is why stores are issued right
  // AFTER a hand-over); the barrier makes everybody's pieces visible — so reads may run ahead into chunk c + 1 during
  // chunk c — and says everybody is done with chunk c - 1, whose slot the issue refills with chunk c + R - 1.  Past the
  // end of the stream the refill pieces are out of range: they move nothing, write zeros into slots nobody reads again,
  // and keep the counted wait the same for every chunk.
  int c = 0;
  // the one lane-dependent value the loops keep: DMA voffset and LDS read base.  Opaque, and the epilogue re-derives its
  // lane indices from it, so that no second copy of the thread id has to survive the loops
  int lane16 = lane * 16;
  asm volatile("" : "+v"(lane16));
  dma_voff = lane16;
  auto rd = [&](const char* q) __attribute__((always_inline)) -> f16x8 {
    if (RCDM_FF_ABLATE & 4) { f16x8 z; for (int e = 0; e < 8; ++e) z[e] = (f16)(float)lane; return z; }
    return *(const f16x8*)q;
  };
  auto mm = [&](f16x8 a, f16x8 b, f32x4 acc) __attribute__((always_inline)) -> f32x4 {
    if (RCDM_FF_ABLATE & 2) { asm volatile("" ::"v"(a), "v"(b)); return acc; }
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  };
  f16x8 fr[PD];
#pragma unroll
  for (int i = 0; i < PD; ++i) fr[i] = rd(smem + lane16 + i * 1024);
  // one chunk: CHF steps of [MFMA on fragment i | read of fragment i + PD | slice i of interleaved VALU work], each step
  // its own scheduling region (sched_barrier): the interleave is what the source says.  post_sync: stores issued right
  // after the hand-over.
  auto run_chunk = [&](auto&& mfma_i, auto&& slice_i, auto&& post_sync) __attribute__((always_inline)) {
    wait_vm<(R - 3) * PPW>();
    if (!(RCDM_FF_ABLATE & 8)) tick_barrier();
    if (!(RCDM_FF_ABLATE & 1)) issue_chunk(c + R - 1, cslot == 0 ? R - 1 : cslot - 1);
    post_sync();
    const char* sb = smem + cslot * CHB + lane16;
    const char* sn = smem + (cslot == R - 1 ? 0 : cslot + 1) * CHB + lane16;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < CHF; ++i) {
      const f16x8 cur = fr[i % PD];
      mfma_i(i, cur);
      fr[i % PD] = rd(i + PD < CHF ? sb + (i + PD) * 1024 : sn + (i + PD - CHF) * 1024);
      slice_i(i);
      __builtin_amdgcn_sched_barrier(0);
    }
    ++c;
    cslot = cslot == R - 1 ? 0 : cslot + 1;
  };
  auto nothing = [&](int) __attribute__((always_inline)) {};
  auto no_stores = [&]() __attribute__((always_inline)) {};
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

  // ---- stage A: tok = a_in W_a^T + b_a (+ res), two halves of NOF / 2 output fragments (fragment order of the stream:
  // half, k-step, fragment), accumulated in 40 registers and folded into tk (f16, P layout) after each half
  if constexpr (HAS_A) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 acc[NOF / 2];
#pragma unroll
      for (int cc = 0; cc < NK / 2; ++cc)
        run_chunk([&](int i, f16x8 w) __attribute__((always_inline)) {
          const int s = 2 * cc + i / (NOF / 2), fi = i % (NOF / 2);
          acc[fi] = mm(w, xr[s], s == 0 ? z4 : acc[fi]);
        }, nothing, no_stores);
#pragma unroll
      for (int fi = 0; fi < NOF / 2; ++fi) {
        const int i = h * (NOF / 2) + fi, s = i >> 1, sub = i & 1;
        const f32x4 b = *(const f32x4*)(par + 32 * s + 8 * kg + 4 * sub);
#pragma unroll
        for (int e = 0; e < 4; ++e) tk[s][4 * sub + e] = (f16)(acc[fi][e] + b[e] + (float)tk[s][4 * sub + e]);
      }
    }
  }
  // stage A's token rows go out at once (plain stores: the next hand-over's counted wait also covers them — one short
  // stall per launch; deferring them kept 40 registers alive into the tail and spilled)
  if (HAS_A && live) {
    f16* tp = p.tok + (size_t)row * p.ldt + 8 * kg;
#pragma unroll
    for (int s = 0; s < NK; ++s) st16(tp + 32 * s, tk[s]);
  }

  // ---- LayerNorm of the token rows (stage A's output, or the input rows) -> xr = the tail's B operands.  Two passes
  // over registers (mean, then squared deviations), a row's 4 lanes combined with two cross-lane adds
  {
    f16x8 (&src)[NK] = HAS_A ? tk : xr;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)src[k][j];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = (float)src[k][j] - mean;
        q += d * d;
      }
    q += __shfl_xor(q, 16, 64);
    q += __shfl_xor(q, 32, 64);
    const float rstd = rsqrtf(q * (1.0f / C) + p.eps);
    const float* pep = !LN_PE ? par : FM ? par + oPE + fm_f * C : par + oPE + (((live ? row : 0) / p.rows_per_frame) % p.frames) * C;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int ch = 32 * k + 8 * kg;
      const f32x4 g0 = *(const f32x4*)(par + oG + ch), g1 = *(const f32x4*)(par + oG + ch + 4);
      f32x4 b0 = *(const f32x4*)(par + oB + ch), b1 = *(const f32x4*)(par + oB + ch + 4);
      if (LN_PE) {
        b0 += *(const f32x4*)(pep + ch);
        b1 += *(const f32x4*)(pep + ch + 4);
      }
      f16x8 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        y[j] = (f16)(((float)src[k][j] - mean) * rstd * g0[j] + b0[j]);
        y[4 + j] = (f16)(((float)src[k][4 + j] - mean) * rstd * g1[j] + b1[j]);
      }
      xr[k] = y;
    }
  }

  // ---- a GEMM with N = NGRP * C / 2 whose B operands are xr, in groups of NOF / 2 output fragments (NK / 2 chunks each); a
  // group's f16 results are stored 16 bytes per lane right after the next hand-over.  ZADD (the trailing projection of
  // TAIL_FFP): + z_bias, rounded, + z_res, rounded — nn.Linear, then the block's residual add (attention.py:352-363,
  // motion_module.py:170-176); the residual rows are requested at the group's first hand-over
  auto gemm_groups = [&](auto ngrp_c, auto zadd_c) __attribute__((always_inline)) {
    constexpr int NGRP = decltype(ngrp_c)::value;
    constexpr bool ZADD = decltype(zadd_c)::value;
    f16x8 pend[NOF / 4], zr[ZADD ? NOF / 4 : 1];
    int pend_col = 0;
    auto store_pend = [&]() __attribute__((always_inline)) {
      if (live) {
        f16* op = p.out + (size_t)row * p.ldo + pend_col + 8 * kg;
#pragma unroll
        for (int m = 0; m < NOF / 4; ++m) st16(op + 32 * m, pend[m]);
      }
    };
    for (int grp = 0; grp < NGRP; ++grp) {
      f32x4 acc[NOF / 2];
#pragma unroll
      for (int cc = 0; cc < NK / 2; ++cc) {
        auto mf = [&](int i, f16x8 w) __attribute__((always_inline)) {
          const int s = 2 * cc + i / (NOF / 2), fi = i % (NOF / 2);
          acc[fi] = mm(w, xr[s], s == 0 ? z4 : acc[fi]);
        };
        if (cc == 0)
          run_chunk(mf, nothing, [&]() __attribute__((always_inline)) {
            if (grp > 0) store_pend();
            if constexpr (ZADD) {
              const f16* zp = p.z_res + (size_t)(live ? row : 0) * p.ldz + grp * (C / 2) + 8 * kg;
#pragma unroll
              for (int m = 0; m < NOF / 4; ++m) zr[m] = ld16(zp + 32 * m);
            }
          });
        else
          run_chunk(mf, nothing, no_stores);
      }
#pragma unroll
      for (int m = 0; m < NOF / 4; ++m) {
        if constexpr (ZADD) {
          const float* bz = par + oZ + C + grp * (C / 2) + 32 * m + 8 * kg;
          const f32x4 b0 = *(const f32x4*)bz, b1 = *(const f32x4*)(bz + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            pend[m][e] = (f16)((float)(f16)(acc[2 * m][e] + b0[e]) + (float)zr[m][e]);
            pend[m][4 + e] = (f16)((float)(f16)(acc[2 * m + 1][e] + b1[e]) + (float)zr[m][4 + e]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            pend[m][e] = (f16)acc[2 * m][e];
            pend[m][4 + e] = (f16)acc[2 * m + 1][e];
          }
        }
      }
      pend_col = grp * (C / 2);
    }
    wait_lgkm0();
    wait_vm<0>();
    store_pend();
  };

  if constexpr (FM) {
    // ---- q | k | v, then softmax(q k^T * scale) v over the five frames of every pixel (TemporalSelfAttention,
    // motion_module.py:299-302 -> CrossAttention._attention), as rcdm_temporal_attn computes it from the stored q | k | v.
    // The stream brings the six 160-column groups as q0 k0 v0 q1 k1 v1 (0 / 1: heads 0-3 / 4-7), so that one half of the
    // heads is finished while the other half's GEMMs run: a group's f16 results (the bits the tail-3 chain stores) stay in
    // registers in the operand layout — lane (l15, kg) holds channels 32 m + 8 kg .. + 7 of the half, m < 5 — and k, then
    // v, of all ten waves pass through X, each wave writing and reading whole lane-linear 1-KiB pieces (conflict-free
    // b128 accesses).  A piece of 8 channels belongs to head (4 m + kg) / 5: the partial dots of a lane are summed per
    // head, then over the row's four lanes.  Time line of a half (chunks of its v group, then of the next q group):
    //   v.0 hand-over: k -> X | v.1-3: 25 partial dots (frame, m) | v.4: cross-lane sums | (next q.0: softmax)
    //   q.0 hand-over: v -> X | q.1-3: 25 (m, frame) products -> o | k.0 hand-over: o -> memory
    // Every write of X follows a barrier behind the last read of what it replaces, and is itself followed by a barrier
    // before its first read (the in-order LDS counter has passed it by then: later fragment reads were waited for).
    constexpr int HG = NK / 2;
    char* const X = smem + XOFF;
    const int kgq = lane16 >> 8, xme = wave * XW + lane16, xgrp = (wave / 5) * 5 * XW + lane16;
    const bool c1 = kgq == 0, c2 = kgq <= 1, c3 = kgq <= 2;   // piece m = 1 / 2 / 3 belongs to head m - 1 (else to head m)
    f16x8 qh[HG], pend[HG], oh[HG];
    f32x4 acc[NOF / 2];
    float sc[4][5], o8[8];
    auto round_to = [&](f16x8 (&dst)[HG]) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < HG; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dst[m][e] = (f16)acc[2 * m][e];
          dst[m][4 + e] = (f16)acc[2 * m + 1][e];
        }
    };
    auto xput = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < HG; ++m) *(f16x8*)(X + xme + m * 1024) = pend[m];
    };
    auto xget = [&](int fp, int m) __attribute__((always_inline)) -> f16x8 { return *(const f16x8*)(X + xgrp + fp * XW + m * 1024); };
    auto score_item = [&](int fp, int m) __attribute__((always_inline)) {
      const f16x8 kv = xget(fp, m);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e += 2)   // v_dot2_f32_f16: exact products, fp32 sums; q stays packed (no 40 converted copies)
        d = __builtin_amdgcn_fdot2(f16x2{qh[m][e], qh[m][e + 1]}, f16x2{kv[e], kv[e + 1]}, d, false);
      // (the empty asm statements here and below pin each item's arithmetic to its slice, as in the GEGLU slices)
      if (m == 0) {
        sc[0][fp] = d; sc[1][fp] = 0.f; sc[2][fp] = 0.f; sc[3][fp] = 0.f;
        asm volatile("" : "+v"(sc[0][fp]));
      } else if (m == 4) {
        sc[3][fp] += d;
        asm volatile("" : "+v"(sc[3][fp]));
      } else {
        const float lo = (m == 1 ? c1 : m == 2 ? c2 : c3) ? d : 0.f;
        sc[m - 1][fp] += lo;
        sc[m][fp] += d - lo;
        asm volatile("" : "+v"(sc[m - 1][fp]), "+v"(sc[m][fp]));
      }
    };
    auto reduce_item = [&](int h, int fp) __attribute__((always_inline)) {
      float v = sc[h][fp];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      asm volatile("" : "+v"(v));   // the sum here, not sunk to its use with both addends kept alive
      sc[h][fp] = v;
    };
    // the arithmetic of temporal_attn_kernel (attn.hip): scale, max, __expf, sum, p_j = e_j * rcp(sum)
    auto softmax_head = [&](int h) __attribute__((always_inline)) {
      float mx = sc[h][0] * p.att_scale;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        sc[h][j] *= p.att_scale;
        mx = fmaxf(mx, sc[h][j]);
      }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        sc[h][j] = __expf(sc[h][j] - mx);
        sum += sc[h][j];
      }
      const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
      for (int j = 0; j < 5; ++j) sc[h][j] *= inv;
      asm volatile("" : "+v"(sc[h][0]), "+v"(sc[h][1]), "+v"(sc[h][2]), "+v"(sc[h][3]), "+v"(sc[h][4]));
    };
    auto pv_item = [&](int m, int fp) __attribute__((always_inline)) {
      const f16x8 vv = xget(fp, m);
      const float pj = m == 0 ? sc[0][fp] : m == 4 ? sc[3][fp] : (m == 1 ? c1 : m == 2 ? c2 : c3) ? sc[m - 1][fp] : sc[m][fp];
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = __builtin_fmaf(pj, (float)vv[e], fp == 0 ? 0.f : o8[e]);
      if (fp == 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) oh[m][e] = (f16)o8[e];
        asm volatile("" : "+v"(oh[m]));
      } else {
        asm volatile("" : "+v"(o8[0]), "+v"(o8[1]), "+v"(o8[2]), "+v"(o8[3]), "+v"(o8[4]), "+v"(o8[5]), "+v"(o8[6]), "+v"(o8[7]));
      }
    };
    auto store_o = [&](int half) __attribute__((always_inline)) {
      if (live) {
        f16* op = p.out + (size_t)row * p.ldo + half * (C / 2) + 8 * kgq;
#pragma unroll
        for (int m = 0; m < HG; ++m) st16(op + 32 * m, oh[m]);
      }
    };
    // one 160-column group: HH = half, GRP = 0 / 1 / 2 for q / k / v (template constants: what rides in a chunk is decided here)
    auto group = [&](auto hh_c, auto grp_c) __attribute__((always_inline)) {
      constexpr int hh = decltype(hh_c)::value, grp = decltype(grp_c)::value;
#pragma unroll
      for (int cc = 0; cc < HG; ++cc)
        run_chunk(
            [&](int i, f16x8 w) __attribute__((always_inline)) {
              const int s = 2 * cc + i / (NOF / 2), fi = i % (NOF / 2);
              acc[fi] = mm(w, xr[s], s == 0 ? z4 : acc[fi]);
            },
            [&](int i) __attribute__((always_inline)) {
              if constexpr (grp == 2) {   // this half's scores, under its v GEMM
                if (cc >= 1 && cc <= 3 && i < (cc == 3 ? 5 : 10)) score_item(2 * (cc - 1) + i / 5, i % 5);
                if (cc == 4) reduce_item(i / 5, i % 5);
              } else if constexpr (grp == 0 && hh == 1) {   // the first half's softmax and output, under the second half's q GEMM
                if (cc == 0 && i % 5 == 2) softmax_head(i / 5);
                if (cc >= 1 && cc <= 3 && i < (cc == 3 ? 5 : 10)) pv_item(2 * (cc - 1) + i / 5, i % 5);
              }
            },
            [&]() __attribute__((always_inline)) {
              if (cc == 0 && (grp == 2 || (grp == 0 && hh == 1))) xput();
              if (cc == 0 && grp == 1 && hh == 1) store_o(0);
            });
      if constexpr (grp == 0) round_to(qh); else round_to(pend);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    group(I0{}, I0{}); group(I0{}, I1{}); group(I0{}, I2{});
    group(I1{}, I0{}); group(I1{}, I1{}); group(I1{}, I2{});
    // the second half's v: the stream has ended, nothing is left to hide under
#pragma unroll
    for (int h = 0; h < 4; ++h) softmax_head(h);
    wait_lgkm0();
    wait_vm<0>();    // the zero-fill pieces issued past the end of the stream (and the stores so far)
    tick_barrier();  // every wave is done reading k
    xput();
    wait_lgkm0();
    tick_barrier();
#pragma unroll
    for (int m = 0; m < HG; ++m)
#pragma unroll
      for (int fp = 0; fp < 5; ++fp) pv_item(m, fp);
    store_o(1);
    return;
  } else if constexpr (!IS_FF) {
    gemm_groups(std::integral_constant<int, 2 * TAIL>{}, std::false_type{});
    return;
  } else {
    // ---- tail feed-forward.  Chunk order in the stream: A_0, then per group g: B_g, A_{g+1}, C_g  (A / B = GEMM1 of the
    // first / second 16 hidden + 16 gate columns of the group, C = GEMM2).  The GEGLU arithmetic of a GEMM1 chunk's
    // accumulators runs UNDER the next chunk's MFMAs (every wave of the block is in the same chunk, so VALU work placed
    // between chunks would leave all four matrix pipes idle at once), cut into CHF slices of 3-4 plain fp32 VALU
    // instructions (packed fp32 issues slower next to MFMAs): gelu(x) = max(x, 0) - |x| q(|x|),
    // q = poly(t) exp(-x^2 / 2) / 2, t = 1 / (1 + p |x| / sqrt 2)  (Abramowitz & Stegun 7.1.26, common.h gelu2); value e
    // uses slices 5 e .. 5 e + 4.  The empty asm statements pin every slice where the source puts it: without them the
    // optimizer sinks the whole (pure) computation to its first use, after the chunk's MFMAs.
    f32x4 oacc[NOF];
#pragma unroll
    for (int i = 0; i < NOF; ++i) oacc[i] = z4;
    struct GegluState { float bh, x, t, pl, ex; };
    auto geglu_slice = [&](int i, GegluState& st, const f32x4& ah, const f32x4& ag, int gp, f16* dst) __attribute__((always_inline)) {
      const int e = i / 5, stage = i - 5 * e;
      if (e >= 4) return;
      const float* bp = (const float*)(smem + PAR0 + (lane16 >> 8) * 16) + oT + gp * 32 + e;  // this value's two biases
      if (RCDM_FF_ABLATE & 32) {
        if (stage == 4) dst[e] = (f16)((ah[e] + bp[0]) * (ag[e] + bp[16]));
        return;
      }
      if (stage == 0) {
        st.x = ag[e] + bp[16];
        st.bh = bp[0];
        st.t = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(st.x), 0.2316418882f, 1.0f));
        st.ex = st.x * st.x;
        asm volatile("" : "+v"(st.t), "+v"(st.ex));
      } else if (stage == 1) {
        st.ex = __builtin_amdgcn_exp2f(st.ex * -0.72134752044f);
        st.pl = __builtin_fmaf(st.t, 0.5307027145f, -0.7265760135f);
        st.pl = __builtin_fmaf(st.pl, st.t, 0.7107068705f);
        asm volatile("" : "+v"(st.pl), "+v"(st.ex));
      } else if (stage == 2) {
        st.pl = __builtin_fmaf(st.pl, st.t, -0.142248368f);
        st.pl = __builtin_fmaf(st.pl, st.t, 0.127414796f);
        st.t = st.pl * st.t;
        asm volatile("" : "+v"(st.t));
      } else if (stage == 3) {
        st.t = st.t * st.ex;
        st.pl = __builtin_fmaxf(st.x, 0.0f);
        st.t = __builtin_fmaf(-__builtin_fabsf(st.x), st.t, st.pl);
        asm volatile("" : "+v"(st.t));
      } else {
        float hv = (ah[e] + st.bh) * st.t;
        asm volatile("" : "+v"(hv));
        dst[e] = (f16)hv;
      }
    };
    // two accumulator sets: A chunks accumulate into (ahA, agA), read by the GEGLU that runs under the following B chunk;
    // B chunks into (ahB, agB), read under the following A chunk.  The first MFMA of a chunk takes C = 0.
    f32x4 ahA = z4, agA = z4, ahB = z4, agB = z4;
    union { f16x8 v; f16 e[8]; } hb;
    GegluState gs;
    auto g1A = [&](int i, f16x8 w) __attribute__((always_inline)) {
      if (i & 1) agA = mm(w, xr[i >> 1], i < 2 ? z4 : agA); else ahA = mm(w, xr[i >> 1], i < 2 ? z4 : ahA);
    };
    auto g1B = [&](int i, f16x8 w) __attribute__((always_inline)) {
      if (i & 1) agB = mm(w, xr[i >> 1], i < 2 ? z4 : agB); else ahB = mm(w, xr[i >> 1], i < 2 ? z4 : ahB);
    };
    auto g2 = [&](int i, f16x8 w) __attribute__((always_inline)) { oacc[i] = mm(w, hb.v, oacc[i]); };
    int g = 0;
    auto sliceA = [&](int i) __attribute__((always_inline)) { geglu_slice(i, gs, ahA, agA, 2 * g, hb.e); };
    auto sliceB = [&](int i) __attribute__((always_inline)) { geglu_slice(i, gs, ahB, agB, 2 * g + 1, hb.e + 4); };
    run_chunk(g1A, nothing, no_stores);  // A_0
    for (; g < NG - 1; ++g) {
      run_chunk(g1B, sliceA, no_stores);   // B_g under GEGLU(A_g)
      run_chunk(g1A, sliceB, no_stores);   // A_{g+1} under GEGLU(B_g)
      run_chunk(g2, nothing, no_stores);   // C_g
    }
    run_chunk(g1B, sliceA, no_stores);
#pragma unroll
    for (int i = 0; i < CHF; ++i) sliceB(i);
    if constexpr (TAIL == TAIL_FFP) {
      // the feed-forward's residual rows (this wave's own stage-A stores: read back past the vector L1) are requested at
      // the last chunk's hand-over; then x2 = f16(f16(acc) + b2 + tok) — the roundings of the staged epilogue below — is, in
      // the P layout, the B operand of the trailing projection, which runs on as two more output groups of the stream
      f16x8 tkr[NK];
      run_chunk(g2, nothing, [&]() __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rsrcT = __builtin_amdgcn_make_buffer_rsrc((void*)p.tok, 0, 0x7FFFFFFF, 0x00020000);
        const int off = ((live ? row : 0) * p.ldt + 8 * kg) * 2;
#pragma unroll
        for (int s = 0; s < NK; ++s) {
          Pack16 t;
          t.v = __builtin_amdgcn_raw_buffer_load_b128(rsrcT, off + 64 * s, 0, 16);
          tkr[s] = t.h;
        }
      });
#pragma unroll
      for (int s = 0; s < NK; ++s) {
        const float* b2p = par + oZ + 32 * s + 8 * kg;
        const f32x4 b0 = *(const f32x4*)b2p, b1 = *(const f32x4*)(b2p + 4);
        f16x8 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          y[e] = (f16)((float)(f16)oacc[2 * s][e] + b0[e] + (float)tkr[s][e]);
          y[4 + e] = (f16)((float)(f16)oacc[2 * s + 1][e] + b1[e] + (float)tkr[s][4 + e]);
        }
        xr[s] = y;
      }
      gemm_groups(std::integral_constant<int, 2>{}, std::true_type{});
      return;
    }
    run_chunk(g2, nothing, no_stores);  // C of the last group
    wait_lgkm0();
    wait_vm<0>();    // the zero-fill pieces issued past the end of the stream (and stage A's stores)
    tick_barrier();  // every wave is done reading the ring and nothing is in flight into it

    // ---- epilogue: accumulators -> f16 rows in this wave's private staging region -> coalesced 16-byte pass with
    // bias + residual (the same two roundings as the unfused rcdm_gemm epilogue).  The residual rows were written by
    // this block's stage A when there is one: read back past the vector L1 (sc1)
    if (RCDM_FF_ABLATE & 16) {
      float sacc = 0.f;
#pragma unroll
      for (int i = 0; i < NOF; ++i) sacc += oacc[i][0] + oacc[i][1] + oacc[i][2] + oacc[i][3];
      if (sacc == 1.2345678e33f) p.out[0] = (f16)sacc;
      return;
    }
    char* st = smem + wave * 16 * RS;
    const int lane_e = lane16 >> 4, l15_e = lane_e & 15, kg_e = lane_e >> 4;
#pragma unroll
    for (int i = 0; i < NOF; ++i) {
      union { f16 h[4]; uint2 u; } pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk.h[e] = (f16)oacc[i][e];
      *(uint2*)(st + l15_e * RS + (16 * i + 4 * kg_e) * 2) = pk.u;
    }
    wait_lgkm0();
    const f16* rbase = HAS_A ? p.tok : p.a_in;
    const int ldres = HAS_A ? p.ldt : p.lda;
    const __amdgpu_buffer_rsrc_t rsrcR = __builtin_amdgcn_make_buffer_rsrc((void*)rbase, 0, 0x7FFFFFFF, 0x00020000);
    constexpr int CPR = C / 8, ITEMS = 16 * CPR, NIT = (ITEMS + 63) / 64;
    constexpr int U = 5;  // residual loads in flight per lane
    static_assert(NIT % U == 0, "epilogue batches");
    for (int it0 = 0; it0 < NIT; it0 += U) {
      Pack16 rr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = min((it0 + u) * 64 + lane_e, ITEMS - 1);
        const int r = idx / CPR, c8 = idx - r * CPR;
        const int m = min(row0 + r, p.M - 1);
        rr[u].v = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (m * ldres + c8 * 8) * 2, 0, HAS_A ? 16 : 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = (it0 + u) * 64 + lane_e;
        const int r = idx / CPR, c8 = idx - r * CPR;
        const int m = row0 + r;
        if (idx < ITEMS && m < p.M) {
          Pack16 v, o;
          v.u = *(const uint4*)(st + r * RS + c8 * 16);
          const f32x4 a0 = *(const f32x4*)(p.b2 + c8 * 8), a1 = *(const f32x4*)(p.b2 + c8 * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o.e[e] = (f16)((float)v.e[e] + a0[e] + (float)rr[u].e[e]);
            o.e[4 + e] = (f16)((float)v.e[4 + e] + a1[e] + (float)rr[u].e[4 + e]);
          }
          *(uint4*)(p.out + (size_t)m * p.ldo + c8 * 8) = o.u;
        }
      }
    }
  }
}

// ---- weight packing: fp32 reference layouts -> the fragment-major streams the kernel consumes ------------------------
// One fragment = 16 output rows x 32 k values as the v_mfma_f32_16x16x32_f16 A operand: lane L = (row l15 = L & 15,
// k-group kq = L >> 4) holds k = 32 s + 8 kq .. + 7.

// N = C GEMM blocks in the P layout (stage A, tail GEMM): n_blocks blocks of C output channels; fragment order per block:
// half (NOF / 2 fragments), k-step, fragment.  Fragment i of a block, D row r  <->  channel 32 (i >> 1) + 8 (r >> 2) +
// 4 (i & 1) + (r & 3) of the block.
// by_half (n_blocks = 3, TAIL_ATT): the six 160-column groups leave in the order q0 k0 v0 q1 k1 v1 instead of q0 q1 k0 k1 v0 v1.
__global__ void pack_pgemm_kernel(const float* __restrict__ w, int C, int n_blocks, f16* __restrict__ ws, int by_half) {
  const int NK = C / 32, NOF = C / 16, HF = NOF / 2;
  const size_t per_block = (size_t)NOF * NK * 512, total = per_block * n_blocks;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 7), L = (int)((idx >> 3) & 63);
    const size_t fq = idx >> 9;
    int blk = (int)(fq / (NOF * NK));
    const int f = (int)(fq % (NOF * NK));
    int h = f / (HF * NK);
    const int rem = f % (HF * NK), s = rem / HF, fi = rem % HF;
    if (by_half) {
      const int gs = 2 * blk + h;   // group of the stream -> (matrix, half)
      blk = gs % 3;
      h = gs / 3;
    }
    const int i = h * HF + fi, r = L & 15, kq = L >> 4;
    const int n = blk * C + 32 * (i >> 1) + 8 * (r >> 2) + 4 * (i & 1) + (r & 3);
    ws[idx] = (f16)w[(size_t)n * C + 32 * s + 8 * kq + j];
  }
}

// feed-forward: fp32 [8C][C] / [8C] / [C][4C] -> chunks A_0, then per group g: B_g, A_{g+1} (absent for the last group),
// C_g; the k-slots of the GEMM2 fragments follow the D layout of the GEGLU values
// pperm: the rows of GEMM2 in the P layout (its accumulators become the operand of a trailing projection, TAIL_FFP)
__global__ void pack_ff_stream_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                      int C, f16* __restrict__ ws, float* __restrict__ b1p, int pperm) {
  const int NK = C / 32, CHF = 2 * NK;
  const size_t total = (size_t)12 * C * C;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(idx & 7), L = (int)((idx >> 3) & 63);
    const size_t fr = idx >> 9;
    const int f = (int)(fr % CHF), c = (int)(fr / CHF);
    int g, part;  // part 0 = A (first 16 hidden + gate columns of the group), 1 = B (second 16), 2 = C (GEMM2)
    if (c == 0) { g = 0; part = 0; }
    else {
      const int NGr = C / 8, q = c - 1;
      if (q < 3 * (NGr - 1)) {
        const int gg = q / 3, r = q - 3 * gg;
        if (r == 0) { g = gg; part = 1; } else if (r == 1) { g = gg + 1; part = 0; } else { g = gg; part = 2; }
      } else {
        g = NGr - 1; part = (q - 3 * (NGr - 1)) == 0 ? 1 : 2;
      }
    }
    const int l15 = L & 15, kg = L >> 4;
    float v;
    if (part < 2) {
      const int s = f >> 1, gate = f & 1;
      const int hr = 32 * g + 16 * part + l15;
      v = w1[(size_t)(gate ? 4 * C + hr : hr) * C + 32 * s + 8 * kg + j];
    } else {
      const int hid = 32 * g + (j < 4 ? 4 * kg + j : 16 + 4 * kg + (j - 4));
      const int n = pperm ? 32 * (f >> 1) + 8 * (l15 >> 2) + 4 * (f & 1) + (l15 & 3) : 16 * f + l15;
      v = w2[(size_t)n * (4 * C) + hid];
    }
    ws[idx] = (f16)v;
    if (idx < (size_t)8 * C) {  // packed bias: [(g, pair)][16 hidden | 16 gate]
      const int q = (int)idx, gp = q >> 5, l = q & 31;
      const int hr = 16 * gp + (l & 15);
      b1p[q] = b1[l < 16 ? hr : 4 * C + hr];
    }
  }
}

template <bool HAS_A, bool A_RES, bool LN_PE, int TAIL>
int launch_chain(const RowArgs& a, hipStream_t stream) {
  constexpr int C = 320, NW = 10, PD = 2;
  constexpr int R = TAIL == TAIL_ATT ? 5 : 7;   // the attention's exchange region takes two chunks' worth of LDS from the ring
  constexpr int CHB = 2 * (C / 32) * 1024;
  const int npar = (HAS_A ? C : 0) + 2 * C + (LN_PE ? a.frames * C : 0) + (TAIL == TAIL_FF || TAIL == TAIL_FFP ? 8 * C : 0) +
                   (TAIL == TAIL_FFP ? 2 * C : 0);
  const int lds = TAIL == TAIL_ATT ? R * CHB + 3 * C * 4 + NW * (C / 64) * 1024 : R * CHB + (npar + (a.gn_stat ? 4 * C : 0)) * 4;
  if (lds > 160 * 1024) return RCDM_ESHAPE;
  static bool attr_set[64] = {};
  if (rcdm_first_on_device(attr_set) &&
      hipFuncSetAttribute((const void*)row_chain_kernel<C, NW, R, PD, HAS_A, A_RES, LN_PE, TAIL>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return RCDM_ELAUNCH;
  const int nblocks = (a.M + NW * 16 - 1) / (NW * 16);
  hipLaunchKernelGGL((row_chain_kernel<C, NW, R, PD, HAS_A, A_RES, LN_PE, TAIL>), dim3(nblocks), dim3(NW * 64), lds, stream, a);
  return rcdm_check_launch();
}

inline unsigned grid_for(size_t n) {
  size_t g = (n + 255) / 256;
  return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// preconditions the kernels do not check themselves: per-column fp32 vectors are fetched as aligned float4, and row offsets
// are 32-bit byte offsets into a 2-GB buffer resource
inline bool misaligned16(const void* p) { return p && ((uintptr_t)p & 15); }
inline bool rows_overflow(int M, int ld) { return (size_t)M * (size_t)ld * 2 >= 0x7FFFFFFFull; }

}  // namespace

extern "C" {

int rcdm_ff_fused_supported(int32_t C) { return C == 320 ? 1 : 0; }
int rcdm_rowchain_supported(int32_t C) { return C == 320 ? 1 : 0; }

// whether rcdm_rowchain has a launch for this configuration: width, tail, frames of the positional-encoding table (0 = no
// pe).  pe rides with tail 1 / 3 only (with the feed-forward tails the parameter region would not fit the 160 KB of LDS)
// and for at most 8 frames.
int rcdm_rowchain_config_supported(int32_t C, int32_t tail, int32_t pe_frames) {
  if (C != 320 || tail < 0 || tail > 4) return 0;
  if (pe_frames < 0 || pe_frames > 8) return 0;
  if (tail == 4 && pe_frames != 0 && pe_frames != 5) return 0;   // the attention tail: five frames (a block = 2 x 5 waves)
  if (pe_frames > 0 && (tail == 0 || tail == 2)) return 0;
  return 1;
}

size_t rcdm_ff_stream_bytes(int32_t C) { return C > 0 ? (size_t)24 * C * C : 0; }

size_t rcdm_rowchain_stream_bytes(int32_t C, int32_t tail) {
  if (C <= 0 || tail < 0 || tail > 4) return 0;
  return (size_t)2 * C * C * (1 + (tail == 0 ? 12 : tail == 2 ? 13 : tail == 4 ? 3 : tail));
}

int rcdm_pack_ff_stream(const float* w1, const float* b1, const float* w2, int32_t C, void* wstream, float* b1_packed,
                        void* stream) {
  if (!w1 || !b1 || !w2 || !wstream || !b1_packed || C <= 0) return RCDM_EINVAL;
  if (C % 32) return RCDM_ESHAPE;
  hipLaunchKernelGGL(pack_ff_stream_kernel, dim3(grid_for((size_t)12 * C * C)), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, C,
                     (f16*)wstream, b1_packed, 0);
  return rcdm_check_launch();
}

int rcdm_pack_rowchain(const float* wa, int32_t C, int32_t tail, const float* wt, const float* w1, const float* b1,
                       const float* w2, void* wstream, float* b1_packed, void* stream) {
  if (!wa || !wstream || C <= 0) return RCDM_EINVAL;
  if (C % 32 || tail < 0 || tail > 4) return RCDM_ESHAPE;
  const bool ff = tail == 0 || tail == 2;
  if ((ff && (!w1 || !b1 || !w2 || !b1_packed)) || (tail != 0 && !wt)) return RCDM_EINVAL;
  f16* ws = (f16*)wstream;
  hipLaunchKernelGGL(pack_pgemm_kernel, dim3(grid_for((size_t)C * C)), dim3(256), 0, (hipStream_t)stream, wa, C, 1, ws, 0);
  ws += (size_t)C * C;
  if (ff) {
    hipLaunchKernelGGL(pack_ff_stream_kernel, dim3(grid_for((size_t)12 * C * C)), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, C,
                       ws, b1_packed, tail == 2 ? 1 : 0);
    ws += (size_t)12 * C * C;
  }
  const int nt = ff ? 1 : tail == 4 ? 3 : tail;
  if (tail != 0)   // tail 2: wt = the trailing [C][C] projection
    hipLaunchKernelGGL(pack_pgemm_kernel, dim3(grid_for((size_t)nt * C * C)), dim3(256), 0, (hipStream_t)stream, wt, C, nt, ws,
                       tail == 4 ? 1 : 0);
  return rcdm_check_launch();
}

int rcdm_ff_fused(const rcdm_ff_desc* d, const void* x, const float* ln_gamma, const float* ln_beta, const void* wstream,
                  const float* b1_packed, const float* b2, void* out, void* stream) {
  if (!d || !x || !ln_gamma || !ln_beta || !wstream || !b1_packed || !b2 || !out) return RCDM_EINVAL;
  if (d->M <= 0 || d->ldx < d->C || d->ldo < d->C || (d->ldx & 7) || (d->ldo & 7)) return RCDM_EINVAL;
  if (d->C != 320) return RCDM_ESHAPE;
  if (misaligned16(ln_gamma) || misaligned16(ln_beta) || misaligned16(b1_packed) || misaligned16(b2) || misaligned16(x) ||
      misaligned16(out) || misaligned16(wstream))
    return RCDM_EINVAL;
  if (rows_overflow(d->M, d->ldx) || rows_overflow(d->M, d->ldo)) return RCDM_ESHAPE;
  RowArgs a{};
  a.a_in = (const f16*)x; a.out = (f16*)out; a.wstream = (const f16*)wstream;
  a.ln_g = ln_gamma; a.ln_b = ln_beta; a.b1p = b1_packed; a.b2 = b2;
  a.M = d->M; a.lda = d->ldx; a.ldo = d->ldo; a.rows_per_frame = 1; a.frames = 1; a.eps = d->eps;
  return launch_chain<false, false, false, TAIL_FF>(a, (hipStream_t)stream);
}

int rcdm_rowchain(const rcdm_rowchain_desc* d, const void* a_in, const void* res, void* tok, const float* a_bias,
                  const float* ln_gamma, const float* ln_beta, const float* pe, const void* wstream, const float* b1_packed,
                  const float* b2, void* out, const float* gn_stat, const float* gn_gamma, const float* gn_beta,
                  const void* z_res, const float* z_bias, void* stream) {
  if (!d || !a_in || !tok || !a_bias || !ln_gamma || !ln_beta || !wstream || !out) return RCDM_EINVAL;
  const int ncol = d->tail == 0 || d->tail == 2 || d->tail == 4 ? d->C : d->tail * d->C;
  if (d->M <= 0 || d->lda < d->C || d->ldt < d->C || d->ldo < ncol || ((d->lda | d->ldt | d->ldo) & 7)) return RCDM_EINVAL;
  if (res && (d->ldr < d->C || (d->ldr & 7))) return RCDM_EINVAL;
  if (pe && (d->rows_per_frame <= 0 || d->frames <= 0 || d->frames > 8)) return RCDM_EINVAL;
  if ((d->tail == 0 || d->tail == 2) && (!b1_packed || !b2)) return RCDM_EINVAL;
  if (d->C != 320 || d->tail < 0 || d->tail > 4) return RCDM_ESHAPE;
  if (d->tail == 4) {   // frame-major blocks: whole samples of five frames, images of whole 16-pixel groups
    if (d->rows_per_frame <= 0 || d->frames <= 0) return RCDM_EINVAL;
    if (d->frames != 5 || d->rows_per_frame % 16 || d->M % (5 * d->rows_per_frame)) return RCDM_ESHAPE;
  }
  if (!rcdm_rowchain_config_supported(d->C, d->tail, pe ? d->frames : 0)) return RCDM_ESHAPE;
  if (misaligned16(a_bias) || misaligned16(ln_gamma) || misaligned16(ln_beta) || misaligned16(pe) || misaligned16(b1_packed) ||
      misaligned16(b2) || misaligned16(z_bias) || misaligned16(gn_gamma) || misaligned16(gn_beta) || misaligned16(a_in) ||
      misaligned16(res) || misaligned16(tok) || misaligned16(out) || misaligned16(z_res) || misaligned16(wstream))
    return RCDM_EINVAL;
  if (rows_overflow(d->M, d->lda) || rows_overflow(d->M, d->ldt) || rows_overflow(d->M, d->ldo) ||
      (res && rows_overflow(d->M, d->ldr)) || (z_res && rows_overflow(d->M, d->ldz)))
    return RCDM_ESHAPE;
  if (d->tail == 2) {   // feed-forward + trailing projection: the form the engine uses (stage-A residual, no pe)
    if (!res || pe || !z_res || !z_bias || d->ldz < d->C || (d->ldz & 7)) return RCDM_EINVAL;
  }
  if (gn_stat) {   // GroupNorm apply on the incoming rows: only the form without a stage-A residual has the operand free
    if (res || !gn_gamma || !gn_beta || d->gn_groups <= 0 || d->gn_rows <= 0) return RCDM_EINVAL;
    if (d->C % d->gn_groups || d->gn_rows % 16) return RCDM_ESHAPE;
    if (d->tail == 4 ? d->gn_rows != d->rows_per_frame : d->gn_rows < 160) return RCDM_ESHAPE;
  }
  RowArgs a{};
  a.a_in = (const f16*)a_in; a.res = (const f16*)res; a.tok = (f16*)tok; a.out = (f16*)out; a.wstream = (const f16*)wstream;
  a.a_bias = a_bias; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.pe = pe; a.b1p = b1_packed; a.b2 = b2;
  a.M = d->M; a.lda = d->lda; a.ldr = d->ldr; a.ldt = d->ldt; a.ldo = d->ldo;
  a.rows_per_frame = pe || d->tail == 4 ? d->rows_per_frame : 1; a.frames = pe || d->tail == 4 ? d->frames : 1; a.eps = d->eps;
  a.att_scale = (float)(1.0 / sqrt((double)(d->C / 8)));   // eight heads (d_head = 40 at C = 320)
  a.z_res = (const f16*)z_res; a.z_bias = z_bias; a.ldz = d->ldz;
  a.gn_stat = gn_stat; a.gn_g = gn_gamma; a.gn_b = gn_beta; a.gn_G = d->gn_groups; a.gn_rows = d->gn_rows;
  hipStream_t s = (hipStream_t)stream;
#define RCDM_CHAIN(T)                                                                  \
  (res ? (pe ? launch_chain<true, true, true, T>(a, s) : launch_chain<true, true, false, T>(a, s)) \
       : (pe ? launch_chain<true, false, true, T>(a, s) : launch_chain<true, false, false, T>(a, s)))
  switch (d->tail) {
    case 0: return RCDM_CHAIN(TAIL_FF);
    case 1: return RCDM_CHAIN(TAIL_N1);
    case 2: return launch_chain<true, true, false, TAIL_FFP>(a, s);
    case 3: return RCDM_CHAIN(TAIL_N3);
    default: return RCDM_CHAIN(TAIL_ATT);
  }
#undef RCDM_CHAIN
}

}  // extern "C"
