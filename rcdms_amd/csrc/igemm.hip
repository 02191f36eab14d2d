// igemm.hip — MFMA implicit-GEMM for gfx950: Linear / 1x1 conv (taps = 1) and conv3x3 (taps = 9)
// over channels-last f16 rows, fp32 accumulate, fused epilogues.
//
// Replaces (reference, muzishen/RCDMs): InflatedConv3d.forward src/models/resnet.py:10-18, the
// nn.Linear calls of CrossAttention src/models/attention.py:121,140-141,164, Transformer3DModel
// proj_in/proj_out :330,:352, TemporalTransformer3DModel proj_in/out motion_module.py:166,170,
// diffusers FeedForward (GEGLU) and ResnetBlock3D conv_shortcut resnet.py:208.
//
// Structure (one kernel template, three tile shapes):
//   * PERSISTENT blocks: grid = min(#tiles, CUs x blocks/CU); a block walks tiles t, t+G, ... and keeps ONE
//     continuous stream of k-steps across tile boundaries, so the next tile's first operand tiles are already in
//     flight while the current tile's epilogue runs (most GEMMs of this UNet have only 5-20 k-steps per tile:
//     per-tile fill/drain, not the MFMA loop, is what costs).
//   * global -> LDS by buffer_load ... lds (LDS-DMA: no VGPR staging, no ds_write), 2-stage ring, counted
//     s_waitcnt vmcnt + one raw s_barrier per k-step.  Out-of-range rows / taps / channel chunks get the voffset
//     0x80000000 (>= num_records): the hardware writes zeros, so there are no branches in the loader.
//   * The DMA writes LDS lane-linearly (wave-uniform base + lane*16): rows are unpadded 128 B and the bank-conflict
//     fix is an XOR swizzle applied on the SOURCE side — LDS slot (row r, 16-B chunk c') holds global chunk
//     c' ^ ((r>>1)&7); a fragment read of chunk kc of row r reads slot kc ^ ((r>>1)&7).  For the 32x32x16 operand
//     pattern (lanes 0-31 = rows, lane>>5 = chunk parity) every ds_read_b128 lane group hits 16 distinct slots.
//   * The WEIGHT tile is the MFMA A operand and the ACTIVATION tile the B operand, so D[channel][pixel]: a lane
//     owns one pixel and 4 consecutive channels per register quad -> the tile is staged through the ring stage
//     that was just consumed (as f16, 8 bytes per quad; as fp32 for split-K slabs), then a coalesced
//     16-byte-per-lane epilogue (bias / per-sample row vector / GELU / GEGLU / residual / scale in fp32) while the
//     other stage already receives the next tile.
//   tiles <BM, BN, WM x WN waves>: 128x128 (2x2, two blocks per CU) and 256x256 (2x4, one block per CU).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "igemm_plan.h"
#include "igemm_loader.h"
#include "gn_plan.h"
#ifndef RCDM_LNX_ABLATE
#define RCDM_LNX_ABLATE 0   // debug builds (tools/lnx_bench.py): 1 = no partial-statistics loads, 64 = no accumulator transform, 128 = no table write, 256 = no producer statistics
#endif

namespace {

// v: 8 accumulated values of row m at packed columns n..n+7 (GEGLU: g = the matching gate columns n+16..).
// n is a multiple of 8, so every per-column vector (bias, row vector) is fetched as two aligned float4.
__device__ __forceinline__ void load8(const float* src, float (&d)[8]) {
  const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
  d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; d[3] = a[3];
  d[4] = b[0]; d[5] = b[1]; d[6] = b[2]; d[7] = b[3];
}

// v[0..8) += eight consecutive slab values at element offset `off` (fp32 slabs, or f16 ones: IgemmArgs::slab16)
__device__ __forceinline__ void slab_add8(const IgemmArgs& p, size_t off, float (&v)[8]) {
  if (p.slab16) {
    Pack16 h;
    h.u = *(const uint4*)((const f16*)p.partial + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)h.e[e];
  } else {
    const f32x4 a = *(const f32x4*)(p.partial + off), b = *(const f32x4*)(p.partial + off + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] += a[e];
      v[4 + e] += b[e];
    }
  }
}

template <bool QG = false>   // QG: the quick-GELU form compiled in (its own reduce kernel: the existing ones keep their code)
__device__ __forceinline__ uint4 epilogue_store(const IgemmArgs& p, int m, int n, float (&v)[8], float (&g)[8]) {   // returns the 8 halfs it stored
  int oc = n;
  if (p.epi & RCDM_EPI_GEGLU) {
    if (p.epi & RCDM_EPI_BIAS) {
      float bh[8], bg[8];
      load8(p.bias + n, bh);
      load8(p.bias + n + kGegluGroup, bg);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] += bh[e];
        g[e] += bg[e];
      }
    }
    gelu8(g);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= g[e];
    oc = geglu_out_col(n);
  } else if (p.epi & RCDM_EPI_BIAS) {
    float bb[8];
    load8(p.bias + n, bb);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += bb[e];
  }
  if (p.epi & RCDM_EPI_ROWVEC) {
    float rv[8];
    load8(p.rowvec + (size_t)(m / p.rows_per_sample) * p.ldt + oc, rv);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += rv[e];
  }
  if constexpr (QG) {
    if (p.epi & RCDM_EPI_QUICK_GELU) quick_gelu8(v);
  }
  if (p.epi & RCDM_EPI_GELU) gelu8(v);
  if (p.epi & RCDM_EPI_RESIDUAL) {
    Pack16 r;
    r.u = *(const uint4*)(p.res + (size_t)m * p.ldr + oc);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += (float)r.e[e];
  }
  Pack16 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o.e[e] = (f16)(v[e] * p.out_scale);
  *(uint4*)(p.out + (size_t)m * p.ldc + oc) = o.u;
  if (p.dup) *(uint4*)(p.out + (size_t)m * p.ldc + oc + p.dup) = o.u;
  return o.u;
}

// Every load the block has in flight — the next tile's first DMA pieces (issued a k-step and a staging phase ago) and
// this tile's residual / bias prefetches — is waited for right before the tile's first output store, with the
// compiler-visible form of s_waitcnt: (a) once stores are in flight vmcnt cannot separate them from DMA pieces, so this
// is the last point where "operands landed" can be established cheaply; (b) the builtin lets the compiler's hazard
// tracking see that no load is pending into a register the main loop reuses (prefetches that a branch never consumes
// would otherwise make it guard those registers with its own vmcnt(0) after every DMA issue in the k-loop).
#define RCDM_PRE_STORE_WAIT() __builtin_amdgcn_s_waitcnt(0x0F70) /* vmcnt(0); expcnt / lgkmcnt untouched */

// -DRCDM_TRACE_PHASES (debug builds for tools/trace_phases.py): the trace record grows from 4 to 8 int64 per block and
// the fused epilogue is stamped after its first barrier, after staging and after the pre-store wait.
#ifdef RCDM_TRACE_PHASES
#define RCDM_PHASE_BEGIN() if (p.trace) tq = __builtin_amdgcn_s_memtime()
#define RCDM_PHASE_STAMP(acc_)                                  \
  if (p.trace) {                                                \
    const long long n_ = __builtin_amdgcn_s_memtime();          \
    acc_ += n_ - tq;                                            \
    tq = n_;                                                    \
  }
constexpr int TRACE_SLOTS = 8;
#else
#define RCDM_PHASE_BEGIN()
#define RCDM_PHASE_STAMP(acc_)
#ifdef RCDM_TRACE_LX   // kernel-start stamps (statistics fetched / first / second barrier) in slots 4-6
constexpr int TRACE_SLOTS = 8;
#else
constexpr int TRACE_SLOTS = 4;
#endif
#endif

template <int TAPS, int BM_, int BN_, int WM, int WN, int NSTAGE, bool E16, int LX = 0>  // LX: deferred-LayerNorm epilogues (rcdm_gemm_lnx) compiled in: 1 = row statistics only, 2 = consumer (+ statistics); 4 = the quick-GELU epilogue instead (RCDM_EPI_QUICK_GELU launches only: every other instantiation keeps its code and registers)
// (second launch bound = waves per SIMD the tile's LDS footprint allows: 4 blocks of 64x64, 3 of 128x64, 2 of 128x128 per CU)
#ifdef RCDM_DMA_MINW2   // A/B builds: the round-3 bound (2 waves per SIMD for every tile)
#define RCDM_DMA_MINW(wm, wn, bm, bn, ns) 2
#else
#define RCDM_DMA_MINW(wm, wn, bm, bn, ns) (((wm) * (wn) == 4 && (bm) * (bn) <= 64 * 64 && (ns) == 2) ? 4 : ((wm) * (wn) == 4 && (bm) * (bn) <= 128 * 64) ? 3 : 2)
#endif
__global__ __launch_bounds__(WM * WN * 64, RCDM_DMA_MINW(WM, WN, BM_, BN_, NSTAGE))
void igemm_dma_kernel(const IgemmArgs p) {
  constexpr int NW = WM * WN;             // waves
  constexpr int FM = BM_ / WM / 32;       // pixel fragments per wave
  constexpr int FN = BN_ / WN / 32;       // channel fragments per wave
  constexpr int A_BYTES = BM_ * 128, B_BYTES = BN_ * 128, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int AI = BM_ / 8 / NW;        // 1-KiB DMA pieces per wave per stage, activations
  constexpr int BI = BN_ / 8 / NW;        // weights
  static_assert(BM_ % (8 * NW) == 0 && BN_ % (8 * NW) == 0, "DMA pieces must divide evenly over the waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // deferred LayerNorm, consumer side (LX & 2): LTPR threads per tile row sum the row's partial statistics at the tile's
  // FIRST k-step — the loads go out in front of the wait for that step's operands and cost no round trip of their own —
  // and (rstd, mean rstd) sits in a [BM][2] table behind the ring until the epilogue reads it
  constexpr bool LXC = (LX & 2) != 0;
  constexpr int LTPR = (WM * WN * 64) / BM_;
  static_assert(!LXC || LTPR == 1 || LTPR == 2 || LTPR == 4, "threads per row of the LayerNorm table");
  float* ltab = (float*)(smem + NSTAGE * (BM_ + BN_) * 128);
  float* lvS = ltab + 2 * BM_;   // [BN] S of the tile's channels
  // the slots' column counts for the statistics of every tile after the first: read from LDS where they are needed (end of an
  // epilogue), not kept in four more SGPRs for the whole kernel — the consumer kernels sit at the SGPR cap, and the scalars
  // that no longer fit go to VGPR lanes and push vector registers into scratch
  // ... followed by [BN] bias, [BN] the row vector of the first sample the tile meets and [BN] that of the second (zeros where
  // the launch has none): everything the epilogue adds per column goes into the accumulators with the LayerNorm identity, so
  // the staged half is the normalised projection itself and is rounded once, as the reference's fp16 Linear rounds it
  float* lgeo = lvS + 4 * BN_;
  static_assert((2 * BM_ + 4 * BN_) * 4 + sizeof(LnxGeo) <= kLnxTabBytes || !LXC, "the LayerNorm table behind the ring");
  static_assert(!LXC || BN_ <= WM * WN * 64, "one thread per four table columns");
  const bool lx_rvp = LXC && (p.epi & RCDM_EPI_ROWVEC) && !(p.epi & RCDM_EPI_GEGLU) && p.rows_per_sample >= BM_;
  // this thread's four entries of the column tables of the tile at (m0, n0): S | bias | row vector | next sample's row vector
  auto lx_cols = [&](int m0, int n0, int ts) __attribute__((always_inline)) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int grp = ts / (BN_ / 4), n = n0 + 4 * (ts % (BN_ / 4));
    if (ts < BN_ && n < p.N) {
      const int smp = lx_rvp ? m0 / p.rows_per_sample + (grp == 3) : 0;
      if (grp == 0) v = *(const f32x4*)(p.lnx_S + n);
      else if (grp == 1) { if (p.epi & RCDM_EPI_BIAS) v = *(const f32x4*)(p.bias + n); }
      else if (lx_rvp && (grp == 2 || (smp * p.rows_per_sample < p.M && smp * p.rows_per_sample < m0 + BM_)))
        v = *(const f32x4*)(p.rowvec + (size_t)smp * p.ldt + n);
    }
    return v;
  };
  if (LXC && threadIdx.x == 0) *(LnxGeo*)lgeo = p.lnx_geo;   // published by the barriers of the first tile's k-loop
  constexpr bool lnx_k = LXC;   // the (LX & 2) instantiation is only launched for consumers (p.lnx_stat != nullptr)

  const int ntiles = p.tilesM * p.tilesN;
  const int G = gridDim.x;
  const int my_tiles = ((int)blockIdx.x < ntiles) ? (ntiles - 1 - (int)blockIdx.x) / G + 1 : 0;
  const int ks_begin = blockIdx.y * p.nk_per_split;
  const int ks_end = min(p.nk, ks_begin + p.nk_per_split);
  const int nkl = ks_end - ks_begin;
  if (my_tiles == 0 || nkl <= 0) return;

  auto tile_of = [&](int i, int& m0, int& n0) __attribute__((always_inline)) {
    igemm_tile_origin<BM_, BN_>(p, (int)blockIdx.x + i * G, m0, n0);
  };

  const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, 0x7FFFFFFF, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcA2 = __builtin_amdgcn_make_buffer_rsrc((void*)(TAPS == 9 ? p.A2 : p.A), 0, 0x7FFFFFFF, 0x00020000);
  const int Hv = p.Hi << p.up, Wv = p.Wi << p.up;

  // ---- loader state of the tile currently being ISSUED (static-indexed arrays: fully unrolled) ----------------
  const int lrow = lane >> 3, lch = lane & 7;
  IgemmPixelRow a_row[AI];
  unsigned w_off[BI];
  int a_c[AI], w_c[BI];
  auto setup_loader = [&](int m0, int n0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int row = (wave * AI + i) * 8 + lrow;
      a_c[i] = igemm_swizzle_chunk(row, lch);
      a_row[i] = igemm_pixel_row<TAPS>(p, m0 + row, m0 + row < p.M);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int row = (wave * BI + i) * 8 + lrow;
      w_c[i] = igemm_swizzle_chunk(row, lch);
      w_off[i] = igemm_weight_row(p, n0 + row);
    }
  };

  auto issue = [&](int ks, int stage) __attribute__((always_inline)) {
    const IgemmKStep k = igemm_kstep<TAPS>(p, ks);
    char* sbase = smem + stage * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const unsigned vo = igemm_pixel_offset<TAPS>(p, k, a_row[i], k.c0 + a_c[i], Hv, Wv);
      if (TAPS == 9 && k.s2)   // (wave-uniform)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rsrcA2, (__attribute__((address_space(3))) void*)(sbase + (wave * AI + i) * 1024), 16, vo, 0, 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rsrcA, (__attribute__((address_space(3))) void*)(sbase + (wave * AI + i) * 1024), 16, vo, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const unsigned vo = igemm_weight_offset(p, k, w_off[i], k.c0 + w_c[i]);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsrcW, (__attribute__((address_space(3))) void*)(sbase + A_BYTES + (wave * BI + i) * 1024), 16, vo, 0, 0, 0);
    }
  };

  // ---- compute mapping -------------------------------------------------------------------------------------
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, hi = lane >> 5;
  const int sw = (lr >> 1) & 7;
  int koff[4];  // byte offset of k-chunk (kk*2 + hi) inside a swizzled 128-B row
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) koff[kk] = (((kk * 2 + hi) ^ sw) << 4);
  const int rowA = (wm * FM * 32 + lr) * 128, rowB = A_BYTES + (wn * FN * 32 + lr) * 128;
  const bool geglu = (p.epi & RCDM_EPI_GEGLU) != 0;

  f32x16 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  long long ts0 = 0, ts_loop = 0, ts_epi = 0;
  long long ts_a = 0, ts_b = 0, ts_c = 0, tq = 0;  // RCDM_TRACE_PHASES only
  if (p.trace) ts0 = __builtin_amdgcn_s_memtime();
  int cm0, cn0;               // tile being computed
  tile_of(0, cm0, cn0);
  // deferred LayerNorm: this thread's share of the first tile's row statistics and its 4 entries of S are requested
  // FIRST — the loader set-up and the prologue DMA below cover their round trip (asked for behind the DMA they cost the
  // 16x16-level attn2.to_q +2.3 us: tools/lnx_bench.py, -DRCDM_LNX_ABLATE=1)
  f32x2 lx_rs = {1.f, 0.f};
  f32x4 lx_s4 = {0.f, 0.f, 0.f, 0.f};
  LnxRow<LTPR, LXC ? kLnxMaxParts : 1> lx_row0;
  if constexpr (LXC) {
    const int lm = cm0 + t / LTPR;
#if !(RCDM_LNX_ABLATE & 1)
    lx_row0.load(p.lnx_stat, p.lnx_ld, lm, lm < p.M, p.lnx_parts, t % LTPR);
#endif
    lx_s4 = lx_cols(cm0, cn0, t);
  }
#ifdef RCDM_TRACE_LX
  if (p.trace) ts_a = __builtin_amdgcn_s_memtime() - ts0;
#endif
  setup_loader(cm0, cn0);
  const int total = my_tiles * nkl;
  int i_tile = 0, i_ks = 0;   // next (tile, k-step) to issue
  int i_stage = 0;            // ring slot the next issue goes to
  auto issue_next = [&]() __attribute__((always_inline)) {
    if (i_ks == nkl) {
      i_ks = 0;
      ++i_tile;
      int im0, in0;
      tile_of(i_tile, im0, in0);
      setup_loader(im0, in0);
    }
    issue(ks_begin + i_ks, i_stage);
    ++i_ks;
    i_stage = i_stage + 1 == NSTAGE ? 0 : i_stage + 1;
  };
  // prologue: NSTAGE-1 steps in flight
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < total) issue_next();
  // deferred LayerNorm: this thread's share of the NEXT tile's row statistics -> (rstd, mean rstd), and its 4 entries of S.
  // Fetched where registers are free and a memory wait follows anyway (here: behind the prologue DMA; for later tiles of a
  // persistent block: at the end of the previous epilogue); written to the LDS table after the tile's first barrier.
  auto lx_fetch = [&](int m0, int n0) __attribute__((always_inline)) {
    const int lm = m0 + t / LTPR;
    float r_ = 1.f, m_ = 0.f;
#if !(RCDM_LNX_ABLATE & 1)
    const f32x4 g4 = *(const f32x4*)lgeo;   // wave-uniform: back to scalars, four VGPRs would not fit either
    auto sc = [](float v) __attribute__((always_inline)) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    lnx_row<LTPR, kLnxMaxParts>(p, LnxGeo{sc(g4[0]), sc(g4[1]), sc(g4[2]), sc(g4[3])}, lm, lm < p.M, t % LTPR, r_, m_);
#endif
    lx_rs = f32x2{r_, m_};
    int ts = t;   // (opaque: the address is formed here, not once in front of the tile loop and held in a VGPR pair)
    asm volatile("" : "+v"(ts));
    lx_s4 = lx_cols(m0, n0, ts);
  };
#ifdef RCDM_TRACE_LX
  if (p.trace) ts_b = __builtin_amdgcn_s_memtime() - ts0;
#endif
#if !(RCDM_LNX_ABLATE & 1)
  if constexpr (LXC) {
    float r_, m_;
    lx_row0.finish(p.lnx_geo, p.lnx_parts, p.lnx_invC, p.lnx_eps, t % LTPR, r_, m_);
    lx_rs = f32x2{r_, m_};
  }
#endif
#ifdef RCDM_TRACE_LX
  if (p.trace) ts_c = __builtin_amdgcn_s_memtime() - ts0 + (long long)(lx_rs.x == 12345.f);   // ticks from kernel start to "statistics finished"
#endif
  int c_ks = 0, c_tile = 0;   // k-step / tile being computed
  int c_stage = 0;            // ring slot being computed
  int post_epi = 0;           // 2: an epilogue just ran (operands of the next step already landed), 1: its stores may be in flight

  constexpr int PIECES = AI + BI;  // DMA instructions per wave per step
  for (int g = 0; g < total; ++g) {
    // this wave's DMA pieces of step g have landed (loads retire in order: at most the pieces of the NSTAGE-2
    // younger steps may still be in flight); the barrier makes everybody's visible and also guarantees every
    // wave is done reading the slot of step g-1, which the issue below refills
    const int younger = min(NSTAGE - 2, total - 1 - g);
    const bool lx_now = lnx_k && c_ks == 0;
    if (post_epi == 2) {
      // first step of a new tile: every DMA piece issued so far was waited for inside the epilogue, BEFORE its output
      // stores were issued — nothing to wait for here, and the stores' round trip to L2 (vmcnt counts them, and they
      // retire out of order with loads, so a counted wait cannot skip them) is hidden under this step's MFMAs
      post_epi = 1;
    } else {
      if (post_epi == 1 || younger <= 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (post_epi == 1: the epilogue's stores may still be counted)
      } else if (NSTAGE >= 4 && younger >= 2) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTAGE >= 4 ? 2 * PIECES : 0) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTAGE >= 3 ? PIECES : 0) : "memory");
      }
      post_epi = 0;
    }
    __builtin_amdgcn_s_barrier();
    if constexpr (LXC && !(RCDM_LNX_ABLATE & 128)) if (lx_now) {   // (after the barrier: the previous tile's epilogue is done reading the table)
      if (t % LTPR == 0) *(f32x2*)(ltab + 2 * (t / LTPR)) = lx_rs;
      if (t < BN_) *(f32x4*)(lvS + 4 * t) = lx_s4;
    }
    // 8-wave blocks put two waves on every SIMD, released by the same barrier: if both issued their DMA pieces first
    // (each piece stalls the issuing wave for ~100 cycles) the SIMD's matrix pipe would idle through both bursts.
    // The second half of the block therefore issues after its first two k-chunks, under the first half's MFMAs.
    const bool more = g + NSTAGE - 1 < total;
    const int issue_kk = (NW == 8 && wave >= 4) ? 2 : 0;
    const char* sb = smem + c_stage * STAGE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if ((kk == 0 || (NW == 8 && kk == 2)) && more && issue_kk == kk) issue_next();
      f16x8 wf[FN], xf[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) wf[i] = *(const f16x8*)(sb + rowB + i * 32 * 128 + koff[kk]);
#pragma unroll
      for (int j = 0; j < FM; ++j) xf[j] = *(const f16x8*)(sb + rowA + j * 32 * 128 + koff[kk]);
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    const int e_stage = c_stage;  // slot just consumed
    c_stage = c_stage + 1 == NSTAGE ? 0 : c_stage + 1;
    if (++c_ks < nkl) continue;
    long long te0 = 0;
    if (p.trace) te0 = __builtin_amdgcn_s_memtime();

    // ---- tile done: epilogue.  The slot just consumed is idle until step g+NSTAGE is issued after the next
    // barrier, so it serves as the fp32 staging tile ([RP rows][BN] floats, 16-B chunks XOR-swizzled by row) for a
    // coalesced 16-byte-per-lane store phase; the DMA of the next tile's first step keeps flowing into the other
    // stage.  Raw s_barrier + lgkmcnt only: a __syncthreads() here would drain that DMA (vmcnt(0)).
    c_ks = 0;
    if constexpr (E16 && (LX & 2) != 0 && !(RCDM_LNX_ABLATE & 64)) {
      // deferred LayerNorm: x W'^T of the raw rows -> rstd acc - (mean rstd) S = LayerNorm(x) W'^T, on the accumulators,
      // before any of the epilogue's prefetches is live; everything below (bias b', row table, GEGLU, residual) runs unchanged
      // on top.  The table was written behind the first k-step's barrier: a one-step tile needs one more barrier here.
      if (nkl == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      f32x2 rs[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j) rs[j] = *(const f32x2*)(ltab + 2 * ((wm * FM + j) * 32 + lr));
      float sec[FM];   // 1: the row belongs to the second sample the tile meets
      const int lx_switch = lx_rvp ? (cm0 / p.rows_per_sample + 1) * p.rows_per_sample : 0x7fffffff;
#pragma unroll
      for (int j = 0; j < FM; ++j) sec[j] = cm0 + (wm * FM + j) * 32 + lr >= lx_switch ? 1.f : 0.f;
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float* col = lvS + (wn * FN + i) * 32 + 8 * q + 4 * hi;   // this quad's 4 channels
          const f32x4 s4 = *(const f32x4*)col;
          f32x4 b4 = *(const f32x4*)(col + BN_);
          if (lx_rvp) {   // (wave-uniform) rows of the second sample get its row vector: b + w (r1 - r0), w = 0 | 1
            const f32x4 r0 = *(const f32x4*)(col + 2 * BN_), r1 = *(const f32x4*)(col + 3 * BN_);
            b4 += r0;
            const f32x4 d4 = r1 - r0;
#pragma unroll
            for (int j = 0; j < FM; ++j)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[i][j][4 * q + e] = __builtin_fmaf(acc[i][j][4 * q + e], rs[j].x,
                                                      __builtin_fmaf(-rs[j].y, s4[e], __builtin_fmaf(sec[j], d4[e], b4[e])));
          } else {
#pragma unroll
            for (int j = 0; j < FM; ++j)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[i][j][4 * q + e] = __builtin_fmaf(acc[i][j][4 * q + e], rs[j].x, __builtin_fmaf(-rs[j].y, s4[e], b4[e]));
          }
        }
    }
    if constexpr (E16 && (LX & 2) != 0 && !(RCDM_LNX_ABLATE & 64)) {
      // a row vector with fewer rows per sample than the tile has (a tile meets more than two samples: no column table holds
      // them): added to the accumulators row by row, here, so that it too is in before the one rounding to f16
      if ((p.epi & RCDM_EPI_ROWVEC) && !geglu && !lx_rvp) {   // (wave-uniform)
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int m = cm0 + (wm * FM + j) * 32 + lr;
          const bool m_ok = m < p.M;
          const float* rvr = p.rowvec + (size_t)((m_ok ? m : 0) / p.rows_per_sample) * p.ldt + cn0;
#pragma unroll
          for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int col = (wn * FN + i) * 32 + 8 * q + 4 * hi;
              if (m_ok && cn0 + col < p.N) {
                const f32x4 r4 = *(const f32x4*)(rvr + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] += r4[e];
              }
            }
        }
      }
    }
    if constexpr (E16) {
      // ---- f16 staging (every launch without split-K): the accumulators are rounded to f16 (the reference's fp16
      // Linear / Conv outputs are rounded at the same point, give or take the bias) and staged as [rows][BN] halfs:
      // half the LDS bytes of an fp32 tile through ds_write_b64, and a 128x128 tile fits the consumed ring slot in ONE
      // pass (two barriers instead of four).  16-byte chunks are XOR-swizzled by (row >> 1) & 7 (two-way conflicts on
      // the 16 writes of a wave, none on the reads).  Bias, row vector, GELU / GEGLU, residual and scale are applied
      // in fp32 on the way out.  The post phase is VALU- and latency-bound (measured: ~3.4 k of a 128x128 tile's ~4.8 k
      // epilogue ticks), so (a) every global read it needs — bias, the row vector of the (at most two) samples the
      // tile touches, residual rows — is issued before the staging barriers and covered by ONE wait, so that no
      // per-item vmcnt wait ends up behind the previous item's store; (b) staged reads of all items are issued
      // together; (c) out = (h + bias + rowvec + res) * scale runs as v_fma_mix_f32 / v_fma_mixlo|hi_f16 on the f16
      // inputs directly: 2 instructions per output instead of cvt + add + add + mul + cvt.
      constexpr int NT = NW * 64;
      constexpr int RPH = (STAGE_BYTES / (BN_ * 2)) >= BM_ ? BM_ : (STAGE_BYTES / (BN_ * 2)) / 32 * 32;
      constexpr int NPASS = BM_ / RPH;
      static_assert(BM_ % RPH == 0 && RPH % 32 == 0, "staging passes must tile the block");
      f16* sH = (f16*)(smem + e_stage * STAGE_BYTES);
      constexpr int P_TPR = BN_ / 8, P_RPI = NT / P_TPR, P_ITEMS = RPH / P_RPI;
      constexpr int G_TPR = BN_ / 16, G_RPI = NT / G_TPR, G_ITEMS = RPH / G_RPI;
      static_assert(NT % P_TPR == 0 && RPH % P_RPI == 0 && NT % G_TPR == 0 && RPH % G_RPI == 0, "epilogue sweep");
      const int pc8 = t % P_TPR, pr0 = t / P_TPR;
      const int oc8 = t % G_TPR, gr0 = t / G_TPR;
      const int hc = (oc8 >> 1) * 4 + (oc8 & 1);  // GEGLU: 16-B chunk (8 halfs) of the hidden columns; the gate is 2 chunks on
      const int pn = geglu ? cn0 + hc * 8 : cn0 + pc8 * 8;   // first packed column this thread handles
      const bool pn_ok = pn < p.N;
      constexpr bool WHOLE = NPASS * P_ITEMS <= 8;
      constexpr int RCH = WHOLE ? P_ITEMS : (P_ITEMS < 4 ? P_ITEMS : 4);  // staged reads in flight per thread
      Pack16 resv[WHOLE ? NPASS : 1][P_ITEMS];
      const bool has_res = !geglu && (p.epi & RCDM_EPI_RESIDUAL);
      const bool has_rv = !geglu && (p.epi & RCDM_EPI_ROWVEC);
      // per-sample row vector: a tile of BM rows touches at most two samples when rows_per_sample >= BM
      const bool rv_pair = has_rv && p.rows_per_sample >= BM_;
      const int smp0 = rv_pair ? cm0 / p.rows_per_sample : 0;
      const int m_switch = rv_pair ? (smp0 + 1) * p.rows_per_sample : 0x7fffffff;
      float bA[8], bB[8], rvA[8], rvB[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) bA[e] = bB[e] = rvA[e] = rvB[e] = 0.f;
      // (a deferred-LayerNorm consumer has bias and the tile's row vectors in its accumulators already)
      if ((p.epi & RCDM_EPI_BIAS) && pn_ok && !LXC) {
        load8(p.bias + pn, bA);
        if (geglu) load8(p.bias + pn + kGegluGroup, bB);
      }
      if (rv_pair && pn_ok && !LXC) {
        load8(p.rowvec + (size_t)smp0 * p.ldt + pn, rvA);
        if (m_switch < p.M && m_switch < cm0 + BM_) load8(p.rowvec + (size_t)(smp0 + 1) * p.ldt + pn, rvB);
      }
      // deferred LayerNorm of the A rows (rcdm_gemm_lnx): LTPR threads per tile row sum that row's partial statistics;
      // (rstd, mean rstd) go to a [BM][2] table behind the ring, published by the staging barrier of the first pass
      constexpr bool lnx = LXC;
      const bool stat_on = (LX & 3) != 0 && p.stat_out != nullptr && !(RCDM_LNX_ABLATE & 256);
      const int stat_tn = cn0 / BN_;
      const int dup_rows = p.dup ? (int)(p.dup / p.ldc) : 0;
      if (WHOLE && !geglu) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
          for (int it = 0; it < P_ITEMS; ++it) {
            const int m = cm0 + ps * RPH + pr0 + it * P_RPI;
            resv[WHOLE ? ps : 0][it].u = make_uint4(0, 0, 0, 0);
            if (has_res && m < p.M && pn_ok) resv[WHOLE ? ps : 0][it].u = *(const uint4*)(p.res + (size_t)m * p.ldr + pn);
          }
      }
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        if (!WHOLE && !geglu) {
#pragma unroll
          for (int it = 0; it < P_ITEMS; ++it) {
            const int m = cm0 + ps * RPH + pr0 + it * P_RPI;
            resv[0][it].u = make_uint4(0, 0, 0, 0);
            if (has_res && m < p.M && pn_ok) resv[0][it].u = *(const uint4*)(p.res + (size_t)m * p.ldr + pn);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        RCDM_PHASE_BEGIN();
        __builtin_amdgcn_s_barrier();  // operand reads (ps = 0) / previous pass's staged reads are complete
        RCDM_PHASE_STAMP(ts_a);
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int blk = wm * FM + j;
          if (blk / (RPH / 32) == ps) {
            const int prow = (blk % (RPH / 32)) * 32 + lr;
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                union { f16 h[4]; uint2 u; } pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk.h[e] = (f16)acc[i][j][4 * q + e];
                const int piece = ((wn * FN + i) * 32 + 8 * q + 4 * hi) >> 2;
                *(uint2*)(sH + prow * BN_ + ((piece ^ (((prow >> 1) & 7) << 1)) << 2)) = pk.u;
              }
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        RCDM_PHASE_STAMP(ts_b);
        RCDM_PRE_STORE_WAIT();
        RCDM_PHASE_STAMP(ts_c);
        const int mbase = cm0 + ps * RPH;
        const float sc = p.out_scale;
        if (geglu) {
          const int oc = geglu_out_col(pn);
#pragma unroll
          for (int it0 = 0; it0 < G_ITEMS; it0 += RCH) {
            Pack16 hh[RCH], gg[RCH];
#pragma unroll
            for (int k = 0; k < RCH; ++k)
              if (it0 + k < G_ITEMS) {
                const int row = gr0 + (it0 + k) * G_RPI;
                const int sx = (row >> 1) & 7;
                hh[k].u = *(const uint4*)(sH + row * BN_ + ((hc ^ sx) << 3));
                gg[k].u = *(const uint4*)(sH + row * BN_ + (((hc + 2) ^ sx) << 3));
              }
#pragma unroll
            for (int k = 0; k < RCH; ++k)
              if (it0 + k < G_ITEMS) {
                const int m = mbase + gr0 + (it0 + k) * G_RPI;
                if (m < p.M && pn_ok) {
                  Pack16 o;
                  o.u = geglu8(hh[k].u, gg[k].u, bA, bB, sc);
                  *(uint4*)(p.out + (size_t)m * p.ldc + oc) = o.u;
                  if (p.dup) *(uint4*)(p.out + (size_t)m * p.ldc + oc + p.dup) = o.u;
                }
              }
          }
        } else {
          const bool gelu_on = (p.epi & (RCDM_EPI_GELU | ((LX & 4) ? RCDM_EPI_QUICK_GELU : 0))) != 0;
          float cA[8], cB[8];  // (bias + row vector) * scale of the tile's first / second sample
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            cA[e] = (bA[e] + rvA[e]) * sc;
            cB[e] = (bA[e] + rvB[e]) * sc;
          }
#pragma unroll
          for (int it0 = 0; it0 < P_ITEMS; it0 += RCH) {
            Pack16 hh[RCH];
            // producer side of a deferred LayerNorm: this thread's 8 stored values as shifted sums about its own first one
            float stk[RCH], stv1[RCH], stv2[RCH];
#pragma unroll
            for (int k = 0; k < RCH; ++k) stk[k] = stv1[k] = stv2[k] = 0.f;
#pragma unroll
            for (int k = 0; k < RCH; ++k)
              if (it0 + k < P_ITEMS) {
                const int row = pr0 + (it0 + k) * P_RPI;
                hh[k].u = *(const uint4*)(sH + row * BN_ + ((pc8 ^ ((row >> 1) & 7)) << 3));
              }
#pragma unroll
            for (int k = 0; k < RCH; ++k)
              if (it0 + k < P_ITEMS) {
                const int it = it0 + k;
                const int m = mbase + pr0 + it * P_RPI;
                if (m < p.M && pn_ok) {
                  const Pack16& rr = resv[WHOLE ? ps : 0][it];
                  Pack16 o;
                  if (gelu_on || (has_rv && !rv_pair)) {
                    // rare forms (stage-1 GELU feed-forward; row vector with fewer rows per sample than the tile): plain
                    // fp32 arithmetic
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = (float)hh[k].e[e] + bA[e];
                    if (has_rv && rv_pair) {
                      const bool second = m >= m_switch;
#pragma unroll
                      for (int e = 0; e < 8; ++e) v[e] += second ? rvB[e] : rvA[e];
                    } else if (has_rv && !LXC) {   // (a deferred-LayerNorm consumer has it in its accumulators)
                      float rv[8];
                      load8(p.rowvec + (size_t)(m / p.rows_per_sample) * p.ldt + pn, rv);
#pragma unroll
                      for (int e = 0; e < 8; ++e) v[e] += rv[e];
                    }
                    if (gelu_on) {
                      if constexpr ((LX & 4) != 0) quick_gelu8(v);
                      else
                      gelu8(v);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) o.e[e] = (f16)((v[e] + (float)rr.e[e]) * sc);
                  } else {
                    const bool second = m >= m_switch;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                      const float c0 = second ? cB[2 * d] : cA[2 * d], c1 = second ? cB[2 * d + 1] : cA[2 * d + 1];
                      const float t0 = mix_f16_f32(hh[k].v[d], 0, sc, c0);
                      const float t1 = mix_f16_f32(hh[k].v[d], 1, sc, c1);
                      o.v[d] = mix_f16_pack(rr.v[d], sc, t0, t1);
                    }
                  }
                  *(uint4*)(p.out + (size_t)m * p.ldc + pn) = o.u;
                  if (p.dup) *(uint4*)(p.out + (size_t)m * p.ldc + pn + p.dup) = o.u;
                  if (stat_on) {   // (v_dot2c_f32_f16 was tried for two elements per instruction: wrong sums on gfx950)
                    stk[k] = (float)o.e[0];
                    const float nk = -stk[k];
#pragma unroll
                    for (int e = 1; e < 8; ++e) {
                      const float f = mix_f16_f32(o.v[e >> 1], e & 1, 1.f, nk);   // x - k in one instruction; exact: both are halfs
                      stv1[k] += f;
                      stv2[k] = __builtin_fmaf(f, f, stv2[k]);
                    }
                  }
                }
              }
            if (stat_on) {
              // the slot rule: igemm_args.h.  Wave-uniform; every lane of the P_TPR-lane row group takes part in the DPP sums.
              // The row's pivot K is its first stored value of this column tile (the pc8 == 0 lane's own pivot); a lane moves its
              // sums from its own pivot k to K with dk = k - K (exact): sum(f - K) = s + 8 dk, sum((f - K)^2) = q + dk (2 s + 8 dk)
              // — nothing of the size of the row's offset is squared or added.  Lanes past N or M (nothing stored) add nothing.
              // The batch's 3 RCH reductions are independent chains the scheduler interleaves; one store per row and column tile
              const float stat_n = (float)min(BN_, p.N - cn0);
              const float stat_inv_n = 1.f / stat_n;
              float piv[RCH];
#pragma unroll
              for (int k = 0; k < RCH; ++k) {
                if constexpr (P_TPR <= 16) piv[k] = group_first<P_TPR>(stk[k]);
                else piv[k] = group_sum<P_TPR>(pc8 == 0 ? stk[k] : 0.f);
              }
#pragma unroll
              for (int k = 0; k < RCH; ++k) {
                const bool on = pn_ok && mbase + pr0 + (it0 + k) * P_RPI < p.M;
                const float dk = on ? stk[k] - piv[k] : 0.f, n8 = 8.f * dk;
                stv2[k] = group_sum<P_TPR>(__builtin_fmaf(dk, 2.f * stv1[k] + n8, stv2[k]));
                stv1[k] = group_sum<P_TPR>(stv1[k] + n8);
              }
              if (pc8 == 0) {
#pragma unroll
                for (int k = 0; k < RCH; ++k) {
                  const int m = mbase + pr0 + (it0 + k) * P_RPI;
                  if (it0 + k < P_ITEMS && m < p.M) {
                    const f32x2 slot = {__builtin_fmaf(stat_n, piv[k], stv1[k]),
                                        fmaxf(__builtin_fmaf(-stv1[k] * stat_inv_n, stv1[k], stv2[k]), 0.f)};
                    *(f32x2*)(p.stat_out + ((size_t)stat_tn * p.stat_ld + m) * 2) = slot;
                    if (dup_rows) *(f32x2*)(p.stat_out + ((size_t)stat_tn * p.stat_ld + m + dup_rows) * 2) = slot;
                  }
                }
              }
            }
          }
        }
      }
    } else {
      // ---- split-K launches only: the fp32 tile goes to this split's slab (rcdm_*_workspace_bytes), staged through
      // the consumed ring slot ([RP rows][BN] floats, 16-B chunks XOR-swizzled by row) so that the slab is written
      // in coalesced 2 x 16-byte pieces per lane; bias / row vector / residual / GEGLU belong to splitk_reduce_kernel
      constexpr int RP = (STAGE_BYTES / (BN_ * 4)) >= 64 ? 64 : 32;   // rows per pass
      constexpr int NPASS = BM_ / RP;
      constexpr int NT = NW * 64;
      constexpr int TPR = BN_ / 8, RPI = NT / TPR, ITEMS = RP / RPI;  // threads per row, rows per sweep
      static_assert(NT % TPR == 0 && RP % RPI == 0, "epilogue sweep must tile the pass exactly");
      float* sC = (float*)(smem + e_stage * STAGE_BYTES);
      float* dst = p.partial + (size_t)blockIdx.y * p.M * p.N;
      const int c8 = t % TPR, r0 = t / TPR;
      const int n = cn0 + c8 * 8;
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // operand reads (ps = 0) / previous pass's staged reads are complete
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int blk = wm * FM + j;
          if (blk / (RP / 32) == ps) {
            const int prow = (blk % (RP / 32)) * 32 + lr;
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int chunk = ((wn * FN + i) * 32 + 8 * q + 4 * hi) >> 2;
                f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                *(f32x4*)(sC + prow * BN_ + ((chunk ^ (prow & 7)) << 2)) = v;
              }
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        RCDM_PRE_STORE_WAIT();
        const int mbase = cm0 + ps * RP;
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
          const int row = r0 + it * RPI;
          const int m = mbase + row;
          if (m < p.M && n < p.N) {
            const f32x4 v0 = *(const f32x4*)(sC + row * BN_ + (((2 * c8) ^ (row & 7)) << 2));
            const f32x4 v1 = *(const f32x4*)(sC + row * BN_ + (((2 * c8 + 1) ^ (row & 7)) << 2));
            if (p.slab16) {   // f16 slab (IgemmArgs::slab16): the same [split][M][N] planes, halfs
              Pack16 h;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                h.e[e] = (f16)v0[e];
                h.e[4 + e] = (f16)v1[e];
              }
              *(uint4*)((f16*)p.partial + ((size_t)blockIdx.y * p.M + m) * p.N + n) = h.u;
            } else {
              *(f32x4*)(dst + (size_t)m * p.N + n) = v0;
              *(f32x4*)(dst + (size_t)m * p.N + n + 4) = v1;
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    ++c_tile;
    post_epi = 2;
    if (c_tile < my_tiles) {
      tile_of(c_tile, cm0, cn0);
      if constexpr (LXC) lx_fetch(cm0, cn0);
    }
    if (p.trace) ts_epi += __builtin_amdgcn_s_memtime() - te0;
  }
  if (p.trace && t == 0) {
    long long* o = p.trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * TRACE_SLOTS;
    o[0] = ts0;
    o[1] = __builtin_amdgcn_s_memtime();
    o[2] = ts_epi;
    o[3] = my_tiles * nkl;
    if (TRACE_SLOTS == 8) {
      o[4] = ts_a;
      o[5] = ts_b;
      o[6] = ts_c;
      o[7] = my_tiles;
    }
  }
  (void)ts_loop; (void)ts_a; (void)ts_b; (void)ts_c; (void)tq;
}

// split-K second pass: fixed-order sum of the fp32 slabs + the epilogue (8 output columns per thread).
template <bool QG>   // QG: RCDM_EPI_QUICK_GELU launches
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const IgemmArgs p) {
  const bool geglu = (p.epi & RCDM_EPI_GEGLU) != 0;
  const int nout8 = (geglu ? p.N / 2 : p.N) / 8;
  const size_t total = (size_t)p.M * nout8;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(idx / nout8);
    const int oc = (int)(idx - (size_t)m * nout8) * 8;
    const int n = geglu ? (oc >> 4) * 32 + (oc & 15) : oc;
    float v[8], g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = g[e] = 0.f;
    for (int s = 0; s < p.splits; ++s) {
      const size_t off = ((size_t)s * p.M + m) * p.N + n;
      slab_add8(p, off, v);
      if (geglu) slab_add8(p, off + kGegluGroup, g);
    }
    epilogue_store<QG>(p, p.ph_rows ? phase_out_row(p, m) : m, n, v, g);   // (phase launches carry a bias at most: no per-row operand)
  }
}

// split-K second pass + the statistics pass of the GroupNorm that reads the result next (rcdm_*_gnstat): the grid, the
// thread -> (row, 16-byte chunk) mapping and the order of every addition are gn_stats_kernel's (norm.hip), so the partials —
// and with them the norm's output — are bit-identical to reduce + rcdm_groupnorm_silu.  Per element: the fixed-order sum of
// the fp32 slabs and the epilogue (what splitk_reduce_kernel does), the row stored as f16, and the statistics taken from the
// STORED halfs (what gn_stats_kernel would read back).  One launch and one read of the tensor less per norm.
// grid (gn_splits, gn_samples); block gn_CH * gn_RPB threads; no GEGLU, no phase rows (checked by the launcher).
__global__ __launch_bounds__(512) void splitk_reduce_gn_kernel(const IgemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* part = (float*)smem;
  const int t = threadIdx.x;
  const int ch = t % p.gn_CH, rl = t / p.gn_CH;
  const int s = blockIdx.y, sp = blockIdx.x;
  const int r_begin = sp * p.gn_rps;
  const int r_end = min(p.gn_P, r_begin + p.gn_rps);
  float S[8], Q[8], kp[8];   // shifted sums and their pivot (gn_plan.h): the thread's first STORED row, as gn_stats_kernel reads it
#pragma unroll
  for (int e = 0; e < 8; ++e) S[e] = Q[e] = kp[e] = 0.f;
  const int n = ch * 8;
  // GN_U rows per thread and pass, as in gn_stats_kernel (the split is sized so that this is normally the block's only pass):
  // per slab, the loads of all GN_U rows are requested before the first addition — `splits` round trips per pass
  for (int r = r_begin + rl; r < r_end; r += GN_U * p.gn_RPB) {
    float v[GN_U][8];
#pragma unroll
    for (int u = 0; u < GN_U; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
    // (both slabs of a split-2 launch requested together — 210 VGPRs — measured +0.06 ms per step against this form)
    for (int k = 0; k < p.splits; ++k) {
      if (p.slab16) {
        Pack16 h[GN_U];
#pragma unroll
        for (int u = 0; u < GN_U; ++u) {
          const int ru = min(r + u * p.gn_RPB, r_end - 1);
          h[u].u = *(const uint4*)((const f16*)p.partial + ((size_t)k * p.M + (size_t)s * p.gn_P + ru) * p.N + n);
        }
#pragma unroll
        for (int u = 0; u < GN_U; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) v[u][e] += (float)h[u].e[e];
        continue;
      }
      f32x4 a[GN_U], b[GN_U];
#pragma unroll
      for (int u = 0; u < GN_U; ++u) {
        const int ru = min(r + u * p.gn_RPB, r_end - 1);
        const float* src = p.partial + ((size_t)k * p.M + (size_t)s * p.gn_P + ru) * p.N + n;
        a[u] = *(const f32x4*)src;
        b[u] = *(const f32x4*)(src + 4);
      }
#pragma unroll
      for (int u = 0; u < GN_U; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[u][e] += a[u][e];
          v[u][4 + e] += b[u][e];
        }
    }
#pragma unroll
    for (int u = 0; u < GN_U; ++u) {
      const int ru = r + u * p.gn_RPB;
      if (ru < r_end) {
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // (GEGLU gates: never with statistics)
        Pack16 o;
        o.u = epilogue_store(p, s * p.gn_P + ru, n, v[u], g);
        if (u == 0 && r == r_begin + rl) {
#pragma unroll
          for (int e = 0; e < 8; ++e) kp[e] = (float)o.e[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) gn_acc(S[e], Q[e], (float)o.e[e], kp[e], true);
      }
    }
  }
  GnArgs ga{};
  ga.partial = p.gn_partial; ga.G = p.gn_G; ga.cg = p.gn_cg; ga.CH = p.gn_CH; ga.RPB = p.gn_RPB; ga.splits = p.gn_splits;
  gn_block_partials(ga, part, t, S, Q, kp, s, sp, r_end - r_begin);
}

// the reduce launch of a split-K GEMM / conv (every kernel family writes the same [split][M][N] fp32 slabs)
int launch_splitk_reduce(const IgemmArgs& a, hipStream_t stream) {
  if (a.gn_partial) {
    const int threads = a.gn_CH * a.gn_RPB;
    const size_t lds = (size_t)(threads + a.gn_CH) * 16 * sizeof(float);
    hipLaunchKernelGGL(splitk_reduce_gn_kernel, dim3(a.gn_splits, a.gn_samples), dim3(threads), lds, stream, a);
    return rcdm_check_launch();
  }
  const bool geglu = (a.epi & RCDM_EPI_GEGLU) != 0;
  const size_t total = (size_t)a.M * ((geglu ? a.N / 2 : a.N) / 8);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (a.epi & RCDM_EPI_QUICK_GELU) hipLaunchKernelGGL(splitk_reduce_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(splitk_reduce_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
  return rcdm_check_launch();
}

long long* g_trace = nullptr;

// The split-K slabs of a planned launch: a.partial points into the caller's workspace (null when the launch is not split)
int bind_slabs(IgemmArgs& a, void* workspace, size_t workspace_bytes) {
  a.partial = nullptr;
  if (a.splits > 1) {
    if (!workspace || workspace_bytes < slab_bytes(a)) return RCDM_EWORKSPACE;
    a.partial = (float*)workspace;
  }
  return RCDM_OK;
}

// "launch, then reduce if split": the tail behind every kernel family (rc: what the GEMM launch returned)
int reduce_if_split(int rc, const IgemmArgs& a, hipStream_t stream) {
  return (rc == RCDM_OK && a.splits > 1) ? launch_splitk_reduce(a, stream) : rc;
}

// The igemm_dma_kernel instantiations: (tile of the LDS-DMA family, what the launch's epilogue does) -> kernel, nullptr where
// kVariants says the tile cannot run it.  Every kernel pointer comes from here — for the one-time dynamic-LDS attribute pass
// and for the launch alike — so an instantiation cannot be launched without having had its attribute set (a missing one
// would fail only on the first launch that needs more than 64 KB on a fresh device).
enum DmaMode {
  kDmaFused,      // direct launch with the fused epilogue (E16 = true: f16 staging)
  kDmaSlab,       // split-K slab writer (E16 = false: fp32 staging)
  kDmaStats,      // GEMMs, LX = 1: fused epilogue + row statistics (deferred-LayerNorm producer)
  kDmaConsumer,   // GEMMs, LX = 2: deferred-LayerNorm consumer (+ statistics)
  kDmaQuickGelu,  // GEMMs, LX = 4: the quick-GELU epilogue
  kNumDmaModes
};
using DmaKernel = void (*)(const IgemmArgs);

template <int TAPS, int V>
DmaKernel dma_kernel_of(DmaMode mode) {
  constexpr VariantRow r = kVariants[V];
  static_assert(r.family == kFamDma, "not an igemm_dma_kernel tile");
  if constexpr (TAPS == 1 || !(r.cannot & kNoConv)) {
    if (mode == kDmaFused) return igemm_dma_kernel<TAPS, r.bm, r.bn, r.wm, r.wn, r.ring, true>;
    if (mode == kDmaSlab) return igemm_dma_kernel<TAPS, r.bm, r.bn, r.wm, r.wn, r.ring, false>;
  }
  if constexpr (TAPS == 1 && !(r.cannot & kNoStats))
    if (mode == kDmaStats) return igemm_dma_kernel<TAPS, r.bm, r.bn, r.wm, r.wn, r.ring, true, 1>;
  if constexpr (TAPS == 1 && !(r.cannot & kNoConsumer))
    if (mode == kDmaConsumer) return igemm_dma_kernel<TAPS, r.bm, r.bn, r.wm, r.wn, r.ring, true, 2>;
  if constexpr (TAPS == 1 && !(r.cannot & kNoQuickGelu))
    if (mode == kDmaQuickGelu) return igemm_dma_kernel<TAPS, r.bm, r.bn, r.wm, r.wn, r.ring, true, 4>;
  return nullptr;
}

template <int TAPS>
DmaKernel dma_kernel(int variant, DmaMode mode) {
  switch (variant) {
    case 0:
    case kVar128: return dma_kernel_of<TAPS, kVar128>(mode);
    case kVar256: return dma_kernel_of<TAPS, kVar256>(mode);
    case kVar64: return dma_kernel_of<TAPS, kVar64>(mode);
    case kVar64Deep: return dma_kernel_of<TAPS, kVar64Deep>(mode);
    case kVar128x64: return dma_kernel_of<TAPS, kVar128x64>(mode);
    case kVar128x64Deep: return dma_kernel_of<TAPS, kVar128x64Deep>(mode);
    default: return nullptr;   // (the other kernel families)
  }
}

template <int TAPS>
int launch_dma(IgemmArgs& a, int variant, hipStream_t stream) {
  const VariantRow& row = kVariants[variant];
  a.slab16 = a.splits > 1 && slab16_mode() && !(a.epi & RCDM_EPI_GEGLU);
  const int ntiles = a.tilesM * a.tilesN;
  int gx = rcdm_num_cus() * row.blocks_per_cu;
  if (a.splits > 1) gx = (gx + a.splits - 1) / a.splits;
  gx = (gx + 7) / 8 * 8;  // keep the b%8 -> XCD pattern aligned across the persistent stride
  static const int persist_mode = rcdm_env_int("RCDM_PERSIST", 1);  // RCDM_PERSIST=0: one tile per block (A/B switch); default: persistent blocks
  // (GEGLU launches used to run one tile per block: a persistent block had to drain its epilogue stores before it
  // could trust the next tile's DMA.  With the loads waited for BEFORE the stores that stall is gone.)
  if (persist_mode == 0) gx = ntiles;
  if (gx > ntiles) gx = ntiles;
  dim3 grid(gx, a.splits);
  // (statistics / consumer launches: TAPS == 1 and unsplit only, checked by launch<>)
  const DmaMode mode = a.lnx_stat ? kDmaConsumer : a.stat_out ? kDmaStats : a.splits > 1 ? kDmaSlab
                       : (TAPS == 1 && (a.epi & RCDM_EPI_QUICK_GELU)) ? kDmaQuickGelu : kDmaFused;
  // a conv on the three-slot 128x64 ring runs the two-slot kernel (in the grid planned for the variant asked for)
  const int kv = (TAPS != 1 && (row.cannot & kNoConv)) ? row.instead : variant;
  const DmaKernel kernel = dma_kernel<TAPS>(kv, mode);
  if (!kernel) return RCDM_ESHAPE;   // (fill_common plans no such launch)
  hipLaunchKernelGGL(kernel, grid, dim3(kVariants[kv].threads()), kVariants[kv].lds_bytes(), stream, a);
  return rcdm_check_launch();
}

template <int TAPS>
int launch(IgemmArgs& a, int variant, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const VariantRow& row = kVariants[variant];
  static bool attr_set[64] = {};
  if (rcdm_first_on_device(attr_set))
    for (int v = 1; v < kNumVariants; ++v)
      for (int m = 0; m < kNumDmaModes; ++m)
        if (const DmaKernel k = dma_kernel<TAPS>(v, (DmaMode)m))
          (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, kVariants[v].lds_bytes());
  int rc = bind_slabs(a, workspace, workspace_bytes);
  if (rc) return rc;
  a.trace = g_trace;
  a.dbg = 0;
  if (a.stat_out && (row.family != kFamDma || a.splits > 1 || (a.epi & RCDM_EPI_GEGLU) || a.stat_parts != a.tilesN))
    return RCDM_ESHAPE;
  if ((a.stat_out || a.lnx_stat) && TAPS != 1) return RCDM_ESHAPE;
  if (a.lnx_stat && (a.splits > 1 || !a.lnx_S || a.lnx_parts < 1 || a.lnx_parts > kLnxMaxParts)) return RCDM_ESHAPE;
  if (a.lnx_stat && (row.cannot & kNoConsumer)) return RCDM_ESHAPE;   // the 256x256 ping-pong tile has no consumer epilogue (register cap); only reachable when that variant is forced
  if (row.family == kFam160) {
    a.slab16 = a.splits > 1 && slab16_mode() && !(a.epi & RCDM_EPI_GEGLU);
    rc = rcdm_igemm16_launch(a, TAPS, stream);
  } else if (row.family == kFamPP) {
    static const int rotate = rcdm_env_int("RCDM_PP_ROTATE", 0);   // measured: no gain (the weight stream is not hot-spotting L2 channels)
    a.dbg = rotate ? 8 : 0;
    rc = rcdm_igemm_pp_launch(a, TAPS, variant - kVarPP, stream);
  } else {
    rc = launch_dma<TAPS>(a, variant, stream);
  }
  return reduce_if_split(rc, a, stream);
}

// the operands of a planned launch, and the checks that need them
int bind_operands(IgemmArgs& a, const void* A, const void* W, const float* bias, const float* rowvec, const void* residual,
                  void* out) {
  a.A = (const f16*)A; a.W = (const f16*)W; a.bias = bias; a.rowvec = rowvec;
  a.res = (const f16*)residual; a.out = (f16*)out;
  return check_common(a);
}

// the plain (upsample 0 | 1) conv launch behind rcdm_conv3x3 / _add1x1 / _gnstat / _add1x1_gnstat; gn: the norm whose
// partial statistics the split-K reduce leaves (nullptr: none)
int conv_launch(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const void* in, const void* in2, const void* W,
                const float* bias, const float* rowvec, const void* residual, void* out, void* workspace,
                size_t workspace_bytes, void* gn_workspace, size_t gn_workspace_bytes, void* stream) {
  IgemmArgs a{};
  int variant = 0;
  int rc = plan_conv(d, a, variant);
  if (rc) return rc;
  a.A2 = (const f16*)in2;
  rc = bind_operands(a, in, W, bias, rowvec, residual, out);
  if (rc) return rc;
  if (a.epi & (RCDM_EPI_GEGLU | RCDM_EPI_QUICK_GELU)) return RCDM_ESHAPE;
  if (gn) {
    rc = attach_gnstat(a, gn, gn_workspace, gn_workspace_bytes, true);
    if (rc) return rc;
  }
  return launch<9>(a, variant, workspace, workspace_bytes, (hipStream_t)stream);
}

// Launch geometry the library chooses for a shape (diagnostics: tools/ceiling.py prices tile quantisation with it): out[8] =
// {tile variant, BM, BN, row tiles, column tiles, split-K factor, resident blocks per CU of that tile, k-steps of 64}.
void plan_out(const IgemmArgs& a, int variant, int32_t* out) {
  out[0] = variant; out[1] = kVariants[variant].bm; out[2] = kVariants[variant].bn; out[3] = a.tilesM; out[4] = a.tilesN;
  out[5] = a.splits; out[6] = kVariants[variant].blocks_per_cu; out[7] = a.nk;
}

}  // namespace

extern "C" {

int rcdm_debug_set_igemm_trace(void* device_buffer) {
  g_trace = (long long*)device_buffer;
  return RCDM_OK;
}

size_t rcdm_gemm_workspace_bytes(const rcdm_gemm_desc* d) {
  IgemmArgs a{};
  int variant = 0;
  return plan_gemm(d, PlanFlags{}, a, variant) ? 0 : slab_bytes(a);
}

size_t rcdm_gemm_lnx_workspace_bytes(const rcdm_gemm_desc* d, int32_t producer, int32_t consumer) {
  IgemmArgs a{};
  int variant = 0;
  return plan_gemm(d, PlanFlags{producer != 0, consumer != 0}, a, variant) ? 0 : slab_bytes(a);
}

int rcdm_gemm(const rcdm_gemm_desc* d, const void* A, const void* W, const float* bias, const float* rowvec,
              const void* residual, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  IgemmArgs a{};
  int variant = 0;
  int rc = plan_gemm(d, PlanFlags{}, a, variant);
  if (!rc) rc = bind_operands(a, A, W, bias, rowvec, residual, out);
  if (rc) return rc;
  return launch<1>(a, variant, workspace, workspace_bytes, (hipStream_t)stream);
}

int rcdm_gemm_gnstat_ok(const rcdm_gemm_desc* d, const rcdm_groupnorm_desc* gn) {
  IgemmArgs a{};
  int variant = 0;
  if (!gn || plan_gemm(d, PlanFlags{}, a, variant)) return 0;
  return attach_gnstat(a, gn, nullptr, 0, false) == RCDM_OK;
}

int rcdm_gemm_gnstat(const rcdm_gemm_desc* d, const rcdm_groupnorm_desc* gn, const void* A, const void* W, const float* bias,
                     const float* rowvec, const void* residual, void* out, void* workspace, size_t workspace_bytes,
                     void* gn_workspace, size_t gn_workspace_bytes, void* stream) {
  IgemmArgs a{};
  int variant = 0;
  int rc = plan_gemm(d, PlanFlags{}, a, variant);
  if (!rc) rc = bind_operands(a, A, W, bias, rowvec, residual, out);
  if (!rc) rc = attach_gnstat(a, gn, gn_workspace, gn_workspace_bytes, true);
  if (rc) return rc;
  return launch<1>(a, variant, workspace, workspace_bytes, (hipStream_t)stream);
}

int rcdm_gemm_stat_parts(const rcdm_gemm_desc* d) { return rcdm_gemm_lnx_stat_parts(d, 0); }

// the tile choice of a statistics-producing launch; the consumer flag the launch will carry steers it too
int rcdm_gemm_lnx_stat_parts(const rcdm_gemm_desc* d, int32_t consumer) {
  IgemmArgs a{};
  int variant = 0;
  if (plan_gemm(d, PlanFlags{true, consumer != 0}, a, variant)) return 0;
  return a.splits > 1 ? 0 : a.tilesN;
}

int rcdm_gemm_lnx(const rcdm_gemm_desc* d, const rcdm_lnx* x, const void* A, const void* W, const float* bias,
                  const float* rowvec, const void* residual, void* out, void* workspace, size_t workspace_bytes,
                  void* stream) {
  if (!d || !x) return RCDM_EINVAL;
  IgemmArgs a{};
  from_gemm(d, a);   // (the operand and statistics checks come first, as they always did: plan_gemm fills the shape again)
  int rc = bind_operands(a, A, W, bias, rowvec, residual, out);
  if (rc) return rc;
  if (a.epi & RCDM_EPI_QUICK_GELU) return RCDM_ESHAPE;
  if (x->stat_out) {
    if (x->stat_parts <= 0 || ((uintptr_t)x->stat_out & 7)) return RCDM_EINVAL;
    a.stat_out = x->stat_out;
    a.stat_parts = x->stat_parts;
    a.stat_ld = x->stat_out_rows;
    if (a.stat_ld < a.M + d->dup_rows) return RCDM_EINVAL;
  }
  if (x->stat_in) {
    if (!x->colsum || x->parts_in <= 0 || x->C <= 0 || ((uintptr_t)x->stat_in & 7) || ((uintptr_t)x->colsum & 15)) return RCDM_EINVAL;
    if (x->parts_in > kLnxMaxParts) return RCDM_ESHAPE;
    a.lnx_stat = x->stat_in; a.lnx_S = x->colsum; a.lnx_parts = x->parts_in; a.lnx_ld = x->stat_in_rows;
    if (a.lnx_ld < a.M) return RCDM_EINVAL;
    a.lnx_invC = 1.0f / (float)x->C; a.lnx_eps = x->eps;
    // the producer's column-tile width, which the consumer's merge needs for the slots' column counts: with two slots or
    // more ceil(C / 64), ceil(C / 128) and ceil(C / 256) differ, so the slot count names the width
    int bn = x->parts_in == 1 ? x->C : 0;
    for (int w = 64; w <= 256 && !bn; w *= 2)
      if ((x->C + w - 1) / w == x->parts_in) bn = w;
    if (!bn) return RCDM_ESHAPE;
    const int last = x->C - (x->parts_in - 1) * bn;
    a.lnx_geo = LnxGeo{(float)bn, 1.0f / (float)bn, (float)last, 1.0f / (float)last};
  }
  // the flags the launch carries, and a producer's slot count (the caller's, where an LDS-DMA tile has it: rcdm_gemm_lnx_parts_ok)
  int variant = 0;
  rc = plan_gemm(d, PlanFlags{a.stat_out != nullptr, a.lnx_stat != nullptr, a.stat_parts}, a, variant);
  if (rc) return rc;
  return launch<1>(a, variant, workspace, workspace_bytes, (hipStream_t)stream);
}

int rcdm_gemm_lnx_parts_ok(const rcdm_gemm_desc* d, int32_t parts, int32_t consumer) {
  if (!d || parts <= 0 || (d->epilogue & RCDM_EPI_GEGLU)) return 0;
  IgemmArgs a{};
  int variant = 0;
  if (plan_gemm(d, PlanFlags{true, consumer != 0, parts}, a, variant)) return 0;   // no tile has that slot count
  // (a split plan that has the count: the answer is, as it always was, whether an unsplit LDS-DMA tile has it too)
  return a.splits == 1 || variant_for_parts(a, parts) >= 0;
}

int rcdm_gemm_ln(const rcdm_gemm_desc* d, const rcdm_ln_fuse* ln, const void* A, const void* W, const float* bias,
                 const void* residual, void* out, void* stream) {
  if (!d || !ln || !ln->gamma || !ln->beta || !ln->out) return RCDM_EINVAL;
  if (ln->pe && (ln->rows_per_frame <= 0 || ln->frames <= 0)) return RCDM_EINVAL;
  IgemmArgs a{};
  from_gemm(d, a);
  int rc = bind_operands(a, A, W, bias, nullptr, residual, out);
  if (rc) return rc;
  // one 160x320 ping-pong tile must span the output row; only the plain epilogues
  if (a.N > kPPShapes[0].bn || (ln->ld & 7) || d->split_k > 1) return RCDM_ESHAPE;
  if (a.epi & (RCDM_EPI_GEGLU | RCDM_EPI_GELU | RCDM_EPI_QUICK_GELU | RCDM_EPI_ROWVEC)) return RCDM_ESHAPE;
  a.tilesM = (a.M + kPPShapes[0].bm - 1) / kPPShapes[0].bm;
  a.tilesN = 1;
  a.kc = (a.Cin + BK - 1) / BK;
  a.nk = a.kc;
  a.splits = 1;
  a.nk_per_split = a.nk;
  a.partial = nullptr;
  a.trace = nullptr;
  a.dbg = 0;
  a.epi |= kEpiLN;
  a.ln_g = ln->gamma; a.ln_b = ln->beta; a.ln_pe = ln->pe; a.ln_out = (f16*)ln->out; a.ln_ld = ln->ld;
  a.ln_rpf = ln->pe ? ln->rows_per_frame : 1; a.ln_frames = ln->pe ? ln->frames : 1; a.ln_eps = ln->eps;
  return rcdm_igemm_pp_launch(a, 1, 0, (hipStream_t)stream);
}

int rcdm_conv3x3_up2_supported(const rcdm_conv3x3_desc* d) {
  IgemmArgs a{};
  int variant = 0;
  return d && d->upsample == 2 && plan_conv(d, a, variant) == RCDM_OK;
}

size_t rcdm_conv3x3_workspace_bytes(const rcdm_conv3x3_desc* d) {
  if (!d) return 0;
  if (d->upsample == 2 && d->c_in2) return 0;   // (no phase form with a second input: every launch entry refuses the pair)
  IgemmArgs a{};
  int variant = 0;
  return plan_conv(d, a, variant) ? 0 : slab_bytes(a);
}

int rcdm_conv3x3(const rcdm_conv3x3_desc* d, const void* in, const void* W, const float* bias, const float* rowvec,
                 const void* residual, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d) return RCDM_EINVAL;
  if (d->c_in2) return RCDM_EINVAL;   // (a descriptor of rcdm_conv3x3_add1x1 — refused in every form, the phase form included)
  if (d->upsample == 2) {
    IgemmArgs a{};
    int variant = 0;
    int rc = plan_conv(d, a, variant);
    if (rc) return rc;
    if (!in || !W || !out || ((a.epi & RCDM_EPI_BIAS) && !bias)) return RCDM_EINVAL;
    if ((a.N & 7) || (a.lda & 7) || (a.ldc & 7) || (size_t)a.ph_rows * (size_t)a.lda * 2 >= 0x7FFFFFFFull) return RCDM_ESHAPE;
    a.A = (const f16*)in; a.W = (const f16*)W; a.bias = bias; a.out = (f16*)out;
    a.trace = nullptr;
    a.dbg = 0;
    rc = bind_slabs(a, workspace, workspace_bytes);
    if (rc) return rc;
    // (a phase launch has no GEGLU, no quick-GELU and no gn_partial: the plain reduce kernel over M x N / 8 threads)
    return reduce_if_split(rcdm_igemm_pp_launch(a, 4, variant - kVarPP, (hipStream_t)stream), a, (hipStream_t)stream);
  }
  return conv_launch(d, nullptr, in, nullptr, W, bias, rowvec, residual, out, workspace, workspace_bytes, nullptr, 0, stream);
}

int rcdm_gemm_plan_query(const rcdm_gemm_desc* d, int32_t producer, int32_t consumer, int32_t* out8) {
  IgemmArgs a{};
  int variant = 0;
  if (!out8 || plan_gemm(d, PlanFlags{producer != 0, consumer != 0}, a, variant)) return RCDM_EINVAL;
  plan_out(a, variant, out8);
  return RCDM_OK;
}

int rcdm_conv3x3_plan_query(const rcdm_conv3x3_desc* d, int32_t* out8) {
  if (!d || !out8) return RCDM_EINVAL;
  IgemmArgs a{};
  int variant = 0;
  if (plan_conv(d, a, variant)) return d->upsample == 2 ? RCDM_ESHAPE : RCDM_EINVAL;
  plan_out(a, variant, out8);
  return RCDM_OK;
}

int rcdm_conv3x3_add1x1(const rcdm_conv3x3_desc* d, const void* in, const void* in2, const void* W, const float* bias,
                        const float* rowvec, const void* residual, void* out, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!d || d->upsample == 2 || d->c_in2 <= 0 || !in2) return RCDM_EINVAL;
  return conv_launch(d, nullptr, in, in2, W, bias, rowvec, residual, out, workspace, workspace_bytes, nullptr, 0, stream);
}

int rcdm_conv3x3_gnstat_ok(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn) {
  if (!d || !gn || d->upsample == 2) return 0;
  IgemmArgs a{};
  int variant = 0;
  if (plan_conv(d, a, variant)) return 0;
  return attach_gnstat(a, gn, nullptr, 0, false) == RCDM_OK;
}

int rcdm_conv3x3_gnstat(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const void* in, const void* W,
                        const float* bias, const float* rowvec, const void* residual, void* out, void* workspace,
                        size_t workspace_bytes, void* gn_workspace, size_t gn_workspace_bytes, void* stream) {
  if (!d || !gn) return RCDM_EINVAL;
  if (d->upsample == 2) return RCDM_ESHAPE;
  if (d->c_in2) return RCDM_EINVAL;
  return conv_launch(d, gn, in, nullptr, W, bias, rowvec, residual, out, workspace, workspace_bytes, gn_workspace,
                     gn_workspace_bytes, stream);
}

int rcdm_conv3x3_add1x1_gnstat(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const void* in, const void* in2,
                               const void* W, const float* bias, const float* rowvec, const void* residual, void* out,
                               void* workspace, size_t workspace_bytes, void* gn_workspace, size_t gn_workspace_bytes,
                               void* stream) {
  if (!d || !gn || d->upsample == 2 || d->c_in2 <= 0 || !in2) return RCDM_EINVAL;
  return conv_launch(d, gn, in, in2, W, bias, rowvec, residual, out, workspace, workspace_bytes, gn_workspace,
                     gn_workspace_bytes, stream);
}

}  // extern "C"
