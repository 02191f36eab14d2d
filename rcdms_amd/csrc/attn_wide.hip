// attn_wide.hip — flash attention for wide heads, 160 < d <= 512 (d % 64 == 0), on MFMA for gfx950.
//
// The shape that matters is the ONE 512-channel head of the SD-1.5 VAE mid block (diffusers AutoencoderKL: UNetMidBlock2D
// attention over all h*w latent pixels of an image), which rcdms_amd/vae.py otherwise runs as Q K^T GEMM -> row softmax ->
// P V GEMM with an hw x hw score buffer in HBM.  flash_attn_kernel (attn.hip) keeps 2 x 32 queries' Q fragments and O^T
// accumulators of a wave in half a register file; at d = 512 one set alone is 128 + 256 registers, so this is its own
// kernel with its own budget:
//
//   block = 4 waves (ONE per SIMD, the whole 512-entry VGPR + AGPR file each) x 32 queries = 128 queries
//   per wave   Q fragments      d/16 x f16x8   = d/4 registers (128 at d = 512)
//              O^T accumulator  d/32 x f32x16  = d/2 registers (256 at d = 512; they end up in the AGPR half)
//              S^T of a tile    f32x16, P f16 8 registers, K / V staging d/16 registers
//   key tile   32 keys; K and V row-major in ping-pong LDS images, 2 x 32 x (d + 8) + 2 x 32 x (d + 32) halfs = 133 KiB at
//              d = 512: one block per CU
//
// As in attn.hip the scores are computed transposed, S^T = K Q^T (v_mfma_f32_32x32x16_f16: keys = rows, queries = columns),
// so a lane owns one query: max / sum / rescale are lane-local plus one exchange with lane ^ 32, and the f16-rounded P
// registers are the B operand of O^T += V^T P^T as they stand.  The A operand of that product is read from the row-major V
// image with ds_read_b64_tr_b16 in the key order the S^T registers hold P.
// LDS traffic: every wave reads the whole K tile (one ds_read_b128 per MFMA) and the whole V tile (two transpose reads per
// MFMA); four waves do that at half the 256 B/clk of the LDS array per 32-cycle MFMA, so the matrix pipe is what binds.
// Row strides: K rows of d + 8 halfs put the 16 rows of a ds_read_b128 lane group into 16 different 4-bank slots (dword
// stride = 4 mod 32, an odd multiple of 4 banks), V rows of d + 32 halfs put the four key rows of a transpose read's lane
// half into four different 16-bank slots (dword stride = 16 mod 32): both reads are conflict-free.
// Softmax: fp32 max / sum / O; p = exp2(s * scale * log2(e) - m), rounded to f16 once (v_cvt_pkrtz) and the row sum taken
// from the ROUNDED values, so numerator and denominator of O / l carry the same P.
// The reference m of a query is FIXED for a whole pass over the keys — the row max of the first key tile — instead of a
// running max with an O *= 2^(m_old - m_new) rescale: any VALU use of the loop-carried accumulators makes hipcc carry all of
// them in VGPRs and copy every fragment into AGPRs in front of its MFMAs, which at d = 512 is the register file twice
// (hundreds of spills; multiplying through asm statements or inside the P V loop does not change that).  With a fixed
// reference the accumulators are touched by MFMAs only.  P stays finite in f16 while a query's scaled scores stay within
// 2^15 = e^10.4 of that first-tile max (P <= 2^15, and the row's largest P is >= 1, so nothing underflows that a running
// max would keep).  Every query tracks its true max on the side; if one leaves the window (a dominant key in a late
// tile, logits in the hundreds), the block runs the key loop a second time with the exact row max of the first pass as
// reference (P <= 1).  The result is the same softmax either way: m cancels in O / l.
#include "attn_wide.h"

namespace {

constexpr int KT = 32;   // keys per tile
constexpr int NT = 256;  // threads per block: 4 waves
constexpr float P_WINDOW = 15.0f;  // log2 of the largest P a pass may produce (f16: 65504 < 2^16)

typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
// gfx950 LDS transpose read: every 16-lane group reads a [4 keys][16 columns] f16 block (lane i supplies the address
// of row i/4, columns 4(i%4)..+3) and lane i receives column i of that block, i.e. 4 keys of one head-dim column.
__device__ __forceinline__ s16x4 lds_read_tr16(const f16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

__host__ __device__ constexpr int k_row_halfs(int ND) { return 64 * ND + 8; }
__host__ __device__ constexpr int v_row_halfs(int ND) { return 64 * ND + 32; }
__host__ __device__ constexpr size_t lds_bytes(int ND) { return (size_t)2 * KT * (k_row_halfs(ND) + v_row_halfs(ND)) * sizeof(f16); }

template <int ND>  // head dim = 64 ND
__global__ __launch_bounds__(NT, 1) void flash_attn_wide_kernel(const AttnWideArgs p) {
  constexpr int D = 64 * ND;
  constexpr int DS = 4 * ND;      // 16-wide k-steps of Q K^T
  constexpr int DF = 2 * ND;      // 32-row fragments of O^T
  constexpr int DCH = 8 * ND;     // 16-B chunks per K / V row
  constexpr int NSLOT = KT * DCH / NT;  // chunks a thread stages per tile (K and V each) = ND
  static_assert(KT * DCH % NT == 0, "every thread stages the same number of chunks");
  constexpr int KP = k_row_halfs(ND), VR = v_row_halfs(ND);
  constexpr int SK = KT * KP, SV = KT * VR;
  constexpr int BQ = 4 * 32;
  constexpr int QG = 2;           // Q K^T k-steps per operand-read group (DS = 4 ND is a multiple)
  constexpr int PG = 1;           // O^T fragments (x 2 key steps) per operand-read group
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f16* sK = (f16*)smem;   // [2][KT][KP]
  f16* sV = sK + 2 * SK;  // [2][KT][VR]  row-major, read transposed

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 31, hi = lane >> 5;
  // XCD-aware block order (as flash_attn_kernel): block `lin` runs on XCD lin % 8, each XCD takes a contiguous run of the
  // (batch, head, query block) sequence, so the query blocks that stream the same K / V share one L2
  const int nqb = (p.Lq + BQ - 1) / BQ;
  int item;
  {
    const int total = nqb * p.heads * p.batch, lin = blockIdx.x;
    const int xcd = lin & 7, q = total >> 3, r = total & 7;
    item = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
    if (p.plain_order) item = lin;
  }
  const int qb = item % nqb, bh = item / nqb;
  const int h = bh % p.heads, b = bh / p.heads;
  const int q0 = qb * BQ + wave * 32 + lr;

  // Q fragments: row q0, columns 16 s + 8 hi .. + 7.  Raw buffer loads, a query past Lq sent out of range (reads as zero):
  // one address register and no branch per fragment
  f16x8 qf[DS];
  {
    const f16* Qb = p.Q + (size_t)b * p.Lq * p.ldq + h * D;
    const __amdgpu_buffer_rsrc_t rQ = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Qb, 0, (int)(((size_t)(p.Lq - 1) * p.ldq + D) * 2), 0x00020000);
    const unsigned q_off = q0 < p.Lq ? (unsigned)(q0 * p.ldq + hi * 8) * 2u : 0x80000000u;
#pragma unroll
    for (int s = 0; s < DS; ++s) {
      Pack16 v;
      v.v = __builtin_amdgcn_raw_buffer_load_b128(rQ, q_off + 32u * s, 0, 0);
      qf[s] = v.h;
    }
  }
  f32x16 oacc[DF];
  float l_run = 0.f;

  // ---- staging: 8 adjacent lanes move 128 contiguous bytes of ONE key row, thread t the chunks (t & 7) + 8 sl of key
  // t >> 3, so the NSLOT pieces of a thread differ by compile-time offsets (128 B in memory and in LDS) and one address
  // register each serves K and V.  Raw buffer loads: keys past Lk (the ragged last tile, and the tile the loop fetches
  // past the end) fall outside num_records and read as zero
  const f16* Kb = p.K + (size_t)b * p.Lk * p.ldk + h * D;
  const f16* Vb = p.V + (size_t)b * p.Lk * p.ldv + h * D;
  const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(
      (void*)Kb, 0, (int)(((size_t)(p.Lk - 1) * p.ldk + D) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)Vb, 0, (int)(((size_t)(p.Lk - 1) * p.ldv + D) * 2), 0x00020000);
  static_assert(NT / 8 == KT && NSLOT == ND, "one key row per 8 lanes");
  const int st_key = t >> 3, st_c = (t & 7) * 8;
  const int k_lds = st_key * KP + st_c, v_lds = st_key * VR + st_c;
  // byte offsets of the NEXT K / V tile to fetch; they stay below 2^31: (Lk + 4 * 64) * ld * 2 < 2^31 (dispatcher)
  const unsigned k_off0 = (unsigned)(st_key * p.ldk + st_c) * 2u, v_off0 = (unsigned)(st_key * p.ldv + st_c) * 2u;
  unsigned k_off = k_off0, v_off = v_off0;
  const unsigned k_step = (unsigned)(KT * p.ldk) * 2u, v_step = (unsigned)(KT * p.ldv) * 2u;
  Pack16 kreg[NSLOT], vreg[NSLOT];
  auto fetch_k = [&]() {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) kreg[sl].v = __builtin_amdgcn_raw_buffer_load_b128(rK, k_off + 128u * sl, 0, 0);
    k_off += k_step;
  };
  auto fetch_v = [&]() {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) vreg[sl].v = __builtin_amdgcn_raw_buffer_load_b128(rV, v_off + 128u * sl, 0, 0);
    v_off += v_step;
  };
  auto put_k = [&](int par) {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) *(uint4*)(sK + par * SK + k_lds + 64 * sl) = kreg[sl].u;
  };
  auto put_v = [&](int par) {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) *(uint4*)(sV + par * SV + v_lds + 64 * sl) = vreg[sl].u;
  };
  // K fragment of a lane: key row lr, columns 16 s + 8 hi .. + 7
  const int k_rd = lr * KP + hi * 8;
  // transposed V fragment base: lane (hi, column half ch, i) addresses key row 4 hi + i/4, columns 16 ch + 4 (i%4)
  const int v_rd = (4 * hi + ((lane & 15) >> 2)) * VR + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  // ---- pipeline: ONE barrier per tile.  Iteration kt reads the images `par` (written in iteration kt - 1, or in the
  // prologue) and writes tile kt + 1 into the images `par ^ 1`, whose last readers (iteration kt - 1) are all behind the
  // barrier that opens iteration kt.  The K fetch flies under the Q K^T MFMAs, the V fetch under the P V MFMAs.
  const int ntiles = (p.Lk + KT - 1) / KT;
  float m_ref = 0.f;  // this query's softmax reference: first-tile max (pass 0) or exact row max (pass 1)
#pragma clang loop unroll(disable)
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int f = 0; f < DF; ++f)
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[f][e] = 0.f;
    l_run = 0.f;
    float m_seen = -INFINITY;
    k_off = k_off0;
    v_off = v_off0;
    fetch_k();
    put_k(0);  // (pass 1: the last readers of these images are behind the barrier of the window vote below)
    __builtin_amdgcn_sched_barrier(0);  // (K and V share the staging registers)
    fetch_v();
    put_v(0);
    for (int kt = 0; kt < ntiles; ++kt) {
      const int par = kt & 1, kbase = kt * KT;
      __syncthreads();
      fetch_k();  // K(kt + 1)
      // S^T = K Q^T: one accumulation chain over the d/16 k-steps
      f32x16 sacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
      // operand reads run one group of MFMAs ahead (fragments of group g + 1 requested before the MFMAs of group g); the
      // scheduling fences keep hipcc from hoisting ALL of a tile's fragment reads — d/4 registers — above the first MFMA
      const f16* kp = sK + par * SK + k_rd;
      f16x8 kf[2][QG];
#pragma unroll
      for (int i = 0; i < QG; ++i) kf[0][i] = *(const f16x8*)(kp + i * 16);
      const f16* vb = sV + par * SV + v_rd;
#pragma unroll
      for (int g = 0; g < DS / QG; ++g) {
        if (g + 1 < DS / QG) {
#pragma unroll
          for (int i = 0; i < QG; ++i) kf[(g + 1) & 1][i] = *(const f16x8*)(kp + ((g + 1) * QG + i) * 16);
        }
#pragma unroll
        for (int i = 0; i < QG; ++i)
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[g & 1][i], qf[g * QG + i], sacc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the first V fragments are requested before the softmax (the V image of this tile is behind the same barrier)
      union VFrag { s16x4 h[2]; f16x8 v; };
      VFrag vf[2][2 * PG];
      auto read_v = [&](int g, VFrag (&dst)[2 * PG]) {
#pragma unroll
        for (int i = 0; i < 2 * PG; ++i) {
          const f16* vp = vb + (16 * (i & 1)) * VR + 32 * (g * PG + (i >> 1));
          dst[i].h[0] = lds_read_tr16(vp);
          dst[i].h[1] = lds_read_tr16(vp + 8 * VR);
        }
      };
      read_v(0, vf[0]);

      // ---- softmax: the lane holds, for its query, keys kbase + (r&3) + 8 (r>>2) + 4 hi
      if (kbase + KT > p.Lk) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kbase + (r & 3) + 8 * (r >> 2) + 4 * hi >= p.Lk) sacc[r] = -INFINITY;
      }
      float mx = sacc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float cand = mx * p.c;  // every tile has >= 1 valid key: finite
      if (pass == 0 && kt == 0) m_ref = cand;
      m_seen = fmaxf(m_seen, cand);
      f16x8 pf[2];
      float lsum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[r], p.c, -m_ref));
        const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[r + 1], p.c, -m_ref));
        const auto pk = __builtin_amdgcn_cvt_pkrtz(p0, p1);  // v_cvt_pkrtz_f16_f32
        lsum += (float)pk[0] + (float)pk[1];                 // the sum of what the P V product will see
        pf[r >> 3][r & 7] = (f16)pk[0];
        pf[r >> 3][(r & 7) + 1] = (f16)pk[1];
      }
      l_run += lsum;

      put_k(par ^ 1);
      __builtin_amdgcn_sched_barrier(0);  // (the V fetch must not rise above the K stores: they share the staging registers)
      fetch_v();  // V(kt + 1)
      // ---- O^T += V^T P^T: 2 steps of 16 keys per 32-row fragment.  The A fragment (head-dim rows x 8 keys per lane) is
      // two transpose reads of the row-major V image: keys 16 st + 4 hi + {0..3} and + 8 + {0..3}, the order P holds
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < DF / PG; ++g) {
        if (g + 1 < DF / PG) read_v(g + 1, vf[(g + 1) & 1]);
#pragma unroll
        for (int i = 0; i < 2 * PG; ++i) {
          const int f = g * PG + (i >> 1);
          oacc[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[g & 1][i].v, pf[i & 1], oacc[f], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      put_v(par ^ 1);
    }
    // window vote (block-wide: the waves share the K / V images and their barriers).  Pass 1 ran on the exact row max
    if (pass == 1 || !__syncthreads_or(m_seen > m_ref + P_WINDOW)) break;
    m_ref = m_seen;
  }

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  // O^T fragment f, register 4 g + i: head-dim row 32 f + 8 g + 4 hi + i of this lane's query.  Raw buffer stores, a query
  // past Lq sent out of range (dropped): no branch, so the fences below hold and the accumulators leave the AGPRs one
  // fragment at a time (behind a branch hipcc reads all d/2 of them into VGPRs first)
  {
    f16* Ob = p.O + (size_t)b * p.Lq * p.ldo + h * D;
    const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Ob, 0, (int)(((size_t)(p.Lq - 1) * p.ldo + D) * 2), 0x00020000);
    const unsigned o_off = q0 < p.Lq ? (unsigned)(q0 * p.ldo + 4 * hi) * 2u : 0x80000000u;
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int f = 0; f < DF; ++f) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        union { f16x4 h; u32x2_t u; } o;
        o.h = f16x4{(f16)(oacc[f][4 * g] * inv), (f16)(oacc[f][4 * g + 1] * inv),
                    (f16)(oacc[f][4 * g + 2] * inv), (f16)(oacc[f][4 * g + 3] * inv)};
        __builtin_amdgcn_raw_buffer_store_b64(o.u, rO, o_off + (unsigned)(f * 32 + 8 * g) * 2u, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int ND>
int launch_wide(const AttnWideArgs& a, hipStream_t stream) {
  constexpr size_t lds = lds_bytes(ND);
  static_assert(lds <= 160 * 1024, "LDS per block");
  static bool attr_done[64] = {};
  if (rcdm_first_on_device(attr_done))
    (void)hipFuncSetAttribute((const void*)flash_attn_wide_kernel<ND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const dim3 grid((unsigned)(((a.Lq + 127) / 128) * a.heads * a.batch));
  hipLaunchKernelGGL(flash_attn_wide_kernel<ND>, grid, dim3(NT), lds, stream, a);
  return rcdm_check_launch();
}

}  // namespace

int rcdm_attn_wide_launch(const AttnWideArgs& a, hipStream_t stream) {
  switch (a.d) {
    case 192: return launch_wide<3>(a, stream);
    case 256: return launch_wide<4>(a, stream);
    case 320: return launch_wide<5>(a, stream);
    case 384: return launch_wide<6>(a, stream);
    case 448: return launch_wide<7>(a, stream);
    case 512: return launch_wide<8>(a, stream);
  }
  return RCDM_ESHAPE;
}
