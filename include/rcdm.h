/*
 * rcdm.h — C-ABI of librcdm_hip.so: the MI355X (gfx950) kernels underneath the RCDMs stage-2
 * denoiser (UNet3DConditionModel.forward + the CFG/DDIM loop).
 *
 * The reference (muzishen/RCDMs) has NO FFI of its own: every op on this path is a torch/ATen call
 * made from Python.  Each entry point below therefore names the reference Python call site(s) it
 * replaces (paths relative to the reference repo).  All functions:
 *   - take plain device pointers + sizes (no torch types), caller-owned buffers, an explicit
 *     hipStream_t (passed as void*), never allocate, never synchronise, are graph-capturable;
 *   - return 0 on success, a negative RCDM_E* code otherwise (never throw);
 *   - compute in fp16 storage / fp32 accumulate ("f16" below = IEEE binary16).
 *
 * Activation layout everywhere: channels-last rows.  A tensor the reference holds as
 * (b, C, f, H, W) is one row-major matrix X[M][ld] with M = b*f*H*W rows ordered (b, f, y, x) and C
 * contiguous channels per row; `ld` (>= C, multiple of 8) lets a tensor live inside a wider
 * "concat" buffer so torch.cat([h, skip], dim=1) (unet_blocks.py:644,754) costs nothing.
 */
#ifndef RCDM_H
#define RCDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCDM_VERSION 0x000300 /* 0.3.0: + rcdm_conv3x3_wino*, rcdm_groupnorm_stats_prestat / _finalize (no descriptor changed) */
/* ABI rule: every descriptor struct below MUST be zero-initialised by the caller (memset / `= {0}` / calloc) before its
 * fields are set.  Descriptors grow at the END between versions and a zero in a field this header does not describe yet
 * always means "the behaviour of the previous version": 0.2.0 added rcdm_conv3x3_desc.c_in2 / lda2 (rcdm_conv3x3_add1x1)
 * and rcdm_attn_desc.flags (RCDM_ATTN_WIDE_RANGE) — a caller compiled against 0.1.0 that did not zero its structs passes
 * garbage there; rcdm_conv3x3 returns RCDM_EINVAL for c_in2 != 0 in every form, the phase form (upsample = 2) included. */

/* error codes */
#define RCDM_OK 0
#define RCDM_EINVAL (-1)   /* bad argument (null pointer, negative size, misaligned ld) */
#define RCDM_ESHAPE (-2)   /* shape not supported by this kernel */
#define RCDM_ELAUNCH (-3)  /* HIP launch / runtime error (see rcdm_last_hip_error) */
#define RCDM_EWORKSPACE (-4) /* workspace too small */
#define RCDM_ECOMM (-5)    /* RCCL missing or an RCCL call failed (see rcdm_comm_last_error) */

/* epilogue flags for rcdm_gemm / rcdm_conv3x3 (applied in fp32, one final rounding to f16) */
#define RCDM_EPI_BIAS 1      /* + bias[n]                              (fp32 [N])                  */
#define RCDM_EPI_ROWVEC 2    /* + rowvec[m / rows_per_sample][n]       (fp32, resnet.py:191-194)   */
#define RCDM_EPI_RESIDUAL 4  /* + residual[m][n]                       (f16, ldr)                  */
#define RCDM_EPI_GELU 16     /* out = gelu(acc + bias + rowvec) (+ residual): exact erf GELU, the "gelu" FeedForward of
                             * the stage-1 prior (diffusers GELU(approximate="none")); not with GEGLU  */
#define RCDM_EPI_GEGLU 8     /* out[m][j] = (h+bh) * gelu(g+bg); W/bias rows packed in groups of   */
                             /* 32 = 16 hidden rows then their 16 gate rows (rcdm_pack_geglu_rows) */
#define RCDM_EPI_QUICK_GELU 32 /* out = v * sigmoid(1.702 v), v = acc + bias + rowvec (+ residual): transformers "quick_gelu", the
                             * MLP activation of the SD-1.5 CLIP text encoder.  rcdm_gemm only (every tile family and the split-K
                             * reduce); not with GELU / GEGLU (RCDM_EINVAL); rcdm_gemm_ln / _lnx / *_gnstat / rcdm_conv3x3*:
                             * RCDM_ESHAPE */
#define RCDM_EPI_RELU 64     /* out = max(v, 0), v = acc + bias; a NaN stays NaN, -0.0 gives +0.0.  rcdm_conv2d only (where the
                             * only other bit allowed is RCDM_EPI_BIAS); every other entry point that takes an epilogue
                             * refuses it, and any bit this list does not name, with RCDM_ESHAPE */

int rcdm_version(void);
/* last HIP error code seen by this library on this thread (0 = none) and its string */
int rcdm_last_hip_error(void);
const char* rcdm_last_hip_error_string(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM  out[M][N] = epi( A[M][K] * W[N][K]^T )        replaces: nn.Linear / 1x1 InflatedConv3d calls
 *   attention.py:121,140-141,164 (to_q/k/v/out), :330,:352 (proj_in/out 1x1 conv),
 *   motion_module.py:166,170 (proj_in/out), resnet.py:208 (conv_shortcut),
 *   diffusers FeedForward GEGLU proj + out (attention.py:514, motion_module.py:243).
 *   A f16 row stride lda; W f16 [N][K] (nn.Linear's own [out,in] layout); K % 8 == 0, N % 8 == 0.
 *   split_k: 0 = library heuristic, 1 = off, >1 = forced; needs workspace (rcdm_gemm_workspace_bytes).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t M, N, K;
  int32_t lda, ldc, ldr;      /* row strides in elements (ldr only with RCDM_EPI_RESIDUAL) */
  int32_t epilogue;           /* RCDM_EPI_* bits */
  int32_t rows_per_sample;    /* RCDM_EPI_ROWVEC: rowvec row = m / rows_per_sample */
  int32_t ldt;                /* RCDM_EPI_ROWVEC: rowvec row stride (floats) */
  float out_scale;            /* out = epi(...) * out_scale   (1/output_scale_factor, resnet.py:210) */
  int32_t split_k;
  int32_t dup_rows;           /* != 0: every output row m is ALSO stored at row m + dup_rows of `out` (the two CFG halves
                               * of a step share everything before the first cross-attention: computed once, stored twice) */
} rcdm_gemm_desc;

size_t rcdm_gemm_workspace_bytes(const rcdm_gemm_desc* d);
/* rcdm_gemm with the LayerNorm that follows it fused into the epilogue: out = epi(A W^T) as rcdm_gemm (bias / residual /
 * out_scale / dup_rows), and ln->out[m][:] = LayerNorm(out[m][:]) * gamma + beta (+ pe[(m / rows_per_frame) % frames][:])
 * computed from the f16-rounded `out` row, exactly what rcdm_layernorm would read back.  For N <= 320 (one 160x320 tile
 * spans the row): the token-matrix GEMMs of the 64x64 level (to_out / proj_in -> norm1/2/3, attention.py:479-526,
 * motion_module.py:234-246), where the separate LayerNorm is a 26-MB read + 26-MB write per call.  No GEGLU / GELU /
 * row vector / split-K; no workspace. */
typedef struct {
  const float* gamma;
  const float* beta;
  const float* pe;            /* NULL, or the positional-encoding table [frames][N] (fp32) */
  void* out;                  /* f16 [M][ld] */
  int32_t ld;
  int32_t rows_per_frame, frames;
  float eps;
} rcdm_ln_fuse;
int rcdm_gemm_ln(const rcdm_gemm_desc* d, const rcdm_ln_fuse* ln, const void* A, const void* W, const float* bias,
                 const void* residual, void* out, void* stream);

/* Deferred LayerNorm: the nn.LayerNorm between two token GEMMs (attention.py:482,502,514: norm1/2/3 in front of to_q|k|v,
 * attn2.to_q and the GEGLU projection; motion_module.py:236,243: norms[i] + pos_encoder, ff_norm) without a launch of its
 * own and without the normalised tensor ever existing in HBM.  With W' = W diag(gamma) and b' = b + W beta (folded once, at
 * pack time; for pos_encoder a per-frame row table b'_f = b' + W pe_f passed as `rowvec`):
 *     LayerNorm(x) W^T + b  =  rstd (x W'^T) - (rstd mean) S + b',      S[n] = sum_c f16(W'[n][c]).
 *   PRODUCER (the GEMM that writes the rows x, e.g. to_out + residual or proj_in): stat_out[slot][m] (float2 each, slot-major:
 *     a consumer's lanes read consecutive rows of one slot) = (sum_t, M2_t) of the n_t f16 values it stores to row m in
 *     column tile t, one slot per column tile of its launch: the tile's sum and its CENTRED sum of squares, formed as
 *     shifted sums about the row's first stored value k of the tile (d = x - k is exact in fp32):
 *         sum_t = sum(d) + n_t k,    M2_t = max(0, sum(d^2) - sum(d)^2 / n_t).
 *     Slots stay independent, so two producers may fill one buffer.  stat_parts
 *     must equal rcdm_gemm_stat_parts(d) (the column-tile count of the tile shape a statistics-producing launch of this
 *     shape uses; RCDM_ESHAPE otherwise).  Plain / bias / row-vector / residual epilogues, no GEGLU, no split-K.
 *   CONSUMER (A = the RAW rows x, W = f16(W'), bias = b', colsum = S in the packed column order of W): stat_in / parts_in
 *     = the producer's partials of the A rows, C = the LayerNorm width, eps.  Its epilogue merges the slots about the first
 *     tile's mean K = sum_0 / n_0 (a_t = sum_t / n_t):
 *         U = sum_t n_t (a_t - K),   Q = sum_t [M2_t + n_t (a_t - K)^2],   mean = K + U / C,   var = (Q - U^2 / C) / C,
 *     so nothing of the size of mean^2 is ever formed: on rows with |mean| / sigma up to 256 rstd is within 1.5e-5 (relative,
 *     the finest threshold of the probe) and the mean within 3.2e-5 sigma of float64, a constant row gives var = 0 up to
 *     the rounding of its mean (measured on an MI355X, tests/test_hip_ln_cond.py; E[x^2] - mean^2, which this replaces,
 *     was off by up to 1.6e-2 there).  n_t is
 *     the producer's tile width (the last tile: what is left of C), which (C, parts_in) determines: parts_in = 1, or
 *     ceil(C / 64), ceil(C / 128), ceil(C / 256); any other count is RCDM_ESHAPE.  (rstd, mean rstd), bias and the row
 *     vector are applied to the fp32 accumulators, before GELU / GEGLU / residual and before the one rounding to f16.  Every epilogue form, no split-K; parts_in <= 20.
 *   One call may be both.  Both sides NULL = rcdm_gemm. */
typedef struct {
  float* stat_out;            /* producer: slot-major [stat_parts][stat_out_rows][2] fp32, or NULL */
  int32_t stat_parts;
  int32_t stat_out_rows;      /* rows per slot plane of stat_out: >= M + dup_rows */
  const float* stat_in;       /* consumer: [parts_in][stat_in_rows][2] fp32 (the producer's buffer), or NULL */
  int32_t parts_in;
  int32_t stat_in_rows;       /* rows per slot plane of stat_in (= the producer's stat_out_rows) */
  const float* colsum;        /* consumer: S [N] fp32 (16-byte aligned) */
  float eps;                  /* LayerNorm eps (1e-5) */
  int32_t C;                  /* LayerNorm width = K of the consumer */
} rcdm_lnx;
int rcdm_gemm_stat_parts(const rcdm_gemm_desc* d);   /* 0: a statistics-producing launch of this shape is not available */
/* The same for a call that is PRODUCER and, with consumer != 0, also CONSUMER: the consumer flag steers the tile choice too,
 * so a call that carries both sides must size stat_out from this query (consumer = 0 is rcdm_gemm_stat_parts). */
int rcdm_gemm_lnx_stat_parts(const rcdm_gemm_desc* d, int32_t consumer);
/* Two producers that fill ONE statistics buffer (the same projection on all rows and, later, on a row subset whose rows it
 * rewrites: the rank-1-context plan of the cross-attention) must use the same slot count.  rcdm_gemm_lnx therefore also
 * accepts a stat_parts other than rcdm_gemm_lnx_stat_parts(d, ..) where an LDS-DMA tile with exactly that column-tile
 * count exists (ceil(N / 64) or ceil(N / 128)) and takes that tile, unsplit; 1 / 0: */
int rcdm_gemm_lnx_parts_ok(const rcdm_gemm_desc* d, int32_t parts, int32_t consumer);
/* Workspace an rcdm_gemm_lnx call of this shape needs, with the SAME tile / split decision the call itself takes (statistics
 * producers and consumers are steered to other tile shapes than a plain rcdm_gemm of the shape: rcdm_gemm_workspace_bytes can
 * disagree).  Non-zero means the shape would run split-K, which rcdm_gemm_lnx refuses on either side (RCDM_ESHAPE). */
size_t rcdm_gemm_lnx_workspace_bytes(const rcdm_gemm_desc* d, int32_t producer, int32_t consumer);
int rcdm_gemm_lnx(const rcdm_gemm_desc* d, const rcdm_lnx* x, const void* A, const void* W, const float* bias,
                  const float* rowvec, const void* residual, void* out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* tuning/test knob for rcdm_gemm and rcdm_conv3x3: -1 = automatic (default: chosen per shape; env
 * RCDM_IGEMM=dma128|dma256|dma64 overrides), tile (pixels x channels): 1 = 128x128, 2 = 256x256, 3 = 64x64,
 * 4 = 64x64 with a four-slot LDS ring, 5 = 128x64.
 * Changes the workspace size a shape needs: query rcdm_*_workspace_bytes after setting it. */
/* per-shape overrides of the tile heuristics: "taps,M,N,Cin,variant,split;..." (taps 1 | 9, variant 1 .. 10, split 0 = that
 * variant's heuristic), looked at before the library's own measured table; "off" ignores the table, "" adds nothing, NULL goes
 * back to the environment variable RCDM_SHAPE_RULES (same syntax).  For tuning another chip / model without a rebuild
 * (tools/tune_rules.py).  Changes workspace sizes like rcdm_set_igemm_variant. */
int rcdm_set_shape_rules(const char* rules);
int rcdm_set_igemm_variant(int32_t variant);  /* 6 / 7 / 8: ping-pong kernel at 160x320 / 160x256 / 256x256; 9: igemm16 (160x160); 10: 128x64 with a three-slot LDS ring (GEMMs; a conv runs as 5) */
/* Tuning switch: 0 = the shape heuristic never picks the 8-wave ping-pong kernel (igemm8.hip), 1 = it may
 * (default; environment RCDM_PP=0 sets the initial state).  Used for same-process A/B timing. */
int rcdm_set_igemm_pingpong(int32_t on);
/* Tuning / test switch: 1 = split-K launches of the 160x160 and the LDS-DMA tile kernels leave f16 slabs (half the bytes to and
 * from the reduce pass; one extra f16 rounding per partial sum; not the GEGLU projections, not the ping-pong kernel), 0 = fp32
 * slabs, -1 = default (environment RCDM_SLAB16, else 1: measured -0.11 ms per step, whole-UNet error unchanged). */
int rcdm_set_splitk_slab_f16(int32_t on);
/* debug: when non-NULL, every igemm block writes 4 int64 {start, end (s_memtime ticks), ticks spent in epilogues,
 * k-steps done} at trace[(blockIdx.y*gridDim.x + blockIdx.x)*4]; NULL (default) disables it. */
/* The launch geometry the library chooses for a shape (what rcdm_gemm / rcdm_gemm_lnx / rcdm_conv3x3* will do; diagnostics:
 * tools/ceiling.py prices tile quantisation with it): out8 = {tile variant, BM, BN, row tiles, column tiles, split-K factor,
 * resident blocks per CU of that tile, k-steps of 64}.  No launch, no device access. */
int rcdm_gemm_plan_query(const rcdm_gemm_desc* d, int32_t producer, int32_t consumer, int32_t* out8);
int rcdm_debug_set_igemm_trace(void* device_buffer);
/* debug, builds with -DRCDM_ATTN_TRACE only (tools/trace_attn.py): when non-NULL every wave of rcdm_flash_attn writes 8 int64 at
 * trace[(block * waves + wave) * 8]: {loop ticks, ticks at the barrier + K/V staging, in the QK^T issue, in the softmax, in the PV
 * issue, key tiles, 0, 0}.  The product build ignores the pointer. */
int rcdm_debug_set_attn_trace(void* device_buffer);
/* roofline calibration: `blocks` x 4 waves each run iters x 4 independent v_mfma_f32_32x32x16_f16 (32768 flop each) and
 * nothing else; ticks[block] (optional) = s_memtime ticks the first wave spent in its loop.  tools/mfma_peak.py */
int rcdm_debug_mfma_peak(int32_t blocks, int32_t iters, float* sink, long long* ticks, void* stream);
int rcdm_gemm(const rcdm_gemm_desc* d, const void* A, const void* W, const float* bias,
              const float* rowvec, const void* residual, void* out, void* workspace,
              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * conv3x3 (pad 1) as implicit GEMM over channels-last rows.   replaces InflatedConv3d.forward
 *   resnet.py:10-18 with k=3: ResnetBlock3D conv1/conv2 (:188,:205), Downsample3D (:104, stride 2),
 *   Upsample3D (:65+:78: F.interpolate(nearest, x2) folded into the input indexing, never
 *   materialised), unet.py:403 conv_in, :457 conv_out.
 *   in : [n_img*h_in*w_in][lda] f16 (c_in channels used);  W f16 [c_out][9*c_in], k = tap*c_in + c,
 *   tap = ky*3+kx (i.e. torch weight.permute(0,2,3,1)); out rows = n_img*h_out*w_out where
 *   h_out = (h_in*(1+upsample) - 1)/stride + 1.  c_in % 8 == 0, c_out % 8 == 0.
 *   upsample = 2: the SAME operation as upsample = 1 (Upsample3D: nearest x2, then the 3x3 conv) computed as four 2x2
 *   "phase" convolutions over the SOURCE grid — output pixel (2y+a, 2x+b) of the upsampled image only ever sees the 2x2
 *   source pixels (y+a-1+r, x+b-1+c), each with the sum of the 3x3 taps that land on it — 4/9 of the multiply-adds.  W is
 *   then the phase image written by rcdm_pack_conv3x3_up2 (f16 [4][c_out][4*c_in]: the tap sums are formed in fp32 from the
 *   fp32 weights and rounded once), the epilogue may only carry RCDM_EPI_BIAS, stride 1, c_in % 64 == 0 (workspace:
 *   rcdm_conv3x3_workspace_bytes, as for the other forms).  Only shapes whose tiles fill the chip are taken: ask rcdm_conv3x3_up2_supported first (0: use
 *   upsample = 1 with the [c_out][9*c_in] weights; rcdm_conv3x3 itself returns RCDM_ESHAPE for such a descriptor).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_img, h_in, w_in, c_in, c_out;
  int32_t stride;     /* 1 | 2 */
  int32_t upsample;   /* 0 | 1 | 2 (2: phase form of 1, see above) */
  int32_t lda, ldc, ldr;
  int32_t epilogue;
  int32_t rows_per_sample, ldt;
  float out_scale;
  int32_t split_k;
  int32_t pad_after_only; /* 0: padding 1 on every side (default).  1: zero rows/columns only AFTER the image —
                           * diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)) then a stride-2 conv (VAE encoder).
                           * Needs stride 2, upsample 0 and EVEN h_in and w_in (h_out = h_in / 2: an odd side would give one
                           * row less than the symmetric form's formula above); RCDM_ESHAPE otherwise */
  int32_t dup_rows;       /* as rcdm_gemm_desc.dup_rows */
  int32_t c_in2, lda2;    /* rcdm_conv3x3_add1x1 only (0 otherwise): channels and row stride of the second input */
} rcdm_conv3x3_desc;

size_t rcdm_conv3x3_workspace_bytes(const rcdm_conv3x3_desc* d);
int rcdm_conv3x3_plan_query(const rcdm_conv3x3_desc* d, int32_t* out8);   /* as rcdm_gemm_plan_query */
int rcdm_conv3x3_up2_supported(const rcdm_conv3x3_desc* d);   /* 1 | 0, d->upsample == 2 */
int rcdm_conv3x3(const rcdm_conv3x3_desc* d, const void* in, const void* W, const float* bias,
                 const float* rowvec, const void* residual, void* out, void* workspace,
                 size_t workspace_bytes, void* stream);
/* conv3x3(in) + conv1x1(in2) accumulated in ONE implicit GEMM over K = 9 c_in + c_in2.   replaces the tail of
 *   ResnetBlock3D.forward for c_in != c_out, resnet.py:205-212: conv2(hidden_states) + conv_shortcut(input_tensor)
 *   (the sum is formed in the fp32 accumulators; the stand-alone shortcut launch, its f16 output and the residual read
 *   of it are gone).  in2: [rows of `out`][lda2] f16, c_in2 channels used — row m of in2 is output pixel m, so stride 1,
 *   upsample 0, no pad_after_only.  W f16 [c_out][9*c_in + c_in2]: the rcdm_conv3x3 layout followed by the 1x1 weight's
 *   [c_out][c_in2] columns; bias = the sum of the two biases.  c_in % 64 == 0 and c_in2 % 64 == 0 (whole k-steps).
 *   Everything else (epilogue flags, residual, split_k, workspace query with the same descriptor) as rcdm_conv3x3;
 *   rcdm_conv3x3 / rcdm_conv3x3_gnstat themselves return RCDM_EINVAL for a descriptor with c_in2 != 0. */
int rcdm_conv3x3_add1x1(const rcdm_conv3x3_desc* d, const void* in, const void* in2, const void* W, const float* bias,
                        const float* rowvec, const void* residual, void* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+SiLU).  replaces torch.nn.GroupNorm applied to the 5-D tensor — statistics over
 *   (C/groups, f, H, W) ACROSS frames — at resnet.py:185-186,196,202 and unet.py:455-456
 *   (samples = b, rows_per_sample = f*H*W), and the per-frame 4-D form at attention.py:328 and
 *   motion_module.py:162 (samples = b*f, rows_per_sample = H*W, eps 1e-6, no SiLU).
 *   Three launches: stats (deterministic fixed-order partials, no float atomics), finalize, apply; ONE launch when a
 *   sample has <= 512 rows (the 8x8 / per-frame 16x16 levels): a block owns a whole (sample, group bundle) slab.
 *   C % (2*groups) == 0, C % 8 == 0.  stats workspace: rcdm_groupnorm_workspace_bytes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t samples, rows_per_sample, C, groups;
  int32_t ldx, ldy;
  float eps;
  int32_t silu;  /* 0 | 1 */
} rcdm_groupnorm_desc;

size_t rcdm_groupnorm_workspace_bytes(const rcdm_groupnorm_desc* d);
int rcdm_groupnorm_silu(const rcdm_groupnorm_desc* d, const void* x, const float* gamma,
                        const float* beta, void* y, void* workspace, size_t workspace_bytes,
                        void* stream);
/* A split-K GEMM / conv whose reduce pass ALSO leaves the partial statistics of the GroupNorm that reads its output next —
 * resnet.py:185-202 (conv1 -> norm2), attention.py:328 / motion_module.py:162 (the norm in front of a transformer / motion
 * module, fed by conv2 or by the feed-forward GEMM) — so that the norm needs no statistics launch and no extra read of the
 * tensor:  rcdm_gemm_gnstat / rcdm_conv3x3_gnstat(d, gn, ..., gn_workspace)  then  rcdm_groupnorm_silu_prestat(gn, out, ...,
 * gn_workspace).  `gn` describes the norm over exactly the rows the launch writes (samples * rows_per_sample == M, C == N,
 * ldx == ldc).  The statistics are taken from the STORED halfs in the order of the stand-alone pass: results are bit-identical
 * to rcdm_gemm / rcdm_conv3x3 followed by rcdm_groupnorm_silu.  *_gnstat_ok: 1 when the pair qualifies (the launch is split-K
 * — only then does a reduce pass exist —, no GEGLU / dup_rows / upsample == 2, the norm takes its three-launch form); the
 * calls return RCDM_ESHAPE otherwise.  gn_workspace: rcdm_groupnorm_workspace_bytes(gn), the same bytes passed on. */
int rcdm_gemm_gnstat_ok(const rcdm_gemm_desc* d, const rcdm_groupnorm_desc* gn);
int rcdm_gemm_gnstat(const rcdm_gemm_desc* d, const rcdm_groupnorm_desc* gn, const void* A, const void* W, const float* bias,
                     const float* rowvec, const void* residual, void* out, void* workspace, size_t workspace_bytes,
                     void* gn_workspace, size_t gn_workspace_bytes, void* stream);
int rcdm_conv3x3_gnstat_ok(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn);
int rcdm_conv3x3_gnstat(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const void* in, const void* W,
                        const float* bias, const float* rowvec, const void* residual, void* out, void* workspace,
                        size_t workspace_bytes, void* gn_workspace, size_t gn_workspace_bytes, void* stream);
int rcdm_conv3x3_add1x1_gnstat(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const void* in, const void* in2,
                               const void* W, const float* bias, const float* rowvec, const void* residual, void* out,
                               void* workspace, size_t workspace_bytes, void* gn_workspace, size_t gn_workspace_bytes,
                               void* stream);   /* rcdm_conv3x3_add1x1 with the statistics-carrying reduce (rcdm_conv3x3_gnstat_ok) */
/* finalize + apply only: the partial statistics are already in `workspace` (left there by a *_gnstat call with this
 * descriptor).  rcdm_groupnorm_prestat_ok: 1 when this descriptor's norm has a statistics pass to replace (three-launch
 * form; the smallest tensors run as one launch). */
int rcdm_groupnorm_prestat_ok(const rcdm_groupnorm_desc* d);
int rcdm_groupnorm_silu_prestat(const rcdm_groupnorm_desc* d, const void* x, const float* gamma, const float* beta, void* y,
                                void* workspace, size_t workspace_bytes, void* stream);
/* tuning / test switch: 1 = norms with >= 4 samples and <= 128 partial blocks per sample (the per-frame norms of the
 * transformers / motion modules) run as TWO launches — statistics, then an apply kernel whose blocks finalise their sample's
 * groups themselves (bit-identical to the three-launch form) — 0 = always statistics / finalize / apply, -1 = default
 * (0: the two-launch form measured 0.05 ms per step slower; environment RCDM_GN_FOLD=1 sets 1). */
int rcdm_set_groupnorm_fold(int32_t on);
/* statistics only: stat[sample][group][2] = (mean, 1 / sqrt(var + eps)), fp32 — the first two launches of the three-launch
 * form, for a consumer that applies the normalisation itself (rcdm_rowchain's gn_stat: the norm in front of proj_in,
 * attention.py:328-330, motion_module.py:162-166).  ldy / silu of the descriptor are ignored; workspace as above. */
int rcdm_groupnorm_stats(const rcdm_groupnorm_desc* d, const void* x, float* stat, void* workspace,
                         size_t workspace_bytes, void* stream);
/* the same when the partial statistics are already in `workspace` (left there by a *_gnstat call with this descriptor, as for
 * rcdm_groupnorm_silu_prestat): the finalize launch only.  RCDM_ESHAPE when the descriptor's norm has no three-launch form. */
int rcdm_groupnorm_stats_prestat(const rcdm_groupnorm_desc* d, float* stat, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* finalize only, on partials a producer wrote in its OWN geometry: partial[samples][groups][splits][3] = (count, mean, M2)
 * fp32 -> stat[samples][groups][2] = (mean, 1 / sqrt(var + eps)); the fixed-order combination of the three-launch form.
 * Used behind rcdm_conv3x3_wino(gn_out, ...), whose output transform leaves one partial per (sample, group, 2x2 tile). */
int rcdm_groupnorm_finalize(int32_t samples, int32_t groups, int32_t splits, float eps, const float* partial, float* stat,
                            void* stream);
/* the apply launch alone: y = (x - mean) rstd gamma + beta (+ SiLU) with (mean, rstd) = stat[sample][group] already final
 * (rcdm_groupnorm_finalize / rcdm_groupnorm_stats) — the third launch of the three-launch form. */
int rcdm_groupnorm_apply(const rcdm_groupnorm_desc* d, const void* x, const float* stat, const float* gamma, const float* beta,
                         void* y, void* stream);

/* conv3x3, stride 1, padding 1, as Winograd F(2x2, 3x3) (wino.hip; round 6): the same operation as rcdm_conv3x3 /
 *   rcdm_conv3x3_add1x1 — ResnetBlock3D's conv1 / conv2 (+ conv_shortcut), resnet.py:188,205-212 — with 4/9 of the
 *   multiply-adds, for the levels where the implicit GEMM is a chain of latencies (the 16x16 / 8x8 latents: few rows, wide
 *   channels).  Three launches: input transform B^T d B (fp32 arithmetic on the f16 pixels, one rounding), 16 (+ 4) batched
 *   160x160-tile GEMMs with fp32 results in the workspace, output transform A^T M A + epilogue in fp32 (one rounding).
 *   `d` is the rcdm_conv3x3_desc of the equivalent call: stride 1, upsample 0, no pad_after_only / dup_rows, h_in and w_in
 *   even, c_in % 64 == 0 (c_in2 % 64 == 0), epilogue bits BIAS | ROWVEC | RESIDUAL; split_k 0 = heuristic (one resident
 *   round of the chip).  U = rcdm_pack_conv3x3_wino(w): f16 [16][c_out][c_in], position p = 4 i + j holds (G g G^T)[i][j]
 *   formed in fp32 from the fp32 weights and rounded once.  in2 / W2 (both or neither; d->c_in2, d->lda2): the second input
 *   of rcdm_conv3x3_add1x1 and its PLAIN f16 [c_out][c_in2] 1x1 weight (rcdm_pack_f16) — it needs no transform, its four
 *   output-parity GEMMs ride as four more batch entries; bias = the sum of the two biases.
 *   gn != NULL: `in` is the RAW input of a GroupNorm (+ SiLU when gn->silu) whose (mean, rstd) pairs are in gn_stat
 *   ([samples][groups][2] fp32, rcdm_groupnorm_stats) and the input transform applies x * rstd * gamma + (beta - mean * rstd *
 *   gamma) (+ SiLU) on the way — resnet.py:185-186 / :202 in front of conv1 / conv2 — before the zero padding; gn->C == c_in,
 *   gn->samples * gn->rows_per_sample == n_img * h_in * w_in; ldx / ldy / eps of gn are not used here.
 *   Numerics: the MFMA operands are f16(B^T d B) (|.| <= 4 max|d|) and f16(G g G^T): about twice the operand-rounding
 *   noise of rcdm_conv3x3 (which multiplies the f16 pixels and f16 weights themselves); accumulation, both transforms and the
 *   epilogue are fp32.  Results are NOT bit-identical to rcdm_conv3x3.  rcdm_conv3x3_wino_supported: 1 | 0.
 *   gn_out != NULL: the GroupNorm that reads `out` NEXT (over exactly the rows written: gn_out->C == c_out, samples *
 *   rows_per_sample == n_img * h_in * w_in); the output transform then also leaves its partial statistics, taken from the stored
 *   halfs, in gn_out_partial — fp32 [samples][groups][rows_per_sample / 4][3] = (count, mean, M2), one per 2x2 tile — for
 *   rcdm_groupnorm_finalize(samples, groups, rows_per_sample / 4, eps, ...): that norm needs no statistics pass (c_out <= 8192). */
int rcdm_conv3x3_wino_supported(const rcdm_conv3x3_desc* d);
size_t rcdm_conv3x3_wino_workspace_bytes(const rcdm_conv3x3_desc* d);
int rcdm_conv3x3_wino_plan_query(const rcdm_conv3x3_desc* d, int32_t* out8);   /* as rcdm_gemm_plan_query; variant 11, column tiles x entries */
int rcdm_pack_conv3x3_wino(const float* w, int32_t c_out, int32_t c_in, void* dst, void* stream);
/* Upsample3D.forward (resnet.py:60-79: F.interpolate(nearest, x2) + conv3x3) as ONE rcdm_gemm + this gather (round 6): on the
 * upsampled grid output pixel (Y, X) = sum over the nine taps of w[ky][kx] . s((Y + ky - 1) >> 1, (X + kx - 1) >> 1), so every
 * product is a tap's 1x1 image of a SOURCE pixel — nine products per source pixel and channel pair (the four-phase form of
 * rcdm_conv3x3 upsample = 2 needs sixteen).  P = rcdm_gemm(source rows [n_img*h*w][c_in], W9) with W9 = f16 [9*c_out][c_in],
 * row tap*c_out + c = weight[c][:][ky][kx] (tap = 3 ky + kx; the ordinary rounded weights, no sums), no bias: f16
 * [n_img*h*w][ldp >= 9 c_out].  The gather adds, per output pixel of the (2h x 2w) image, the nine planes' values of the source
 * pixels its taps land on (taps outside the upsampled image skipped = its zero padding) + bias[c_out] (may be NULL), fp32 sum,
 * one rounding: out f16 [n_img*4*h*w][ldc].  Numerics: the nine products are rounded to f16 before the sum (one more rounding
 * per term than the implicit GEMM's fp32 accumulation). */
int rcdm_upsample_taps_gather(const void* P, int32_t ldp, int32_t n_img, int32_t h, int32_t w, int32_t c_out, const float* bias,
                              void* out, int32_t ldc, void* stream);
/* the same gather with upsample = 0: a plain stride-1, padding-1 conv3x3 as rcdm_gemm (N = 9 c_out tap planes over its own
 * pixels) + gather — no multiply saved, but a conv with very few output channels (unet.py:457 conv_out: 320 -> 4) becomes a
 * plain GEMM whose N is 9x wider than the conv's, instead of an implicit GEMM that pads 4 channels to a 64-wide tile.
 * upsample = 1 is rcdm_upsample_taps_gather. */
int rcdm_conv_taps_gather(const void* P, int32_t ldp, int32_t n_img, int32_t h, int32_t w, int32_t c_out, int32_t upsample,
                          const float* bias, void* out, int32_t ldc, void* stream);
/* tuning / test switch: 1 = the batched GEMM of rcdm_conv3x3_wino leaves f16 slabs (half the bytes between it and the output
 * transform, whole-row stores; every transform-domain sum is rounded to f16 before A^T M A), 0 = fp32 slabs, -1 = default
 * (environment RCDM_WINO_SLAB16, else 1). */
int rcdm_set_wino_slab_f16(int32_t on);
int rcdm_conv3x3_wino(const rcdm_conv3x3_desc* d, const rcdm_groupnorm_desc* gn, const float* gn_stat,
                      const float* gn_gamma, const float* gn_beta, const void* in, const void* in2, const void* U,
                      const void* W2, const float* bias, const float* rowvec, const void* residual, void* out,
                      void* workspace, size_t workspace_bytes, const rcdm_groupnorm_desc* gn_out, float* gn_out_partial,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (eps 1e-5, torch default) with optional fused positional-encoding add
 *   replaces nn.LayerNorm at attention.py:482,502,514 and motion_module.py:236,243; with pe != NULL
 *   also PositionalEncoding.forward motion_module.py:265-267 applied after the "(b f) d c -> (b d) f c"
 *   regroup (:299-302): y[m] += pe[(m / rows_per_frame) % frames].   C % 8 == 0, C <= 2048.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t M, C, ldx, ldy;
  float eps;
  int32_t rows_per_frame, frames; /* only with pe */
} rcdm_layernorm_desc;

int rcdm_layernorm(const rcdm_layernorm_desc* d, const void* x, const float* gamma,
                   const float* beta, const float* pe, void* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flash-style multi-head attention, softmax(scale * Q K^T) V, no mask, online softmax in fp32.
 *   replaces CrossAttention._attention attention.py:170-199 (+ reshape_heads_to_batch_dim :93-105):
 *   self-attention over the hw latent patches of one frame and cross-attention over the L_text
 *   context rows of that frame.  Q rows [batch*Lq][ldq] with head h at columns [h*d, (h+1)*d);
 *   K,V rows [batch*Lk][ldk|ldv]; out [batch*Lq][ldo].  Head dim: d % 8 == 0 for d <= 160; d % 64 == 0 for
 *   160 < d <= 512 (rcdm_flash_attn, and rcdm_flash_attn_masked with key_valid == NULL and causal == 0, only: a mask at
 *   d > 160 is RCDM_ESHAPE, as is d > 512).  The wide heads are the one 512-channel head of the SD-1.5 VAE mid block
 *   (diffusers 0.24.0 AutoencoderKL, UNetMidBlock2D attention over the h*w latent pixels of an image) at any image size:
 *   a kernel of its own (csrc/attn_wide.hip: 4 waves x 32 queries per block, one wave per SIMD), same layout rules
 *   (ldq / ldk / ldv % 8 == 0, ldo % 4 == 0, column views of wider buffers allowed), no workspace, capturable.  Its
 *   softmax reference is fixed per pass over the keys (first-tile row max; a second pass on the exact row max when a
 *   query's scores leave the f16 range of exp2 around it), so it has no score-range limit and ignores `flags`.
 *   Range: scaled scores |scale * log2(e) * q.k| < 2^15 (the d = 40, Lk >= 256 kernel keeps its running max as an f16 inside
 *   the Q fragment and re-rounds Q * scale * log2(e) to f16: relative error ln2 * 2^-12 * |scaled score| on a probability).
 *   A caller that cannot bound its scores below that sets RCDM_ATTN_WIDE_RANGE in `flags` (or the environment sets
 *   RCDM_ATTN_MSUB=0): the fp32-fma softmax kernel, which has neither limit.  rcdms_amd/engine.py sets it from a
 *   data-independent bound on |q| |k| (LayerNorm output norm x Frobenius norms of the folded per-head weights).
 *   Rounding (rcdm_flash_attn, rcdm_flash_attn_masked and rcdm_xattn, every head dim): the probabilities are rounded toward
 *   zero to f16 and normalised by the sum of the ROUNDED values, so a constant V column is reproduced exactly.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_ATTN_WIDE_RANGE 1
typedef struct {
  int32_t batch, heads, Lq, Lk, d;
  int32_t ldq, ldk, ldv, ldo;
  float scale;
  int32_t flags;              /* 0, or RCDM_ATTN_WIDE_RANGE */
} rcdm_attn_desc;

int rcdm_flash_attn(const rcdm_attn_desc* d, const void* Q, const void* K, const void* V, void* out,
                    void* stream);
/* the same with a mask: key k of batch b is visible to query q iff key_valid[b*Lk + k] != 0 (key_valid may be NULL =
 * all valid) and, with causal != 0, k <= q.  Replaces the additive attention_mask of the stage-1 prior transformer
 * (myprior_transformer.py:389-393: (1 - text_mask) * -10000 padded, + causal_attention_mask :250-256), whose masked
 * probabilities are exactly 0 in fp32.  A query with no visible key yields a zero row. */
int rcdm_flash_attn_masked(const rcdm_attn_desc* d, const void* Q, const void* K, const void* V,
                           const unsigned char* key_valid, int32_t causal, void* out, void* stream);

/* Cross-attention with a short key sequence (Lk <= 96): CrossAttention.forward with encoder_hidden_states,
 * attention.py:139-168, at the 85 / 91 context rows of the stage-2 UNet.  A wave holds all scores of 32 queries of one
 * head in registers (no key loop, no online rescale); a block of 8 waves shares one head's operands through LDS.  K and V are passed as the per-context FRAGMENT-MAJOR image rcdm_xattn_pack_kv
 * writes once per context (they do not change over the denoising steps): every MFMA operand fragment is one contiguous
 * 1-KiB block in lane order; rcdm_xattn_image_bytes sizes it.  `d` is the rcdm_attn_desc of the equivalent
 * rcdm_flash_attn call (ldk / ldv unused by rcdm_xattn); results agree with rcdm_flash_attn to f16 rounding. */
size_t rcdm_xattn_image_bytes(int32_t batch, int32_t heads, int32_t d);
int rcdm_xattn_pack_kv(const void* K, const void* V, int32_t batch, int32_t Lk, int32_t heads, int32_t d, int32_t ldk,
                       int32_t ldv, void* image, void* stream);
int rcdm_xattn(const rcdm_attn_desc* d, const void* Q, const void* image, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Temporal self-attention over the f frames of every (sample, pixel, head).
 *   replaces VersatileAttention.forward motion_module.py:294-354 between to_q/k/v and to_out: the
 *   "(b f) d c -> (b d) f c" regroup, 5x5 softmax(QK^T*scale)V and the inverse regroup become index
 *   arithmetic.  qkv rows ordered (b, f, pixel), [q | k | v] at columns [0,C) [C,2C) [2C,3C).
 *   frames <= 8, d % 8 == 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t samples, frames, pixels, heads, d;
  int32_t ldqkv, ldo;
  float scale;
} rcdm_temporal_attn_desc;

int rcdm_temporal_attn(const rcdm_temporal_attn_desc* d, const void* qkv, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused feed-forward, row-stationary (rowff.hip):  out[m][:] = x[m][:] + FF_geglu(LayerNorm(x[m][:]))  in one launch.
 *   replaces the chain nn.LayerNorm -> diffusers FeedForward(dim, activation_fn="geglu") -> + hidden_states at
 *   attention.py:514 (norm3 / ff of BasicTransformerBlock.forward) and motion_module.py:243 (ff_norm / ff of
 *   TemporalTransformerBlock.forward): Linear(C -> 8C) -> split (hidden, gate) -> hidden * gelu(gate) (exact erf
 *   GELU) -> Linear(4C -> C) -> + bias -> + x.  The 4C-wide hidden tensor is never written: a wave keeps its 16 token
 *   rows and their fp32 output accumulator in registers and streams the weights through LDS.
 *   Weights come as the fragment-major stream rcdm_pack_ff_stream writes once (12 C^2 halfs, rcdm_ff_stream_bytes):
 *   w1 = ff.net.0.proj.weight fp32 [8C][C], b1 = ff.net.0.proj.bias [8C], w2 = ff.net.2.weight fp32 [C][4C];
 *   b1_packed [8C] floats.  b2 = ff.net.2.bias [C].  out may alias x.  Supported C: rcdm_ff_fused_supported.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t M, C;
  int32_t ldx, ldo;   /* row strides in elements, multiples of 8 */
  float eps;          /* LayerNorm eps (1e-5) */
} rcdm_ff_desc;
size_t rcdm_ff_stream_bytes(int32_t C);
int rcdm_ff_fused_supported(int32_t C);
int rcdm_pack_ff_stream(const float* w1, const float* b1, const float* w2, int32_t C, void* wstream, float* b1_packed,
                        void* stream);
int rcdm_ff_fused(const rcdm_ff_desc* d, const void* x, const float* ln_gamma, const float* ln_beta, const void* wstream,
                  const float* b1_packed, const float* b2, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-stationary chain (rowff.hip), one launch:
 *     tok[m][:] = a_in[m][:] W_a^T + a_bias (+ res[m][:])                  -> stored (f16 [M][ldt])
 *     y[m][:]   = LayerNorm(tok[m][:]) * gamma + beta (+ pe[(m / rows_per_frame) % frames][:])
 *     tail 1 / 3:  out[m][0 : tail*C] = y[m][:] W_t^T          (no bias; W_t = fp32 [tail*C][C], e.g. [to_q; to_k; to_v])
 *     tail 0:      out[m][:] = tok[m][:] + FF_geglu(y[m][:])   (as rcdm_ff_fused; may be written in place of tok)
 *     tail 2:      out[m][:] = z_res[m][:] + ((tok[m][:] + FF_geglu(y[m][:])) W_z^T + z_bias)   — the block's proj_out and the
 *                  residual add of Transformer3DModel / TemporalTransformer3DModel.forward (attention.py:352-363,
 *                  motion_module.py:170-176) ride too; the feed-forward's output rows are NOT stored (tok keeps the rows
 *                  stage A wrote).  Needs res, no pe.  W_z = fp32 [C][C], passed to rcdm_pack_rowchain as wt.
 *     tail 4:      out[m][0 : C] = temporal self-attention of q | k | v = y[m][:] W_t^T (W_t as for tail 3; q, k, v rounded to
 *                  f16 as tail 3 stores them, never stored): for the pixel of row m, softmax over its `frames` rows of
 *                  q k^T / sqrt(C / 8) per head (8 heads), times v — what rcdm_temporal_attn computes from tail 3's output
 *                  (motion_module.py:299-302).  Rows are [sample][frame][pixel]: frames = 5, rows_per_frame % 16 == 0 and
 *                  M % (5 * rows_per_frame) == 0 (RCDM_ESHAPE otherwise), both given with or without pe.  A block takes
 *                  2 x 16 pixels x 5 frames; with gn_stat, gn_rows == rows_per_frame (one GroupNorm sample per image, any
 *                  multiple of 16).  out may alias a_in.  The stream is packed for this tail (rcdm_pack_rowchain tail 4).
 *   replaces, in BasicTransformerBlock.forward / Transformer3DModel.forward (attention.py:330,479-514) and
 *   TemporalTransformer3DModel / TemporalTransformerBlock.forward (motion_module.py:166,234-243,299-302):
 *     proj_in -> norm1 -> [to_q | to_k | to_v]                         (res = NULL, tail 3)
 *     attn1.to_out[0] + hidden_states -> norm2 -> attn2.to_q           (res = tok, tail 1)
 *     attention_blocks[i].to_out[0] + hidden_states -> norms[i + 1] + pos_encoder -> [to_q | to_k | to_v]   (tail 3, pe)
 *     attn2.to_out[0] / attention_blocks[-1].to_out[0] + hidden_states -> norm3 / ff_norm -> ff -> + hidden_states  (tail 0)
 *   W_a = fp32 [C][C] (nn.Linear layout).  The weights come as one fragment-major stream (rcdm_pack_rowchain,
 *   rcdm_rowchain_stream_bytes); b1_packed / b2 only with tail 0.  tok may alias res, out may alias tok (tail 0) — a block
 *   reads and writes only its own rows.  Supported C: rcdm_rowchain_supported; supported (C, tail, pe) combinations:
 *   rcdm_rowchain_config_supported — pe (with rows_per_frame, frames <= 8) rides with tail 1 / 3 only: with the feed-forward
 *   tails the per-block parameter region (up to 19 C floats) would not fit the 160 KB of LDS (RCDM_ESHAPE).
 *   Preconditions (RCDM_EINVAL / RCDM_ESHAPE when violated): every pointer 16-byte aligned (the fp32 vectors a_bias, ln_*,
 *   pe, b1_packed, b2, z_bias, gn_* are fetched as float4, the rows as 16-byte pieces), and M * ld * 2 < 2^31 for every row
 *   operand (32-bit byte offsets into 2-GB buffer resources).  The same two rules hold for rcdm_ff_fused.
 *   gn_stat != NULL (only with res == NULL): a_in is the RAW input of the GroupNorm in front of proj_in and the kernel
 *   applies  a_in[m][c] * rstd * gn_gamma[c] + (gn_beta[c] - mean * rstd * gn_gamma[c])  (rounded to f16 like the separate
 *   launch) with (mean, rstd) = gn_stat[m / gn_rows][c / (C / gn_groups)] from rcdm_groupnorm_stats; gn_rows % 16 == 0,
 *   gn_rows >= 160.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t M, C;
  int32_t lda, ldr, ldt, ldo;      /* row strides in elements, multiples of 8 (ldr only with res) */
  int32_t tail;                    /* 0 = feed-forward, 1 = GEMM to C columns, 2 = feed-forward + projection, 3 = GEMM to 3C,
                                      4 = GEMM to 3C + temporal attention */
  int32_t rows_per_frame, frames;  /* only with pe or tail 4 */
  float eps;                       /* LayerNorm eps (1e-5) */
  int32_t gn_groups, gn_rows;      /* only with gn_stat: groups and rows per sample of the GroupNorm */
  int32_t ldz;                     /* row stride of z_res (tail 2) */
} rcdm_rowchain_desc;
int rcdm_rowchain_supported(int32_t C);
int rcdm_rowchain_config_supported(int32_t C, int32_t tail, int32_t pe_frames);   /* pe_frames = 0: no pe */
size_t rcdm_rowchain_stream_bytes(int32_t C, int32_t tail);
/* wa [C][C]; tail 1 / 3: wt [tail*C][C]; tail 4: wt [3C][C]; tail 0 / 2: w1 [8C][C], b1 [8C], w2 [C][4C] and b1_packed [8C] (out); tail 2: wt [C][C] */
int rcdm_pack_rowchain(const float* wa, int32_t C, int32_t tail, const float* wt, const float* w1, const float* b1,
                       const float* w2, void* wstream, float* b1_packed, void* stream);
int rcdm_rowchain(const rcdm_rowchain_desc* d, const void* a_in, const void* res, void* tok, const float* a_bias,
                  const float* ln_gamma, const float* ln_beta, const float* pe, const void* wstream, const float* b1_packed,
                  const float* b2, void* out, const float* gn_stat, const float* gn_gamma, const float* gn_beta,
                  const void* z_res, const float* z_bias, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row softmax: y[m][n] = softmax over n of (scale * x[m][n]); f16 rows, fp32 math, N % 8 == 0, N <= 4096, scale > 0.
 *   With two rcdm_gemm calls (scores = Q K^T, out = P V^T^T) it is the score-buffer form of the single 512-channel
 *   head of the SD-1.5 VAE mid block (diffusers 0.24.0 AutoencoderKL, called at RCDMs_pipeline.py:281,429 — SURVEY §8f
 *   N3) up to 4096 latent pixels; above, rcdm_flash_attn at d = 512 (rcdms_amd/vae.py, mid_attention_form).
 * ---------------------------------------------------------------------------------------------- */
int rcdm_softmax_rows(int32_t M, int32_t N, int32_t ldx, int32_t ldy, float scale, const void* x, void* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Timestep embedding: diffusers 0.24.0 Timesteps(dim, flip_sin_to_cos=True, freq_shift=0) as used
 *   at unet.py:100,383: out[r][0:half] = cos(t_r*w_i), out[r][half:] = sin(t_r*w_i),
 *   w_i = exp(-ln(10000)*i/half).  t fp32 device array [rows]; out fp32 [rows][dim].
 * ---------------------------------------------------------------------------------------------- */
int rcdm_timestep_embed(const float* t, int32_t rows, int32_t dim, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tiny-M fp32 linear: out[r][n] = act_out( sum_k act_in(x[r][k]) * W[n][k] + bias[n] ), rows <= 8.
 *   replaces TimestepEmbedding (linear_1 -> SiLU -> linear_2, unet.py:103,389) and every
 *   ResnetBlock3D.time_emb_proj(silu(temb)) (resnet.py:191), all 22 batched as one N = sum(Cout).
 *   W f16 [N][K]; silu_in / silu_out are 0|1.  K % 8 == 0.
 * ---------------------------------------------------------------------------------------------- */
int rcdm_small_linear(const float* x, int32_t rows, int32_t K, const void* W, const float* bias,
                      int32_t N, int32_t silu_in, int32_t silu_out, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Assemble the UNet input rows from the sampling-loop state: replaces
 *   torch.cat([latents]*2) + cat([x, mask, masked_latents], dim=1) RCDMs_pipeline.py:482-486 and the
 *   NCFHW->channels-last f16 conversion.  latents fp32 (S,4,f,H,W); mask fp32 (reps*S,1,f,H,W);
 *   masked fp32 (reps*S,4,f,H,W); reps = 2 with CFG (uncond copies first), 1 without.
 *   out rows [(reps*S)*f*H*W][ld] f16, channels 0..8 written, 9..c_pad-1 zeroed.
 * ---------------------------------------------------------------------------------------------- */
int rcdm_assemble_input(const float* latents, const float* mask, const float* masked, int32_t S,
                        int32_t reps, int32_t frames, int32_t H, int32_t W, void* out, int32_t ld,
                        int32_t c_pad, void* stream);

/* generic layout converters for UNet3DConditionModel.forward called directly with a 5-D tensor
 * (unet.py:322-330): fp32 (b,C,f,H,W) -> f16 rows [b*f*H*W][ld] (channels >= C zeroed up to c_pad)
 * and f16 rows -> fp32 (b,C,f,H,W). */
int rcdm_ncfhw_to_rows(const float* x, int32_t b, int32_t C, int32_t frames, int32_t H, int32_t W,
                       void* out, int32_t ld, int32_t c_pad, void* stream);
int rcdm_rows_to_ncfhw(const void* rows, int32_t ld, int32_t b, int32_t C, int32_t frames, int32_t H,
                       int32_t W, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused classifier-free guidance + DDIM step (eta = 0, epsilon prediction), in place on `latents`:
 *   replaces noise_pred.chunk(2); eps = eps_u + s*(eps_c - eps_u) RCDMs_pipeline.py:492-494 and
 *   diffusers 0.24.0 DDIMScheduler.step (:497):  x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);
 *   x' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps.
 *   eps rows f16 [(reps*S)*f*H*W][ld] (uncond sample block first); latents fp32 (S,4,f,H,W).
 *   coef: device fp32 table [n_steps][4] = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)};
 *   step_counter: device int32; the kernel uses row coef[*step_counter] (the counter is advanced by
 *   rcdm_advance_step so a captured graph replays with no host-side parameter change).
 * ---------------------------------------------------------------------------------------------- */
int rcdm_cfg_ddim_step(const void* eps, int32_t ld, float* latents, int32_t S, int32_t reps,
                       int32_t frames, int32_t H, int32_t W, float guidance_scale, const float* coef,
                       const int32_t* step_counter, void* stream);
/* Fused classifier-free guidance + one PLMS step of diffusers 0.24.0 PNDMScheduler(skip_prk_steps=True) — the other scheduler
 *   type RCDMsPipeline's constructor accepts (RCDMs_pipeline.py:72-79), stepped at :497 — in place on `latents`:
 *   e = eps_u + s (eps_c - eps_u); e' = the linear-multistep combination of e with up to three stored predictions;
 *   x' = sqrt(a'/a) x - (a' - a) e' / (a sqrt(1 - a') + sqrt(a (1 - a) a')).
 *   table: device fp32 [n_calls][12], one row per model evaluation (n_calls = num_inference_steps + 1: the second
 *   timestep is evaluated twice), as rcdms_amd.scheduler.PNDMScheduler.plms_table() lays it out:
 *   (a, b, w_now, w1, w2, w3, slot_now, s1, s2, s3, mode, 0); history: device fp32 [5][S*4*f*H*W], caller-owned, carries
 *   the stored predictions (slots 0..3) and the first sample (slot 4) between calls; no initialisation needed.
 *   step_counter as in rcdm_cfg_ddim_step. */
int rcdm_cfg_pndm_step(const void* eps, int32_t ld, float* latents, float* history, int32_t S, int32_t reps,
                       int32_t frames, int32_t H, int32_t W, float guidance_scale, const float* table,
                       const int32_t* step_counter, void* stream);
/* Fused classifier-free guidance + one step of diffusers 0.24.0 EulerDiscreteScheduler (s_churn = 0),
 *   EulerAncestralDiscreteScheduler, LMSDiscreteScheduler (order 4) or DPMSolverMultistepScheduler (dpmsolver / dpmsolver++,
 *   midpoint / heun, orders 1-3) — the remaining scheduler types RCDMsPipeline's constructor accepts (RCDMs_pipeline.py:72-79),
 *   stepped at :497 with scale_model_input (:484) of the next step fused — driven by one table row per step:
 *     e  = eps_u + s (eps_c - eps_u)                  (reps = 2; the eps row itself when reps = 1)
 *     d  = px x + pe e                                (Euler / LMS: d = e;  DPM-Solver++: d = x0 = (x - sigma_t e) / alpha_t)
 *     x' = a x + b d + w1 hist[s1] + w2 hist[s2] + w3 hist[s3] + c noise[*step_counter]
 *     hist[slot_now] = d  (slot_now in 0..2);   latents = x';   model_in = cin_next x'
 *   table: device fp32 [n_steps][16], row (*step_counter) =
 *     (px, pe, a, b, w1, w2, w3, c, cin_next, slot_now, s1, s2, s3, cin, 0, 0)
 *   as rcdms_amd.scheduler.*.sigma_table() lays it out; slots are small integers stored as floats, a slot outside 0..2
 *   is not used, hist[s_k] is read only when w_k != 0 and the noise row only when c != 0; cin (this step's input scale) is
 *   not read.  eps rows f16 [(reps*S)*f*H*W][ld] (uncond sample block first); latents, model_in fp32 (S,4,f,H,W), distinct
 *   buffers — model_in is what rcdm_assemble_input reads for the next UNet evaluation; history: device fp32
 *   [3][S*4*f*H*W], caller-owned, no initialisation needed; noise: device fp32 [n_steps][S*4*f*H*W] or NULL when no row
 *   has c != 0.  step_counter as in rcdm_cfg_ddim_step. */
int rcdm_cfg_sigma_step(const void* eps, int32_t ld, float* latents, float* model_in, float* history, const float* noise,
                        int32_t S, int32_t reps, int32_t frames, int32_t H, int32_t W, float guidance_scale,
                        const float* table, const int32_t* step_counter, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Guidance rescale (Lin et al. 2023 §3.4, diffusers `rescale_noise_cfg`; the `guidance_rescale` argument the reference
 *   driver passes, stage2_batchtest_rcdms_model.py:352) inside the captured step.  Per story s, over its n = 4 f H W
 *   elements, with e = eps_u + g (eps_c - eps_u) in fp32 from the f16 eps rows:
 *     factor[s] = phi std(eps_c) / std(e) + (1 - phi)          std unbiased (n - 1), as torch.std
 *   and the step then uses factor[s] e wherever it used e (x0, the multistep history, d of the table form).
 *   A deliberate guard: std(e) == 0 (a constant prediction) gives factor 1 where diffusers divides and hands on inf / nan.
 * rcdm_cfg_rescale_factor: two launches — fixed-order per-block partial sums, shifted by the story's first element, into
 *   `workspace`; then one thread per story adds them in block order in fp64 — so the factors are bitwise reproducible; no
 *   atomics, no counters, and nothing is read from `workspace` that this call did not write (no initialisation needed).
 *   eps as the step kernels take it: f16 rows [(2S)*f*H*W][ld], uncond block first, channels 0..3, ld >= 4; always the two
 *   CFG halves (without CFG there is nothing to rescale).  workspace: 4-byte aligned, at least
 *   rcdm_cfg_rescale_workspace_bytes(S, f, H, W) bytes (0 for sizes <= 0); factor: device fp32 [S].
 *   RCDM_EINVAL: null pointers, sizes <= 0, ld < 4, misaligned pointers; RCDM_ESHAPE: S > 65535; RCDM_EWORKSPACE: a short
 *   workspace — all before any device work.
 * rcdm_cfg_{ddim,pndm,sigma}_step_scaled: the step entries above with `factor` (device fp32 [S], or NULL: no rescale,
 *   exactly the unscaled entry — which forwards here with NULL).  A factor of 1.0f is exact: ones == NULL bit for bit.
 * ---------------------------------------------------------------------------------------------- */
size_t rcdm_cfg_rescale_workspace_bytes(int32_t S, int32_t frames, int32_t H, int32_t W);
int rcdm_cfg_rescale_factor(const void* eps, int32_t ld, int32_t S, int32_t frames, int32_t H, int32_t W,
                            float guidance_scale, float guidance_rescale, void* workspace, size_t workspace_bytes,
                            float* factor, void* stream);
int rcdm_cfg_ddim_step_scaled(const void* eps, int32_t ld, float* latents, int32_t S, int32_t reps,
                              int32_t frames, int32_t H, int32_t W, float guidance_scale, const float* coef,
                              const int32_t* step_counter, const float* factor, void* stream);
int rcdm_cfg_pndm_step_scaled(const void* eps, int32_t ld, float* latents, float* history, int32_t S, int32_t reps,
                              int32_t frames, int32_t H, int32_t W, float guidance_scale, const float* table,
                              const int32_t* step_counter, const float* factor, void* stream);
int rcdm_cfg_sigma_step_scaled(const void* eps, int32_t ld, float* latents, float* model_in, float* history,
                               const float* noise, int32_t S, int32_t reps, int32_t frames, int32_t H, int32_t W,
                               float guidance_scale, const float* table, const int32_t* step_counter,
                               const float* factor, void* stream);
/* Stage-1 prior, per step of prior_pipeline.py:311-344.
 * rcdm_prior_assemble: tok[(b, l)] (f16, B*L rows of C) <- base rows, except l == time_row <- temb (one fp32 row of C);
 *   x16[b] (f16, E) <- latents[b % n_lat] (fp32): the `torch.cat([latents] * 2)` of :314 and the sequence concat of
 *   myprior_transformer.py:363-387 without re-projecting what does not change between steps.
 * rcdm_cfg_unclip_step: x0 = clamp(u + s (c - u), +-clip_range) with u / c = rows r / n + r of pred (f16, ld);
 *   latents[r] = coef[*step][0] x0 + coef[*step][1] latents[r] + coef[*step][2] noise[*step][r]  — the CFG combine
 *   (:328-333) fused with diffusers 0.24.0 UnCLIPScheduler.step for prediction_type "sample" / "fixed_small_log";
 *   coef fp32 [n_steps][3]; noise fp32 [n_steps][n][E] or NULL; clip_range <= 0 disables the clamp. */
int rcdm_prior_assemble(const void* base, const float* temb, const float* latents, int32_t n_lat, void* tok, void* x16,
                        int32_t B, int32_t L, int32_t C, int32_t E, int32_t time_row, void* stream);
int rcdm_cfg_unclip_step(const void* pred, int32_t ld, float* latents, int32_t n, int32_t reps, int32_t E,
                         float guidance_scale, float clip_range, const float* coef, const float* noise,
                         const int32_t* step_counter, void* stream);
/* CLIP encoders (transformers CLIPTextModel / CLIPVisionModel, loaded at stage2_batchtest_rcdms_model.py:200-216 and called from
 * RCDMs_pipeline.py:_encode_prompt / prior_pipeline.py), the two embedding layers in front of the transformer stacks.
 * rcdm_embed_tokens: out[r][0..C) = f16(table[ids[r]][:] + pos[r % L][:]) for r < n_rows — CLIPTextEmbeddings.forward.  ids: device
 *   int32 [n_rows]; table fp32 [vocab][C]; pos fp32 [>= L][C]; C % 8 == 0, ldo % 8 == 0 (16-byte stores).  The kernel does NOT
 *   clamp: the caller guarantees 0 <= ids[r] < vocab.
 * rcdm_patch_rows: the im2col of CLIPVisionEmbeddings.patch_embedding (Conv2d(3, C, patch, stride patch, bias=False)): pixels fp32
 *   (B, 3, H, W) -> f16 rows [B * (P + 1)][ldk], P = (H / patch)(W / patch); row b (P + 1) is all zero (the class-token slot), row
 *   b (P + 1) + 1 + p holds patch p flattened in the weight's own (c, ky, kx) order, columns 3 patch^2 .. ldk are zero.  One
 *   rcdm_gemm against the zero-padded [C][ldk] weight with RCDM_EPI_RESIDUAL = the position table (+ class embedding in row 0)
 *   is then the whole embedding.  H, W multiples of patch, ldk % 8 == 0, ldk >= 3 patch^2 (RCDM_ESHAPE otherwise). */
int rcdm_embed_tokens(const int32_t* ids, int32_t n_rows, int32_t L, const float* table, int32_t vocab, const float* pos,
                      int32_t C, void* out, int32_t ldo, void* stream);
int rcdm_patch_rows(const float* pixels, int32_t B, int32_t H, int32_t W, int32_t patch, void* out, int32_t ldk, void* stream);
/* t_out[0..rows) = timesteps[*step_counter] (fp32) — feeds rcdm_timestep_embed inside a graph */
int rcdm_load_timestep(const float* timesteps, const int32_t* step_counter, float* t_out,
                       int32_t rows, void* stream);
int rcdm_advance_step(int32_t* step_counter, void* stream);
/* dst[0..row_floats) = table[*step_counter][0..row_floats) (fp32): the per-step row of a table computed once per
 * schedule — the whole timestep-embedding chain of unet.py:381-389 and the 22 time_emb_proj outputs (resnet.py:191)
 * depend on the timestep only, so the sampling loop evaluates them for all T steps when the schedule is set and a
 * captured step starts with this one copy instead of five serial launches.  row_floats % 4 == 0, 16-byte aligned. */
int rcdm_load_table_row(const float* table, const int32_t* step_counter, float* dst, size_t row_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight repacking (fp32 reference layout -> f16 kernel layout), device to device:
 *   rcdm_pack_f16: elementwise fp32 -> f16.
 *   rcdm_pack_conv3x3: torch (Cout,Cin,3,3) fp32 -> f16 [Cout][9*cin_pad], k = tap*cin_pad + c.
 *   rcdm_pack_conv3x3_up2: torch (Cout,Cin,3,3) fp32 -> f16 [4 phases][Cout][4*Cin] for rcdm_conv3x3 with upsample = 2:
 *   phase = 2a + b (output parity), k = (2r + c)*Cin + ci, value = sum of w[co][ci][ky][kx] over the taps with
 *   (a+ky-1)>>1 == a-1+r and (b+kx-1)>>1 == b-1+c.
 *   rcdm_pack_geglu_rows: FeedForward.net.0.proj weight (8C,K)/bias(8C) -> rows reordered so every
 *   32-row group holds 16 "hidden" rows then the matching 16 "gate" rows (RCDM_EPI_GEGLU): the two
 *   land in the same lane of the 16x16x32 and of the 32x32x16 MFMA accumulator layouts.
 * ---------------------------------------------------------------------------------------------- */
int rcdm_pack_f16(const float* src, void* dst, size_t n, void* stream);
int rcdm_pack_conv3x3(const float* w, int32_t c_out, int32_t c_in, int32_t cin_pad, void* dst,
                      void* stream);
int rcdm_pack_conv3x3_up2(const float* w, int32_t c_out, int32_t c_in, void* dst, void* stream);
/* C[n][m] = A[n][k] B[k][m], fp32 row-major, device to device: composition of two linear maps at pack time (proj_out behind
 * ff.net.2, the context stacks' projections) before the product is rounded to f16.  Fixed summation order; not a hot-path call. */
int rcdm_matmul_f32(const float* A, const float* B, float* C, int32_t n, int32_t k, int32_t m, void* stream);
int rcdm_pack_geglu_rows(const float* w, const float* bias, int32_t n_out /*8C*/, int32_t K,
                         void* w_dst, float* bias_dst, void* stream);

/* Mish activation, fp32 elementwise: y = x * tanh(softplus(x)).  Replaces `Mish.forward`
 * (src/models/resnet.py:215-217); never instantiated by configs/testing.yaml, kept for drop-in completeness. */
int rcdm_mish(const float* x, float* y, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Images: uint8 frames in, uint8 frames out.
 *
 * rcdm_image_resample: Pillow's ImagingResample for 8-bit channels, the arithmetic under the driver's two preprocessors
 *   (stage2_batchtest_rcdms_model.py:172-196,255-276: CLIPImageProcessor's bicubic shortest-edge resize + centre crop +
 *   rescale + normalise, and ToPILImage -> Resize -> ToTensor -> Normalize(0.5, 0.5)), bit for bit: one launch resamples
 *   n equally sized HWC images, horizontal pass first (rounded to uint8), vertical pass over it; the intermediate image
 *   lives in LDS only.  The caller builds the integer tables (Pillow's precompute_coeffs + normalize_coeffs_8bpc, in double):
 *     kx int32 [out_w][taps_x]  coefficients of output column x, 22 fractional bits, entries past the count unused
 *     bx int32 [out_w][2]       (first source column, count <= taps_x) of output column x
 *     ky / by                   the same for rows.
 *   One pass per axis: acc = 2^21 + sum_i pix[first + i] * k[i] in int32, out = clamp(acc >> 22, 0, 255).  An axis Pillow
 *   skips (size kept, no box) is the table (k = 2^22, count 1), which is the identity.  A crop after the resize is a table
 *   that holds only the rows / columns inside the crop window: out_h x out_w is the window.  The kernel clamps every table
 *   entry to the source image, so a wrong table gives wrong pixels, never an access outside `src`.
 *   tile_rows: the largest number of source rows (max(first + count) - min(first)) that the output rows of one
 *   RCDM_IMAGE_TILE-row tile (rows t * TILE .. t * TILE + TILE - 1) read; sizes the LDS of the launch
 *   (rcdm_image_resample_lds_bytes: 0 for a descriptor the entry point would refuse; more than 64 KiB is RCDM_ESHAPE).
 *   Output modes, channel c of the output = channel (flip_channels ? 2 - c : c) of the source (BGR <-> RGB):
 *     RCDM_IMAGE_U8        uint8 HWC, dst_pitch / dst_stride bytes per row / per image
 *     RCDM_IMAGE_F32_NCHW  fp32 (n, 3, out_h, out_w) dense: (u8 * (1/255) - mean[c]) * (1 / std[c]), every step rounded to fp32
 *     RCDM_IMAGE_F16_ROWS  f16 pixel rows [n * out_h * out_w][ld] (the activation layout above): the fp32 value of
 *                          RCDM_IMAGE_F32_NCHW rounded once to f16 in channels 0..2, zeros in channels 3..c_pad
 *                          (c_pad % 8 == 0, ld % 8 == 0, ld >= c_pad >= 8, dst 16-byte aligned).
 *   Limits (RCDM_ESHAPE): channels == 3, taps <= 40 per axis (an 8x bicubic reduction), sides <= 8192, n <= 65535.  Null
 *   pointers, a pitch below 3 * width, an unknown mode, std <= 0: RCDM_EINVAL.  All checked before anything is launched.
 * rcdm_frames_to_u8: the back end, RCDMs_pipeline.py:274-287 + the driver's (x * 255).astype(uint8):
 *   u8 = trunc(clamp(x * 0.5 + 0.5, 0, 1) * 255) in fp32 (the product by 255 rounded on its own; NaN -> 0) from either the VAE
 *   decoder's f16 pixel rows [n * H * W][ld] (ld >= 3, channels 0..2) or an fp32 (n, 3, H, W) tensor, to uint8 HWC at
 *   dst + image * dst_stride + y * dst_pitch + 3 x: with dst_stride = 3 W and dst_pitch = the pitch of a grid image the n
 *   frames land side by side in one row of cells.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_IMAGE_TILE 32
#define RCDM_IMAGE_U8 0
#define RCDM_IMAGE_F32_NCHW 1
#define RCDM_IMAGE_F16_ROWS 2
typedef struct {
  int64_t src_pitch, src_stride;   /* bytes between source rows / source images */
  int64_t dst_pitch, dst_stride;   /* RCDM_IMAGE_U8: bytes between output rows / output images */
  int32_t n, channels;
  int32_t in_h, in_w, out_h, out_w;
  int32_t taps_x, taps_y;          /* row length of kx / ky */
  int32_t tile_rows;
  int32_t flip_channels;
  int32_t mode;                    /* RCDM_IMAGE_* */
  int32_t ld, c_pad;               /* RCDM_IMAGE_F16_ROWS */
  float mean[3], std[3];           /* RCDM_IMAGE_F32_NCHW / _F16_ROWS, per OUTPUT channel */
} rcdm_resample_desc;
size_t rcdm_image_resample_lds_bytes(const rcdm_resample_desc* d);
int rcdm_image_resample(const rcdm_resample_desc* d, const void* src, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                        const int32_t* by, void* dst, void* stream);

#define RCDM_FRAMES_F16_ROWS 0
#define RCDM_FRAMES_F32_NCHW 1
typedef struct {
  int64_t dst_pitch, dst_stride;   /* bytes between output rows / output images */
  int32_t n, H, W, channels;       /* channels == 3 */
  int32_t src_kind;                /* RCDM_FRAMES_* */
  int32_t ld;                      /* RCDM_FRAMES_F16_ROWS: row stride in elements */
} rcdm_frames_u8_desc;
int rcdm_frames_to_u8(const rcdm_frames_u8_desc* d, const void* src, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG: n equally sized uint8 RGB images on the device (HWC, src_pitch bytes between rows, src_stride between images — the
 * buffers rcdm_frames_to_u8 writes, the cells of a grid included) -> n complete PNG files in device memory + their sizes.
 * What the driver does per story with PIL.Image.save (stage2_batchtest_rcdms_model.py:378-401).  The files are plain PNG
 * (8-bit, colour type 2, no interlace, no ancillary chunks) that any decoder reads; the deflate stream is LITERALS ONLY:
 *   filter     per scanline with bpp = 3, the row above the first row is zeros.  RCDM_PNG_ADAPTIVE: all five filters (None,
 *              Sub, Up, Average, Paeth) are tried, cost = sum over the row's bytes of (v < 128 ? v : 256 - v), the smallest
 *              cost wins, the lowest filter number on a tie.  filter = 0..4: that filter for every row.
 *   blocks     the filtered stream of an image, h * (1 + 3 w) bytes, is cut every RCDM_PNG_BLOCK bytes regardless of rows.
 *              Each cut is one dynamic-Huffman block (BFINAL 0) over 256 literals + end-of-block: HLIT 257, HDIST 1 with
 *              the one distance length 0, HCLEN 19, code-length code fixed (symbols 0..15: 4 bits, 16..18 unused), so the
 *              header is 1103 bits behind the 3 block-type bits.  Behind its end-of-block code comes an empty stored block
 *              (3 bits, pad to a byte, 00 00 FF FF) whose BFINAL is 1 behind the image's last block only.
 *   code       Huffman over the block's histogram, end-of-block counting 1, by the two-queue construction: leaves ascending
 *              by (count, symbol index); internal nodes in creation order; the leaf queue wins a tie.  If the tree is deeper
 *              than 15 every non-zero count becomes (c + 1) >> 1 and it is rebuilt, until it fits.  Canonical codes (RFC 1951
 *              3.2.2).  A block of one distinct byte gets length 1 for it and for end-of-block.
 *   container  signature, IHDR, one IDAT per block — the first starts with the zlib header 78 01, the last ends with the
 *              Adler-32 of the whole filtered stream —, IEND; every chunk with its CRC-32.
 * No match search: a file is never smaller than 1 bit per filtered byte (h (1 + 3 w) / 8 bytes), so flat images come out
 * many times larger than zlib's; on noisy decoder-like frames the size is about Pillow's default.
 *   rcdm_png_bound            worst-case bytes of ONE file (0 for a descriptor the entry point refuses); dst_stride >= it
 *   rcdm_png_workspace_bytes  filtered streams + one RCDM_PNG_SLOT-byte slot and one 16-byte record per block
 *   rcdm_png_encode           three launches on `stream`, no host readback: file i lies at dst + i * dst_stride, its length in
 *                             sizes[i] (device memory, 8-byte aligned); bytes of the stream's slot past sizes[i] are not
 *                             written.  workspace: 16-byte aligned, read and written; src is only read.
 * RCDM_EINVAL: null pointers, src_pitch < 3 w, negative src_stride, dst_stride < rcdm_png_bound when n > 1, channels != 3,
 * a filter outside -1..4, n < 1, a misaligned workspace / sizes.  RCDM_ESHAPE: a side outside 1..8192, n > 65535.  All
 * checked before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_PNG_BLOCK 32768
#define RCDM_PNG_SLOT 41728
#define RCDM_PNG_ADAPTIVE (-1)
typedef struct {
  int64_t src_pitch, src_stride;   /* bytes between source rows / source images */
  int64_t dst_stride;              /* bytes between output files */
  int32_t n, h, w, channels;       /* channels == 3 */
  int32_t filter;                  /* RCDM_PNG_ADAPTIVE or 0..4 */
} rcdm_png_desc;
size_t rcdm_png_bound(const rcdm_png_desc* d);
size_t rcdm_png_workspace_bytes(const rcdm_png_desc* d);
int rcdm_png_encode(const rcdm_png_desc* d, const void* src, void* workspace, void* dst, uint64_t* sizes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG, match mode: the same descriptor, the same files except for what a block's dynamic-Huffman block holds — (length,
 * distance) pairs where the filtered stream repeats itself at one of a few fixed distances.  Opt-in; rcdm_png_encode and its
 * bytes are unchanged.  Filtering, the cut every RCDM_PNG_BLOCK filtered bytes, one IDAT per block, the empty stored block
 * behind each, the zlib header, Adler-32 and the container are those of "PNG" above.  With S = 1 + 3 w (a filtered row) and
 * a block [b0, b1) of the image's stream s:
 *   candidates  at position i the distances 1, 2, 3, 4, 6, 9, 12, S - 3, S, S + 3, 2 S, in this order; d is dropped if d < 1,
 *               d > 32768 or d > i.  The source may lie in front of b0, in the image's earlier bytes, never in another
 *               image's.  (For w <= 2 a distance occurs twice; that changes nothing.)
 *   length      of candidate d: the count of k >= 0 with s[i + k] == s[i + k - d], capped at 258 and at b1 - i — a match never
 *               crosses the cut.  The longest candidate is the position's match, the earlier one in the list on a tie; it
 *               is usable from length 4.
 *   parse       greedy from b0: a usable match at i emits (length, distance) and continues at i + length, otherwise the
 *               literal s[i] and i + 1.
 *   match form  a dynamic-Huffman block with HLIT 286, HDIST 30, HCLEN 19 and the same fixed 4-bit code-length code: a
 *               header of 3 + 5 + 5 + 4 + 57 + 316 * 4 = 1338 bits.  Literal / length code over 286 symbols (end-of-block
 *               counts 1), distance code over 30, each by the two-queue construction of "PNG" with its tie rules and its
 *               (c + 1) >> 1 limiter on its own counts; canonical codes.  ONE used distance symbol gets length 1 (RFC 1951
 *               3.2.7).  Length and distance extra bits as in RFC 1951 3.2.5 (length 258 is symbol 285).
 *   fallback    the block's bits in match form, up to and including the end-of-block code, are compared with its bits in the
 *               literal form of "PNG"; the match form is taken only if it is STRICTLY smaller, otherwise the block's bytes
 *               are exactly rcdm_png_encode's.
 * So every block is <= its literal-only size — rcdm_png_bound and RCDM_PNG_SLOT hold for both modes — and a file whose
 * blocks all fall back is byte-identical to rcdm_png_encode's.  There is no hash search and no lazy matching: a flat 256 x
 * 256 cartoon comes out at 0.29 of its literal-only size, 0.85 of zlib level 1's and 1.7 of zlib level 6's on the same stream.
 *   rcdm_png_match_workspace_bytes  the workspace of rcdm_png_encode_match (today the same number as rcdm_png_workspace_bytes)
 *   rcdm_png_encode_match           as rcdm_png_encode: three launches on `stream` (filter, match block, assemble), no host
 *                                   readback, the same layout of dst / sizes, the same alignment rules
 * Argument checks and error codes are those of rcdm_png_encode, all before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
size_t rcdm_png_match_workspace_bytes(const rcdm_png_desc* d);
int rcdm_png_encode_match(const rcdm_png_desc* d, const void* src, void* workspace, void* dst, uint64_t* sizes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PNG, reading: n PNG files, uploaded as ONE byte buffer, -> n uint8 HWC images (RGB or BGR) in device memory.  What the
 * drivers do on the host with cv2.imdecode over the whole test set (stage2_batchtest_rcdms_model.py:41-46, :446-450) and
 * with Image.open(...).convert("RGB") (:256-260, :304-343).  Files of one call may differ in size and kind, so the call
 * takes one record per file.  The HOST walks the container (signature, chunk headers — rcdms_amd/image.py) and fills the
 * records and the IDAT table; the DEVICE does everything that touches the bulk: gathering the IDAT payloads, zlib header,
 * inflate (stored, fixed and dynamic blocks, window 32 K), Adler-32, the five PNG filters, the colour conversion.
 *   scope       bit depth 8, no interlace; colour types 0 grey (replicated), 2 RGB, 3 palette (looked up; an index beyond
 *               plte_entries is black), 4 grey + alpha and 6 RGBA (alpha dropped).  Ancillary chunks are the host's to skip.
 *   kernels     two launches on `stream`, no host readback, graph-capturable.  One wavefront per file in both: inflate
 *               (symbol decode is wave-uniform, a match of length L is copied by L lanes in an LDS ring of the last 32 K),
 *               then unfilter + convert (a lane per row of a 64-row band, each row one pixel behind the row above).
 *   status[i]   0, or the first thing wrong with file i (RCDM_PNG_E* below).  A bad FILE is never a bad CALL: the call
 *               returns 0, the other files come out right, and no byte of a bad file's image is written.
 *   workspace   file i uses RCDM_PNG_FILE_WORKSPACE(zlib_bytes, h * (1 + bpp * w)) bytes at workspace + ws_offset (a
 *               multiple of 16, regions disjoint — the host lays them end to end): its zlib stream, then its inflated
 *               rows.  Read and written, 16-byte aligned; src is only read.
 *   rcdm_png_decode_workspace_bytes  the largest ws_offset + size over the records: what `workspace` must hold.  It is
 *                                    also the only check of the records: 0 for a side outside 1..8192, a colour type
 *                                    not listed, dst_pitch < 3 w, a ws_offset that is no multiple of 16, or n outside
 *                                    1..65535.  rcdm_png_decode itself takes device pointers and cannot look.
 * The records and the IDAT table are the caller's contract, trusted as the host's own work (offsets inside the buffers it
 * uploaded, rows that do not overlap, aligned regions): the kernels do not re-check them, but for a side or colour type
 * out of range, for which nothing can be inflated and status[i] is RCDM_PNG_EUNDERRUN.  Everything
 * that comes out of a FILE's bytes — lengths, distances, code lengths, stored sizes, filter bytes — is checked before a
 * position is formed from it.
 * RCDM_EINVAL: null pointers, n < 1, n_idat < 1, an order other than RCDM_PNG_RGB / RCDM_PNG_BGR, workspace not 16-byte
 * aligned, status not 4-byte aligned, files / idats not 8-byte aligned.  RCDM_ESHAPE: n > 65535.  All before any launch.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_PNG_RGB 0
#define RCDM_PNG_BGR 1
#define RCDM_PNG_EZLIB 1      /* zlib header: CM != 8, window > 32 K, preset dictionary, header checksum */
#define RCDM_PNG_ETRUNC 2     /* the stream ends inside a block or in front of its Adler-32 */
#define RCDM_PNG_EBLOCK 3     /* block type 3 */
#define RCDM_PNG_ESTORED 4    /* stored block: LEN != ~NLEN */
#define RCDM_PNG_ECODES 5     /* code lengths: over-subscribed, incomplete (but for ONE distance code), too many, no end-of-block */
#define RCDM_PNG_ESYMBOL 6    /* length symbol 286 / 287, distance symbol 30 / 31, or bits that no code owns */
#define RCDM_PNG_EDISTANCE 7  /* a distance that reaches in front of the first output byte */
#define RCDM_PNG_EOVERRUN 8   /* the stream inflates to more than h * (1 + bpp * w) bytes */
#define RCDM_PNG_EUNDERRUN 9  /* ... to fewer */
#define RCDM_PNG_EADLER 10    /* Adler-32 of the inflated bytes */
#define RCDM_PNG_EFILTER 11   /* a filter byte above 4 */
#define RCDM_PNG_FILE_WORKSPACE(zlib_bytes, raw_bytes) ((((zlib_bytes) + 15) & ~(uint64_t)15) + (((raw_bytes) + 15) & ~(uint64_t)15))
typedef struct {                   /* one per file, filled by the host from the container */
  uint64_t src_offset, src_bytes;  /* the file inside the uploaded byte buffer */
  uint64_t dst_offset;             /* first output byte of this image */
  uint64_t ws_offset;              /* this file's region of the workspace */
  uint64_t zlib_bytes;             /* sum of its IDAT payloads */
  uint32_t dst_pitch;              /* bytes between output rows, >= 3 w */
  uint32_t w, h;                   /* 1..8192 each */
  uint32_t color_type;             /* 0, 2, 3, 4, 6 */
  uint32_t idat_first, idat_count; /* this file's run in the IDAT table */
  uint32_t plte_offset;            /* colour type 3: the PLTE payload, relative to src_offset */
  uint32_t plte_entries;           /* its length / 3, <= 256 */
} rcdm_png_file;
typedef struct {
  uint64_t offset;                 /* payload of one IDAT chunk, relative to the file's src_offset */
  uint32_t bytes, reserved;
} rcdm_png_idat;
size_t rcdm_png_decode_workspace_bytes(const rcdm_png_file* files, int n);
int rcdm_png_decode(const rcdm_png_file* files, const rcdm_png_idat* idats, int n, int n_idat, int order, const void* src,
                    void* workspace, void* dst, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame metrics: n pairs of equally sized uint8 RGB images on the device (HWC; each side with its own pitch, bytes between
 * rows, and stride, bytes between images — the buffers rcdm_frames_to_u8 and rcdm_image_resample write, the cells of a grid
 * included) -> per pair and channel the mean SSIM and the sums of squared and absolute differences.  What the stage-2 driver
 * is set up for and never computes: it imports skimage's structural_similarity (stage2_batchtest_rcdms_model.py:23) and pairs
 * every generated frame with its resized target (:389-401).  Neither base pointer nor pitch needs any alignment, and no byte
 * beyond the 3 * W bytes of a row is read.
 *   ssim  [n][3] float64: scikit-image's structural_similarity(a, b, channel_axis=-1, data_range=255) per channel, K1 = 0.01,
 *         K2 = 0.03, C1 = (K1 255)^2, C2 = (K2 255)^2.  With F the window mean:
 *           ux = F(x), uy = F(y), vx = cn (F(x x) - ux ux), vy = cn (F(y y) - uy uy), vxy = cn (F(x y) - ux uy)
 *           S  = (2 ux uy + C1)(2 vxy + C2) / ((ux ux + uy uy + C1)(vx + vy + C2))
 *         and the figure is the mean of S over the window positions that lie inside the image (skimage crops the first and
 *         last (win - 1) / 2 rows and columns; there is no border mode).  Its three-channel mean is skimage's return value.
 *           RCDM_SSIM_UNIFORM7  skimage's default, a 7 x 7 box.  The five window sums are integers and the variances are
 *                               NP sum(x x) - sum(x)^2 in integers (NP = 49): nothing cancels in floating point.
 *           RCDM_SSIM_GAUSS11   gaussian_weights=True, sigma=1.5: win[11] float64 = exp(-i^2 / (2 sigma^2)), i = -5..5,
 *                               normalised to sum 1 by the caller; separable passes in float64 over the integer products.
 *                               (win is not read for the box and may be null.)
 *           sample_covariance   cn = NP / (NP - 1) with NP = 49 / 121 (skimage's use_sample_covariance=True, its default),
 *                               0: cn = 1.
 *         Identical images give exactly 1.0.  The sums have a fixed order (no atomics): the same inputs give the same bits.
 *   sse, sad  [n][3] int64: exact sums over the whole image of (a - b)^2 and |a - b|; the mean squared error (the sum of
 *         sse's three channels / (3 H W)), PSNR = 10 log10(255^2 / mse) and the mean absolute error are the caller's to derive.
 *   rcdm_frame_metrics_workspace_bytes  nine 8-byte partials per tile and pair (0 for a descriptor the entry point refuses)
 *   rcdm_frame_metrics                  two launches on `stream`, no host readback, no allocation.  workspace: 8-byte
 *                                       aligned, written then read; a and b are only read.
 * RCDM_EINVAL: null pointers (win with RCDM_SSIM_GAUSS11), n < 1, H or W < 1, an unknown window, a pitch below 3 W, a negative
 * stride, win / ssim / sse / sad / workspace not 8-byte aligned.  RCDM_ESHAPE: channels != 3, H or W below the window side, a
 * side above 8192, n > 65535.  RCDM_EWORKSPACE: workspace null or short.  All checked before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_SSIM_UNIFORM7 0
#define RCDM_SSIM_GAUSS11 1
typedef struct {
  int64_t a_pitch, a_stride;       /* bytes between rows / images of a */
  int64_t b_pitch, b_stride;       /* ... of b */
  int32_t n, H, W, channels;       /* channels == 3 */
  int32_t window;                  /* RCDM_SSIM_* */
  int32_t sample_covariance;       /* non-zero: cn = NP / (NP - 1) */
} rcdm_metrics_desc;
size_t rcdm_frame_metrics_workspace_bytes(const rcdm_metrics_desc* d);
int rcdm_frame_metrics(const rcdm_metrics_desc* d, const void* a, const void* b, const double* win, double* ssim, int64_t* sse,
                       int64_t* sad, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fréchet distance: running float64 statistics of feature rows on the device, and the distance
 *   |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2)
 * between two sets of them (FID when the rows are Inception pool features; here the CLIP image embeddings the story runner
 * already holds, a "CLIP-FD").  The reference drivers compute no set-level figure.  tr (S_a S_b)^(1/2) is the sum of the
 * singular values of F_b^T F_a for factors S = F F^T; both the factors and the singular values come from one-sided (Hestenes)
 * Jacobi on the rows of a buffer (csrc/frechet_core.h: pairing, rotation, rules 1-3).  No matrix square root is taken and no
 * matrix is squared.  Every sum has a fixed order and nothing but the rotation counter is atomic: the same inputs give the
 * same bits.  All buffers are on the device; float64 pointers are 8-byte aligned.  1 <= d <= 4096.
 *   rcdm_feature_stats_update    x: n rows of d features, RCDM_FSTATS_F32 or _F16, ld elements between rows (columns d..ld are
 *                                never read); shift: float32[d], the point the sums are taken about.  sum[d] += sum_r (x_r - k),
 *                                outer[d][d] (dense) += sum_r (x_r - k)(x_r - k)^T, operands widened to float64 before the
 *                                subtraction, the outer product on the float64 matrix pipe.  Two launches.  The column sums
 *                                are one thread per column over all n rows (d / 256 workgroups, a chain of n additions):
 *                                measured at n = 1000 only; a caller with millions of rows should pass them in chunks.
 *   rcdm_gemm_tn_f64             c[m][n] = a^T b for a[k][m], b[k][n], float64 (the same kernel, on doubles, without a shift).
 *   rcdm_feature_stats_finalize  mean[d] = k + sum / n; with cov != null (n >= 2): cov[d][d] = (outer - sum sum^T / n) / (n - 1),
 *                                both triangles written from the upper one of `outer`, and trace[0] = tr cov.
 *   rcdm_frechet_trace           out[0] = the trace of a dense d x d matrix;  rcdm_frechet_mean_term  out[0] = |mu_a - mu_b|^2.
 *   rcdm_jacobi_sweep            one sweep over w: `rows` vectors (even; an odd dimension is padded with one zero vector) of
 *                                `len` doubles, ld doubles apart; dim: the dimension the thresholds of rules 2 and 3 use.
 *                                rows + 1 launches: the norms, the sweep's threshold, and one launch per round of rows / 2
 *                                disjoint pairs.  *count (int32) is zeroed and then holds the rotations of the sweep: the caller
 *                                reads it back and stops at 0.  No launch waits on another workgroup.
 *   rcdm_jacobi_norm_sum         out[0] = the sum of the vectors' norms (after the last sweep: of the singular values),
 *                                out[1] = the largest.
 *   rcdm_frechet_factor          len == dim: after the last sweep over a covariance, vector j is lambda_j v_j.  f[len][ldf >= rows]
 *                                gets column j = w_j / sqrt(lambda_j), or zeros where lambda_j <= dim 2^-52 lambda_max (rule 3);
 *                                *rank (int32) = the columns kept.  f^T f' is then rcdm_gemm_tn_f64's to form.
 *   rcdm_jacobi_workspace_bytes  (4 + rows) doubles, shared by the three entry points above (0 for a refused descriptor).
 *   rcdm_cholesky_pivoted_f64    the other way to a factor: a[d][ld], dense and symmetric, is left intact; f[d][ldf] gets column
 *                                j = column j of P L of the diagonally pivoted Cholesky factorisation, rows in the original
 *                                order, zero columns from the rank on; *rank (int32) = the steps taken.  Step j takes the
 *                                largest remaining diagonal (lowest index on a tie) and stops when it is not above d 2^-52 x the
 *                                largest diagonal of a (zero, negative and NaN diagonals stop it the same way).  Blocked and
 *                                right-looking in panels of nb columns (16, 32, 64 or 128; 0: the library's choice, 16): 1 + 2 d +
 *                                (d - 1) / nb launches, the trailing update on the float64 matrix pipe, no read-back, no
 *                                atomics.  Columns d..ld of a and d..ldf of f are neither read nor written.
 *   rcdm_cholesky_workspace_bytes  8 + d d + nb d + 2 d doubles and 2 (d rounded up to even) int32 (0 for a refused descriptor).
 * RCDM_EINVAL: null pointers, n or d < 1, ld < d (len, rows, the GEMM's sizes), an unknown dtype, odd rows, a misaligned
 * pointer, cov with n < 2.  RCDM_ESHAPE: d, rows, len or dim above 4096, n above 2^30.  RCDM_EWORKSPACE: workspace null or short.
 * All checked before anything is launched; no allocation.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_FSTATS_F32 0
#define RCDM_FSTATS_F16 1
typedef struct {
  int64_t ld;                      /* elements between rows of x, >= d */
  int32_t n, d;
  int32_t dtype;                   /* RCDM_FSTATS_* */
  int32_t reserved;
} rcdm_fstats_desc;
typedef struct {
  int64_t ld;                      /* doubles between vectors, >= len */
  int32_t rows, len, dim;
  int32_t reserved;
} rcdm_jacobi_desc;
int rcdm_feature_stats_update(const rcdm_fstats_desc* d, const void* x, const float* shift, double* sum, double* outer,
                              void* stream);
int rcdm_gemm_tn_f64(int32_t m, int32_t n, int32_t k, const double* a, int64_t lda, const double* b, int64_t ldb, double* c,
                     int64_t ldc, void* stream);
int rcdm_feature_stats_finalize(int32_t d, int64_t n, const float* shift, const double* sum, const double* outer, double* mean,
                                double* cov, double* trace, void* stream);
int rcdm_frechet_trace(int32_t d, const double* a, double* out, void* stream);
int rcdm_frechet_mean_term(int32_t d, const double* mu_a, const double* mu_b, double* out, void* stream);
size_t rcdm_jacobi_workspace_bytes(const rcdm_jacobi_desc* d);
int rcdm_jacobi_sweep(const rcdm_jacobi_desc* d, double* w, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
int rcdm_jacobi_norm_sum(const rcdm_jacobi_desc* d, const double* w, double* out, void* workspace, size_t workspace_bytes,
                         void* stream);
int rcdm_frechet_factor(const rcdm_jacobi_desc* d, const double* w, double* f, int64_t ldf, int32_t* rank, void* workspace,
                        size_t workspace_bytes, void* stream);
typedef struct {
  int64_t ld;                      /* doubles between rows of a, >= d */
  int64_t ldf;                     /* doubles between rows of f, >= d */
  int32_t d;
  int32_t nb;                      /* panel width: 16, 32, 64, 128, or 0 for the library's choice */
} rcdm_cholesky_desc;
size_t rcdm_cholesky_workspace_bytes(const rcdm_cholesky_desc* d);
int rcdm_cholesky_pivoted_f64(const rcdm_cholesky_desc* d, const double* a, double* f, int32_t* rank, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel distance: the unbiased squared maximum mean discrepancy under a polynomial kernel, over subsets of stored feature
 * rows (KID: Binkowski et al., "Demystifying MMD GANs", 2018; here on CLIP image embeddings, a "CLIP-KID").  The companion of
 * the Fréchet distance for few samples: no covariance, no factorisation, no sweeps.  csrc/kid_core.h holds the arithmetic,
 * shared with tools/kid_host.cpp; restated from the definition, not pinned against torch-fidelity, torchmetrics or clean-fid.
 *   kernel      k(x, y) = (gamma <x, y> + coef0)^degree, degree an integer in 1 .. 8 (KID: gamma = 1 / d, coef0 = 1, degree = 3).
 *   one subset  index lists ia[0..m) into the rows of x and ib[0..m) into the rows of y, m >= 2:
 *                 Sxx = sum over POSITIONS i != j of k(x_ia[i], x_ia[j]), Syy the same over y,
 *                 Sxy = sum over all i, j of k(x_ia[i], y_ib[j]),
 *                 mmd2 = (Sxx / (m (m - 1)) + Syy / (m (m - 1))) - 2 (Sxy / (m m)), evaluated in that order in float64, with
 *                 m (m - 1) and m m formed in int64 and converted once.
 *               The diagonal mask goes by position, not by row number: a list with a repeated row is well defined.
 *   KID         the mean of mmd2 over the subsets and their population standard deviation (ddof = 0): the caller's to take.
 *   arithmetic  float32 / float16 features are widened exactly (every product is exact in float64), the dot is summed in
 *               float64 on the matrix pipe, t = fl(fl(gamma dot) + coef0) without contraction, k = ((t t) t) ... left to right.
 *               Positions outside the subset and the masked diagonal are skipped in the epilogue (a padded row that enters
 *               the matrix pipe as 0.0 has k = coef0^degree: zero operands mask nothing).  Every reduction has a fixed order
 *               and no atomics — a lane's 16 values in register order, a tree over the 256 threads of a 64 x 64 tile, then the
 *               tile partials of one (subset, block) through the fixed sum of the Fréchet entries in a second launch, which
 *               also forms mmd2 — so the same input gives the same bits.  The symmetric blocks are computed from their
 *               upper-triangle tiles only; an off-diagonal tile counts twice (exact).
 *   rcdm_poly_mmd         x[nx][ldx], y[ny][ldy]: RCDM_FSTATS_F32 or _F16 rows (columns d..ld are never read); ix, iy:
 *                         int32 [subsets][m], or null for rows 0 .. m - 1 in every subset; out: double [subsets][4] = Sxx, Syy,
 *                         Sxy, mmd2.  All subsets and all three blocks in one launch of the tile kernel plus one of the reduce.
 *                         Row addresses are formed in int64.  The indices are the caller's responsibility: they are not
 *                         checked on the device.  x == y is allowed.
 *   rcdm_poly_gram_f64    the first subset of the descriptor only: out[m][ldo >= m] = k(x_ia[i], y_ib[j]), unmasked, from the
 *                         same tile body with a storing epilogue (a kernel matrix for other two-sample tests).
 *   rcdm_poly_mmd_workspace_bytes   subsets x 3 x ceil(m / 64)^2 doubles (0 for a refused descriptor).
 * RCDM_EINVAL: null descriptor, x, y or out; d < 1, m < 2, subsets, nx or ny < 1, ld < d, ldo < m, degree outside 1 .. 8, an
 * unknown dtype, flags != 0, a misaligned pointer, a null list with m above the rows there are.  RCDM_ESHAPE: d > 4096,
 * m > 65536, subsets > 65535.  RCDM_EWORKSPACE: workspace null or short.  All checked before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t ldx, ldy;                /* elements between rows of x and of y, >= d */
  int32_t nx, ny, d;               /* rows of x and of y, features per row */
  int32_t subsets, m;              /* index lists, rows per list */
  int32_t degree;                  /* 1 .. 8 */
  int32_t dtype;                   /* RCDM_FSTATS_* */
  double gamma, coef0;
  uint32_t flags;                  /* 0 */
} rcdm_mmd_desc;
size_t rcdm_poly_mmd_workspace_bytes(const rcdm_mmd_desc* d);
int rcdm_poly_mmd(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy, double* out,
                  void* workspace, size_t workspace_bytes, void* stream);
int rcdm_poly_gram_f64(const rcdm_mmd_desc* d, const void* x, const void* y, const int32_t* ix, const int32_t* iy, double* out,
                       int64_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Manifold figures: improved precision and recall (Kynkaanniemi et al., 2019) and density and coverage (Naeem et al., 2020)
 * over stored feature rows — whether a model lost fidelity or lost diversity, which one distance cannot say.
 * csrc/prdc_core.h holds the arithmetic, shared with tools/prdc_host.cpp.  Restated from the papers; not pinned against prdc,
 * torch-fidelity or torchmetrics.
 *   inputs      real rows x[nx][ldx] and generated rows y[ny][ldy], RCDM_FSTATS_F32 or _F16 (columns d..ld are never read),
 *               widened exactly.  k = nearest_k, an integer in 1 .. 16; nx, ny >= k + 1.
 *   distance    D2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>) in float64 with no contraction.  |a|^2 is summed from the exact
 *               products through the fixed sum of the Fréchet entries (256 strided partial sums, then the tree); the dot is
 *               summed in float64 on the matrix pipe.  Every comparison is made on squared distances: no square root.
 *   radius      rX2[i] = the k-th smallest of { D2(x_i, x_j) : j != i }, counted with multiplicity.  Self-exclusion goes BY
 *               POSITION, as the kernel distance's diagonal mask does: a repeated row is its twin's neighbour at distance 0.
 *               rY2 the same over y.
 *   balls       closed (<=) in all four figures:
 *                 fake_count[j] = #{ i : D2(x_i, y_j) <= rX2[i] }
 *                 real_hit[i]   = 1 if some j has D2(x_i, y_j) <= rY2[j], else 0
 *                 real_min2[i]  = min_j D2(x_i, y_j)
 *   figures     precision = #{ j : fake_count[j] > 0 } / ny          recall   = sum_i real_hit[i] / nx
 *               density   = sum_j fake_count[j] / (k ny)              coverage = #{ i : real_min2[i] <= rX2[i] } / nx
 *               out[4] = the four NUMERATORS as int64, in the order precision, recall, density, coverage; the divisions are
 *               the caller's, once, in float64.
 *   deviation   the prdc package compares strictly; the two rules differ on exact ties only.
 *   masks       positions outside a set, and the position-diagonal of the radius sweep, are masked in the epilogue: a padded
 *               row enters the matrix pipe as the zero vector, which is a real point near a centred cloud — zero operands mask
 *               nothing.
 *   order       every reduction after the distances is a k-smallest selection, an integer sum, an or or a minimum: the same
 *               input gives the same bits whatever col_chunks is.  No atomics.
 *   rcdm_row_norms2_f64   out[n] = |x_i|^2 in float64, the fixed sum; one launch.
 *   rcdm_knn_radii2       r2[n].  Grid (row strips of 64, column chunks); each chunk keeps k candidates per row in the workspace,
 *                         a second launch merges them.  col_chunks = 0: the library chooses enough chunks to fill 256 compute
 *                         units at this n (eight workgroups each, at most one chunk per tile column); 1 .. 1024: the caller's (more chunks than tile columns is allowed).  The distance
 *                         matrix never reaches memory.
 *   rcdm_prdc_counts      rx2[nx], ry2[ny]: the radii (of rcdm_knn_radii2 or the caller's own).  out: int64[4]; fake_count:
 *                         int32[ny]; real_hit: int32[nx]; real_min2: double[nx]; all caller-owned, all fully written.  One sweep
 *                         of the nx x ny tiles, a fold launch and a last launch of one workgroup.  x == y is allowed.
 *   *_workspace_bytes     radii: (1 + chunks k) n doubles.  Counts: nx + ny + chunks nx doubles, 4 int64 per 256 of
 *                         max(nx, ny), chunks nx int32 and ceil(nx / 64) ny bytes, each part rounded up to 8 bytes.  0 for a
 *                         refused descriptor.
 * RCDM_EINVAL: a null descriptor or pointer; d < 1, n < 1, ld < d, k outside 1 .. 16, n < k + 1, col_chunks outside 0 .. 1024,
 * an unknown dtype, flags != 0, a misaligned pointer (rows at their element size, int32 at 4, double / int64 / workspace at 8).
 * RCDM_ESHAPE: d > 4096, n > 65536.  RCDM_EWORKSPACE: workspace null or short.  All checked before anything is launched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t ld;                      /* elements between rows, >= d */
  int32_t n, d;                    /* rows, features per row */
  int32_t k;                       /* nearest_k, 1 .. 16 */
  int32_t dtype;                   /* RCDM_FSTATS_* */
  int32_t col_chunks;              /* 0: the library chooses */
  uint32_t flags;                  /* 0 */
} rcdm_knn_desc;
typedef struct {
  int64_t ldx, ldy;                /* elements between rows of x and of y, >= d */
  int32_t nx, ny, d;               /* real rows, generated rows, features per row */
  int32_t dtype;                   /* RCDM_FSTATS_* */
  int32_t col_chunks;              /* 0: the library chooses */
  uint32_t flags;                  /* 0 */
} rcdm_prdc_desc;
int rcdm_row_norms2_f64(const void* x, int32_t n, int32_t d, int64_t ld, int32_t dtype, double* out, void* stream);
size_t rcdm_knn_radii2_workspace_bytes(const rcdm_knn_desc* d);
int rcdm_knn_radii2(const rcdm_knn_desc* d, const void* x, double* r2, void* workspace, size_t workspace_bytes, void* stream);
size_t rcdm_prdc_counts_workspace_bytes(const rcdm_prdc_desc* d);
int rcdm_prdc_counts(const rcdm_prdc_desc* d, const void* x, const void* y, const double* rx2, const double* ry2, int64_t* out,
                     int32_t* fake_count, int32_t* real_hit, double* real_min2, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scores from logits: the multi-label counts behind Char-F1 / Frm-Acc (the character classifier of the story-visualisation
 * papers) and the Inception Score, over classifier logits that are already on the device.  csrc/scores_core.h holds every
 * rule and every summation order, shared with tools/scores_host.cpp.  Restated from the definitions; the label figures are
 * held against scikit-learn, the Inception Score is not pinned against torch-fidelity / torchmetrics.
 *   label counts  logits[n][ld_logits]: RCDM_FSTATS_F32 or _F16; labels[n][ld_labels]: bytes; classes = 1 .. 64 columns of
 *                 each are read.  Prediction: logit > threshold[c], strictly, in float32 (thresholds: float32[classes], or
 *                 null: all 0.0); a NaN predicts 0; a label is 1 when its byte is non-zero.
 *     state       int64[rcdm_label_state_len(classes)] = [n | tp, fp, fn per class | H[t][e], (classes + 1)^2], H counting
 *                 the rows with t true positives and e false positives + false negatives.  rcdm_label_counts ADDS its n rows
 *                 into the state in place on the caller's stream: no read-back, no memset (the caller zeroes a new state).
 *                 Integer sums: exact, and two states merge by addition.  Two launches, no atomics.
 *     workspace   one int32 state per 256 rows, rounded up to 8 bytes.
 *   Inception Score  logits[n][ld]: classes = 2 .. 4096; order: int32[n] row numbers (position p reads row order[p]; every
 *                 entry in 0 .. n - 1, not checked) or null: the given order.  Split k = positions [k n / splits,
 *                 (k + 1) n / splits).  kl_out[splits]: mean over the split's rows of KL(p_row || p_mean), in float64; the
 *                 score is exp of it.  row_h: null, or double[n]: sum_c p_c log p_c of the row at each position.  Three
 *                 launches (a wave per row; a thread per class over chunks of 256 positions; a block per split), no atomics,
 *                 fixed summation orders: the same input gives the same bits, whatever chunks_per_block (how many chunks one
 *                 block of the second launch walks; 0: the library chooses, else 1 .. 64).
 *     workspace   3 n + splits x slots x (classes + 1) doubles, slots = ceil(ceil(n / splits) / 256).
 * RCDM_EINVAL: a null descriptor or pointer (thresholds, order and row_h may be null); n < 1, splits < 1, splits > n, ld below
 * classes, an unknown dtype, chunks_per_block outside 0 .. 64, flags != 0, a misaligned pointer (logits at their element size,
 * thresholds and order at 4, state, kl_out, row_h and workspace at 8).  RCDM_ESHAPE: classes outside the range, n > 2^30,
 * splits > 65535.  RCDM_EWORKSPACE: workspace null or short.  All checked before anything is launched; the *_workspace_bytes
 * and rcdm_label_state_len give 0 for what would be refused.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t ld_logits;               /* elements between rows of logits, >= classes */
  int64_t ld_labels;               /* bytes between rows of labels, >= classes */
  int32_t n, classes;
  int32_t dtype;                   /* RCDM_FSTATS_*: the logits */
  uint32_t flags;                  /* 0 */
} rcdm_label_desc;
typedef struct {
  int64_t ld;                      /* elements between rows of logits, >= classes */
  int32_t n, classes, splits;
  int32_t dtype;                   /* RCDM_FSTATS_* */
  int32_t chunks_per_block;        /* 0: the library chooses */
  uint32_t flags;                  /* 0 */
} rcdm_isc_desc;
int64_t rcdm_label_state_len(int32_t classes);
size_t rcdm_label_counts_workspace_bytes(const rcdm_label_desc* d);
int rcdm_label_counts(const rcdm_label_desc* d, const void* logits, const uint8_t* labels, const float* thresholds, int64_t* state,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t rcdm_inception_score_workspace_bytes(const rcdm_isc_desc* d);
int rcdm_inception_score(const rcdm_isc_desc* d, const void* logits, const int32_t* order, double* kl_out, double* row_h,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Denoising objective: what surrounds the UNet when the stage-2 training quantity F.mse_loss(noise_pred, noise) is evaluated
 * at one random timestep per story (train_stage2.py:420-486), without an fp32 NCFHW tensor on either side of the network.
 * csrc/objective_core.h holds every rule and the order of every sum, shared with tools/objective_host.cpp.  Restated from
 * train_stage2.py and the diffusers DDPMScheduler.add_noise formula; not pinned against diffusers.  Forward only.
 *   rcdm_diffuse_assemble   one launch.  x0, noise, masked: fp32 (B,4,f,H,W); mask: fp32 (B,1,f,H,W); offs: fp32 (B,4,f) or
 *                 null — the noise_offset term of train_stage2.py:445-449, n = noise + offs_scale * offs[b][c][f], the product
 *                 and the sum each rounded to fp32; t: int64[B] ON THE DEVICE, never read by the host; table: fp32 [T][2] =
 *                 (sqrt(a_t), sqrt(1 - a_t)).  out rows [(B*f*H*W)][ld] f16 in rcdm_assemble_input's channel layout:
 *                 channels 0..3 = f16((sa * x0) + (s1m * n)), every product and sum rounded to fp32 on its own and never
 *                 contracted into an fma — the bits of torch's mul, mul, add and .half() —, channel 4 = mask, 5..8 = masked,
 *                 9..c_pad-1 = 0; columns c_pad..ld are not touched.  A story whose t is outside [0, T) reads nothing from
 *                 the table and gets the f16 NaN 0x7E00 in channels 0..3.  A row is stored as c_pad / 8 16-byte vectors.
 *   rcdm_eps_sqerr  out[B][f] (float64) = sum over the frame's 4 H W elements of (double(eps) - double(n))^2; eps: the UNet's f16
 *                 output rows [(B*f*H*W)][ld], channels 0..3; n formed from noise / offs / offs_scale as above.  Two launches
 *                 (chunks of 256 pixels of a frame, then a fold), fixed order: a pixel's four channels ascending, a binary
 *                 tree over the chunk, the chunk sums ascending.  No atomics, no memset: the same bits for every `blocks`
 *                 (the grid of the first launch; 0: the library chooses, else 1 .. 65535) and on every rerun.  NaN and inf
 *                 propagate.
 *     workspace   B * f * ceil(H W / 256) doubles.
 * RCDM_EINVAL: a null pointer (offs may be null), a dimension or T below 1, blocks outside 0 .. 65535, a misaligned pointer
 * (fp32 operands at 4, t, out[B][f], eps and the workspace at 8, the input rows at 16).  RCDM_ESHAPE: B f H W >= 2^31; c_pad
 * below 16, above 1024 or no multiple of 8, ld below c_pad or no multiple of 8 (rcdm_diffuse_assemble); ld below 4 or no
 * multiple of 4 (rcdm_eps_sqerr).  RCDM_EWORKSPACE: workspace null or short.  All checked before anything is launched;
 * rcdm_eps_sqerr_workspace_bytes gives 0 for what would be refused.
 * ---------------------------------------------------------------------------------------------- */
int rcdm_diffuse_assemble(const float* x0, const float* noise, const float* offs, float offs_scale, const int64_t* t,
                          const float* table, int32_t T, const float* mask, const float* masked, int32_t B, int32_t frames,
                          int32_t H, int32_t W, void* out, int32_t ld, int32_t c_pad, void* stream);
size_t rcdm_eps_sqerr_workspace_bytes(int32_t B, int32_t frames, int32_t H, int32_t W);
int rcdm_eps_sqerr(const void* eps, int32_t ld, const float* noise, const float* offs, float offs_scale, int32_t B,
                   int32_t frames, int32_t H, int32_t W, int32_t blocks, double* out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * CLIP tokenizer: n ASCII captions on the device -> the rows transformers.CLIPTokenizer(...)(texts, padding="max_length",
 * max_length=..., truncation=..., return_tensors="pt") returns, what both pipelines ask of their tokenizer
 * (RCDMs_pipeline.py:_encode_prompt, prior_pipeline.py:_encode_prompt), plus what the text encoder otherwise reads back to the
 * host for (row lengths, pooled position).  Pinned to the `tokenizers` backend of transformers 5.x on synthetic vocabularies
 * (tests/golden/tok_*.npz); never run on the real CLIP files.  One launch, one wavefront per caption, no host readback.
 *   1. added tokens   rows with special != 0 (the bos / eos strings) are matched on the raw bytes, then the other rows (add_tokens;
 *                     text lower-cased by the caller) on the lower-cased bytes of each stretch between those matches, also
 *                     inside words.  Leftmost-longest, non-overlapping; each match is the row's id and never merges.
 *   2. normalise      ASCII letters are lower-cased; whitespace is bytes 9-13 and 32.
 *   3. split          's|'t|'re|'ve|'m|'ll|'d|[a-z]+|[0-9]|[^whitespace a-z 0-9]+ in order; whitespace dropped.
 *   4. BPE per word   byte b is byte_ids[b], the word's last byte byte_ids[256 + b] (the </w> form).  Repeat: of the live
 *                     adjacent pairs that the pair table holds, merge the ONE of lowest rank, leftmost first.
 *   5. frame          bos_id, the tokens, eos_id, pad_id up to max_length; attention_mask 1 through eos.  truncation != 0 keeps
 *                     the first max_length - 2 tokens.  With truncation == 0 a longer caption's row is written the same way
 *                     and lengths[i] > max_length tells the caller, who raises.
 *   text, offsets   the captions end to end and n + 1 int32 offsets into them (ascending, offsets[n] <= text_bytes)
 *   byte_ids        int32[512]
 *   added           n_added rcdm_tok_added rows (may be null when n_added == 0)
 *   pairs           pair_slots rcdm_tok_pair slots, an open-addressing table with linear probing from
 *                   rcdm_tok_pair_hash(a, b) & (pair_slots - 1); an empty slot has a == 0xFFFFFFFF; at most half full
 *   input_ids, attention_mask   int64, row i at element i * ld
 *   lengths         int32[n]: tokens + 2, not truncated; -1 for a caption the kernel refuses (longer than
 *                   RCDM_TOK_MAX_CAPTION, a byte >= 0x80, offsets out of order or outside text): its row is that of ""
 *   pool_index      int32[n][2]: position of the row's largest id (the first of equals: the rule of eos_token_id == 2
 *                   configurations — a token of add_tokens outranks eos there, as in transformers) and of its first eos_id
 * rcdm_clip_tokenize_workspace_bytes: a caption's symbols live in LDS, so this is 0 for every descriptor the entry point
 * takes; it is there so that a later layout can need one.  workspace may be null when it is 0.
 * RCDM_EINVAL: null pointers, n < 1, max_length < 2, ld < max_length, a negative id, n_added or text_bytes, pair_slots no power
 * of two, input_ids / attention_mask not 8-byte, pairs not 16-byte, the others not 4-byte aligned.  RCDM_ESHAPE: n >
 * RCDM_TOK_MAX_CAPTIONS, max_length > RCDM_TOK_MAX_CAPTION + 2, n_added > RCDM_TOK_MAX_ROWS, text_bytes >= 2^31, pair_slots >
 * 2^26.  RCDM_EWORKSPACE: workspace short (or null when bytes are needed).  All before the device is touched.
 * ---------------------------------------------------------------------------------------------- */
#define RCDM_TOK_MAX_CAPTION 1024     /* bytes of one caption */
#define RCDM_TOK_MAX_ADDED 64         /* tokens of add_tokens */
#define RCDM_TOK_MAX_ROWS 66          /* ... plus the two special strings: rows of the added table */
#define RCDM_TOK_MAX_ADDED_LEN 32     /* bytes of one row */
#define RCDM_TOK_MAX_RANK (1 << 22)   /* ranks are below this */
#define RCDM_TOK_MAX_CAPTIONS (1 << 20)
typedef struct {
  uint8_t text[RCDM_TOK_MAX_ADDED_LEN];
  int32_t len, id, special, reserved;
} rcdm_tok_added;
typedef struct {
  uint32_t a, b, rank, merged;     /* (a, b) -> merged at `rank` */
} rcdm_tok_pair;
typedef struct {
  int64_t ld;                      /* elements between rows of input_ids and attention_mask, >= max_length */
  int64_t text_bytes;
  int32_t n, max_length, truncation;
  int32_t bos_id, eos_id, pad_id;
  int32_t n_added;
  uint32_t pair_slots;
} rcdm_tokenize_desc;
uint32_t rcdm_tok_pair_hash(uint32_t a, uint32_t b);
size_t rcdm_clip_tokenize_workspace_bytes(const rcdm_tokenize_desc* d);
int rcdm_clip_tokenize(const rcdm_tokenize_desc* d, const void* text, const int32_t* offsets, const int32_t* byte_ids,
                       const rcdm_tok_added* added, const rcdm_tok_pair* pairs, int64_t* input_ids, int64_t* attention_mask,
                       int32_t* lengths, int32_t* pool_index, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * General conv2d, pools, bilinear frames: what an Inception-v3 forward (torchvision.models.inception_v3, pytorch-fid's
 * FIDInceptionA/C/E_1/E_2) needs beyond the kernels above; rcdms_amd/inception.py is the caller.  Activations are the f16
 * pixel rows [n * h * w][ld] of this header, so a block's torch.cat(branches, 1) is a column window per branch of one wider
 * buffer (out = buffer + column offset, ldc = the buffer's row stride).  Output sides, conv and pools alike:
 *   h_out = (h_in + 2 pad_h - kh) / stride_h + 1 (floor), likewise w_out; below 1 is RCDM_ESHAPE.
 * Every check is made before anything is launched: null pointers, sizes <= 0, ld below the channel count, a pointer that is
 * not 16-byte aligned give RCDM_EINVAL, a shape limit RCDM_ESHAPE.  No atomics: equal inputs give equal bits.  Row and
 * byte offsets are 64-bit (n_img * h_out * w_out itself must stay below 2^31 - 64).
 *
 * rcdm_conv2d: out[m][o] = epi( sum_{ky,kx,c} in[img, oy stride_h - pad_h + ky, ox stride_w - pad_w + kx][c] * W[o][(ky kw + kx) c_in + c] ),
 *   m = (img, oy, ox); taps outside the image are zeros.  W f16 [c_out][kh * kw * c_in] = torch weight.permute(0, 2, 3, 1),
 *   the convention of rcdm_conv3x3.  fp32 accumulation on v_mfma_f32_16x16x32_f16 (64 x 64 output tile per 4-wave block, k in
 *   steps of 32 in ascending order), epilogue in fp32, one rounding to f16.  epilogue: RCDM_EPI_BIAS (fp32 [c_out]) and / or
 *   RCDM_EPI_RELU; any other bit is RCDM_ESHAPE.  Limits (RCDM_ESHAPE): c_in % 8 == 0 (a 16-byte operand chunk never
 *   straddles a tap: a 3-channel image is padded to 8 with zeros), c_out % 8 == 0, lda % 8 == 0, ldc % 8 == 0, kh, kw <= 7,
 *   pad < kernel per axis, strides 1 or 2, sides <= 8192.
 * rcdm_pool2d: window <= 3 x 3, strides 1 or 2, 2 pad <= window per axis (so no window is all padding), c % 8 == 0,
 *   ld_in % 8 == 0, ld_out % 8 == 0.  Taps are visited ky-major then kx; padding is skipped, never read.
 *     RCDM_POOL_MAX               the largest in-image tap (exact; a NaN in the window is the result)
 *     RCDM_POOL_AVG_INCLUDE_PAD   fp32 sum of the in-image taps in that order / (kh kw), fp32 division, rounded once
 *     RCDM_POOL_AVG_EXCLUDE_PAD   the same sum / the number of in-image taps
 * rcdm_global_avgpool: out_f32[img][ch] = (((0 + x[0][ch]) + x[1][ch]) + ... + x[rows_per_img - 1][ch]) / rows_per_img over
 *   the rows of image img (in + img * rows_per_img * ld): ONE fp32 accumulator per channel, the rows added in ascending
 *   order, one fp32 division by (float)rows_per_img at the end.  c % 8 == 0, ld % 8 == 0, ldo % 4 == 0.
 * rcdm_image_bilinear_rows: n uint8 HWC frames (channels == 3; src_pitch / src_stride bytes between rows / frames, as
 *   rcdm_resample_desc) -> f16 rows [n * out_h * out_w][ld]: channel ch of the output is channel (flip_channels ? 2 - ch : ch)
 *   of torch.nn.functional.interpolate(x / 255, (out_h, out_w), mode="bilinear", align_corners=False) (no antialias: the FID
 *   definition of pytorch-fid, not Pillow's resampler) times scale[ch] plus shift[ch] (two roundings), rounded to f16; channels
 *   3 .. c_pad are zeros (c_pad % 8 == 0, 8 <= c_pad <= ld, ld % 8 == 0).  All fp32, per axis
 *     s = max(fma((float)in / out, o + 0.5, -0.5), 0)  (one rounding, as torch's CPU build evaluates it; nothing else is contracted),
 *     i0 = min((int)s, in - 1), i1 = min(i0 + 1, in - 1), l1 = s - i0, l0 = 1 - l1
 *   value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11) with v = u8 / 255 (a division).  Equal sizes give
 *   l1 = 0 on both axes, so the result is exactly f16((u8 / 255) * scale + shift).  Sides <= 8192 (RCDM_ESHAPE).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n_img, h_in, w_in;
  int32_t c_in, c_out;
  int32_t kh, kw, stride_h, stride_w, pad_h, pad_w;
  int32_t lda, ldc;               /* row strides of in / out in elements */
  int32_t epilogue;               /* RCDM_EPI_BIAS | RCDM_EPI_RELU */
} rcdm_conv2d_desc;
int rcdm_conv2d(const rcdm_conv2d_desc* d, const void* in, const void* W, const float* bias, void* out, void* stream);

#define RCDM_POOL_MAX 0
#define RCDM_POOL_AVG_INCLUDE_PAD 1
#define RCDM_POOL_AVG_EXCLUDE_PAD 2
typedef struct {
  int32_t n_img, h_in, w_in, c;
  int32_t kh, kw, stride_h, stride_w, pad_h, pad_w;
  int32_t ld_in, ld_out;
  int32_t mode;                   /* RCDM_POOL_* */
} rcdm_pool2d_desc;
int rcdm_pool2d(const rcdm_pool2d_desc* d, const void* in, void* out, void* stream);
int rcdm_global_avgpool(int32_t n_img, int32_t rows_per_img, int32_t c, const void* in, int64_t ld, float* out_f32, int64_t ldo,
                        void* stream);

typedef struct {
  int64_t src_pitch, src_stride;   /* bytes between source rows / source frames */
  int32_t n, channels;             /* channels == 3 */
  int32_t in_h, in_w, out_h, out_w;
  int32_t flip_channels;
  int32_t ld, c_pad;
  float scale[3], shift[3];        /* per OUTPUT channel */
} rcdm_bilinear_desc;
int rcdm_image_bilinear_rows(const rcdm_bilinear_desc* d, const void* src_u8, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS: the learned perceptual distance of Zhang et al. (The Unreasonable Effectiveness of Deep Features as a Perceptual
 * Metric, 2018), v0.1, over a VGG-16 or AlexNet tower built from rcdm_conv2d / rcdm_pool2d; rcdms_amd/lpips.py is the caller.
 * csrc/lpips_core.h holds the head's arithmetic and its summation orders, shared with tools/lpips_host.cpp; restated from the
 * paper and the lpips package's published forward, not pinned against the package.  Checks as for the conv2d block: every one
 * before anything is launched, RCDM_EINVAL for a null or misaligned pointer, a size <= 0 or an ld below the channel count,
 * RCDM_ESHAPE for a shape limit.  Row and byte offsets are 64-bit.
 *
 * rcdm_lpips_head: one tap of `pairs` frame pairs.  a and b are f16 pixel rows [pairs * h * w][lda | ldb] of c channels,
 *   post-ReLU; they may be the two halves of one buffer of 2 pairs frames (b = a + pairs h w lda).  lin: fp32 [c], >= 0.
 *   Per pixel, in fp32 on the widened f16 values:  na = sqrt(sum_c a_c^2) + 1e-10 (epsilon after the root), nb likewise,
 *   v = sum_c lin_c (a_c / na - b_c / nb)^2 with true divisions; an all-zero pixel gives 0 / 1e-10 = 0, finite.
 *   out[p] = (sum over the h w pixels of pair p of v) / (h w) in float64: the pixel values of a tile of 64 pixels go through
 *   a binary tree in float64, the tile partials of a pair through the fixed sum of frechet_core.h, one float64 division
 *   (lpips_core.h has the orders).  Two launches (tile partials into the workspace, then one workgroup per pair); no atomics,
 *   no memset: the same input gives the same bits for every grid size.  blocks: the grid of the first launch, 0 = the
 *   library's choice (for tests of that property).  Every feature row is read once; nothing but the tile partials is written.
 *   Limits (RCDM_ESHAPE): c % 8 == 0, c <= 512, lda % 8 == 0, ldb % 8 == 0, pairs <= 65535, sides <= 8192; a, b, lin and the
 *   workspace 16-byte aligned, out 8-byte aligned.  workspace: rcdm_lpips_head_workspace_bytes (0 for a bad descriptor);
 *   smaller is RCDM_EWORKSPACE.
 * rcdm_lpips_input_rows: n uint8 HWC frames (3 channels; src_pitch / src_stride bytes between rows / frames, as
 *   rcdm_bilinear_desc) -> the towers' f16 input rows with the scaling layer applied:
 *     value = f16(fma(u8 / 255, mul[ch], add[ch]))   — a division, ONE fused multiply-add (one rounding to fp32), one rounding
 *   to f16 (not the two-rounding form of rcdm_image_bilinear_rows); with mul = 2 / scale and add = (-1 - shift) / scale this is
 *   (2 u8 / 255 - 1 - shift) / scale of LPIPS's ScalingLayer.
 *     space_to_depth == 1   rows [n * in_h * in_w][ld]: channels 0 .. 2 the pixel, 3 .. 7 zeros (rcdm_conv2d's padded image)
 *     space_to_depth == 4   AlexNet's Conv2d(3, 64, 11, stride=4, padding=2) as a 3 x 3 stride-1 pad-0 rcdm_conv2d: rows
 *                           [n * (h_out + 2) * (w_out + 2)][ld] of 48 channels, h_out = (in_h - 7) / 4 + 1 (sides >= 7),
 *                           Q[n][Y][X][(dy 4 + dx) 3 + ch] = x[n][4 Y + dy - 2][4 X + dx - 2][ch], 0 outside the image (torch
 *                           pads the scaled tensor with zeros); the weights are W'[o][(KY 3 + KX) 48 + (dy 4 + dx) 3 + ch] =
 *                           W[o][ch][4 KY + dy][4 KX + dx], zeros for the twelfth row and column.  Exact, K = 432 against 363.
 *   Columns at and above 8 (48) of a wider row are left alone.  ld % 8 == 0, dst 16-byte aligned.
 *   rcdm_lpips_input_sides: the output sides and channel count of a descriptor (the same checks).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t lda, ldb;                /* row strides of a / b in elements */
  int32_t pairs, h, w, c;
  int32_t blocks;                  /* grid of the first launch; 0: the library's choice */
  int32_t reserved;
} rcdm_lpips_head_desc;
size_t rcdm_lpips_head_workspace_bytes(const rcdm_lpips_head_desc* d);
int rcdm_lpips_head(const rcdm_lpips_head_desc* d, const void* a, const void* b, const float* lin, double* out, void* workspace,
                    size_t workspace_bytes, void* stream);

typedef struct {
  int64_t src_pitch, src_stride;   /* bytes between source rows / source frames */
  int32_t n, in_h, in_w;
  int32_t space_to_depth;          /* 1 or 4 */
  int32_t ld;
  float mul[3], add[3];            /* per channel */
} rcdm_lpips_input_desc;
int rcdm_lpips_input_sides(const rcdm_lpips_input_desc* d, int32_t* out_h, int32_t* out_w, int32_t* channels);
int rcdm_lpips_input_rows(const rcdm_lpips_input_desc* d, const void* src_u8, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * hipGraph plumbing: capture the ~10^3 launches of one denoising step once, replay per step.
 * ---------------------------------------------------------------------------------------------- */
int rcdm_graph_begin_capture(void* stream);
int rcdm_graph_end_capture(void* stream, void** graph_exec_out);
int rcdm_graph_launch(void* graph_exec, void* stream);
int rcdm_graph_destroy(void* graph_exec);

/* HIP-event timing on an explicit stream (bench.py roofline leg) */
int rcdm_event_create(void** ev_out);
int rcdm_event_record(void* ev, void* stream);
int rcdm_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out); /* synchronises on stop */
int rcdm_event_destroy(void* ev);
int rcdm_stream_synchronize(void* stream);

/* ------------------------------------------------------------------------------------------------
 * Thin RCCL layer (librccl is dlopen'ed on first use; a single-GPU process never maps it).  The reference has no
 * inter-GPU communication at all: stage2_batchtest_rcdms_model.py:457-468 spawns one process per device and every
 * process loads every checkpoint.  These serve the packed-weight broadcast and the CFG-split latency mode (two GPUs
 * per story, one classifier-free-guidance half each, RCDMs_pipeline.py:482-497: the halves' noise predictions are
 * all-gathered inside the step graph).  Byte-typed, in place on the caller's HIP stream, graph-capturable.
 *   rcdm_comm_unique_id: rank 0 of a group fills 128 bytes, the caller ships them to the other ranks out of band
 *                        (file, socket, torch.distributed object broadcast);
 *   rcdm_comm_create:    collective over the group's ranks (blocks until all have called it); the communicator is bound
 *                        to the HIP device that is current at this call, and later calls from a thread whose current
 *                        device differs are refused with RCDM_EINVAL;
 *   rcdm_bcast:          `bytes` at `buf` from rank `root` (0 <= root < nranks, else RCDM_EINVAL) to every rank's `buf`;
 *   rcdm_allgather:      recv[r * bytes_per_rank ...] on every rank = rank r's send (send may alias its own slot).
 * ---------------------------------------------------------------------------------------------- */
int rcdm_comm_unique_id(void* id128);
int rcdm_comm_create(const void* id128, int32_t nranks, int32_t rank, void** comm_out);
int rcdm_comm_destroy(void* comm);
int rcdm_bcast(void* comm, void* buf, size_t bytes, int32_t root, void* stream);
int rcdm_allgather(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int rcdm_comm_last_error(void); /* last non-zero ncclResult_t seen on this thread */

#ifdef __cplusplus
}
#endif
#endif /* RCDM_H */
