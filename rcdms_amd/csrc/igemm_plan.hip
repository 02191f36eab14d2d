// igemm_plan.hip — host-side planner of the implicit-GEMM launches (igemm_plan.h): the tile-variant heuristics, the per-shape
// rule table, split-K planning and the process-wide switches behind them.  No kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "igemm_plan.h"
#include "gn_plan.h"

// the ping-pong tile shapes (igemm8.hip): rows kVarPP .. of the variant table
const PPShape kPPShapes[kNumPPShapes] = {{kVariants[kVarPP].bm, kVariants[kVarPP].bn},
                                         {kVariants[kVarPP + 1].bm, kVariants[kVarPP + 1].bn},
                                         {kVariants[kVarPP256].bm, kVariants[kVarPP256].bn}};

namespace {

// the variant (igemm_plan.h) forced by rcdm_set_igemm_variant(0 .. 10) or RCDM_IGEMM=dma128 | dma256 | dma64; 0 runs as 1
constexpr int kForceFromEnv = -2, kHeuristic = -1;
int g_force_variant = kForceFromEnv;
int forced_variant() {
  if (g_force_variant == kForceFromEnv) {
    const char* e = getenv("RCDM_IGEMM");
    g_force_variant = kHeuristic;
    if (e && !strcmp(e, "dma128")) g_force_variant = kVar128;
    if (e && !strcmp(e, "dma256")) g_force_variant = kVar256;
    if (e && !strcmp(e, "dma64")) g_force_variant = kVar64;
  }
  return g_force_variant;
}
int g_pp_mode = -1;  // RCDM_PP=0: never pick the ping-pong kernel (A/B switch)
// f16 split-K slabs on the 160x160 and the LDS-DMA kernels (IgemmArgs::slab16): -1 = not set (environment RCDM_SLAB16, default below)
int g_slab16 = -1;

// Split-K for the ping-pong kernel: its tiles are big, so shapes with fewer tiles than CUs (M = 10240 / 2560 rows with
// N = 640 / 1280) are cut along K until one round of the chip is full; a slice keeps >= 16 k-steps.
// taps of a launch: 1 (GEMM), 9 (conv3x3), 4 (phase form); the W row holds taps * Cin columns (+ Cin2 of a second input)
inline int taps_of(const IgemmArgs& a) { return (a.Ktot - a.Cin2) / a.Cin; }

int pp_splits(int tiles, int nk) {
  int s = rcdm_num_cus() / (tiles > 0 ? tiles : 1);
  if (s > nk / 16) s = nk / 16;
  if (s > 8) s = 8;
  return s < 1 ? 1 : s;
}

// The ping-pong kernel (igemm8.hip).  Measured against the 128x128 / 256x256 one-barrier kernels (tools/kbench.py,
// profiles/r2_pp_kbench.txt): it wins where its big tile comes out as whole rounds of the chip AND the k-loop is long
// enough to amortise a prologue / epilogue that nothing overlaps (one block per CU): the conv3x3 of the 64x64 level
// (160x320: exactly 256 tiles, 1.37-1.42x), the other convs with >= 2560 rows (1.04-1.07x), and the M = 40960 GEMMs
// with N <= 960 (qkv 1.13x, feed-forward out 1.12x).  The K = 640 / 1280 GEMMs of the 32x32 / 16x16 levels stay on the
// two-blocks-per-CU kernel, whose second block hides the epilogue.  Returns the shape index or -1.
int pick_pp(const IgemmArgs& a) {
  const int taps = taps_of(a);
  const int nk = (a.Cin + BK - 1) / BK * taps;
  if (a.M < 2048 || a.N < 256) return -1;
  if (taps == 1) {
    if (a.M < 20480 || a.N > 1024) return -1;
    // (nk 10 / 15: the 1x1 shortcut convs of the 64x64 level, tools/autotune.py + same-box A/B in the graph)
    if (!(nk >= 10 || (a.N >= 640 && nk >= 5))) return -1;
  } else if (nk < 40) {
    return -1;
  }
  const int cus = rcdm_num_cus();
  int best = -1;
  float best_score = 0.80f;
  for (int sh = 0; sh < kNumPPShapes; ++sh) {
    const int bm = kPPShapes[sh].bm, bn = kPPShapes[sh].bn;
    const int tm = (a.M + bm - 1) / bm, tn = (a.N + bn - 1) / bn, tiles = tm * tn;
    const int sp = tiles < cus ? pp_splits(tiles, nk) : 1;
    const int work = tiles * sp, rounds = (work + cus - 1) / cus;
    const float useful = (float)a.M * (float)a.N / ((float)tiles * bm * bn);
    const float fill = (float)work / (float)(rounds * cus);
    float score = useful * fill * (sp > 1 ? 0.90f : 1.0f);
    if (sh == 2) score *= 1.03f;  // 256x256 moves fewer operand bytes per flop
    if (score > best_score) {
      best_score = score;
      best = sh;
    }
  }
  return best;
}

// The 160x160 two-blocks-per-CU kernel (igemm16.hip), measured against every other variant (tools/kbench.py,
// profiles/r2_kbench.txt): it wins on the wide-N GEMMs with K <= 1280 and >= 2560 rows — fused [q;k;v] and GEGLU
// projections of the 64x64 / 32x32 / 16x16 levels: 7-15 % (no padded columns at N = 960 / 1920, 20 % fewer operand bytes
// per flop than 128x128, and unlike the ping-pong kernel its epilogue hides under the CU's other block) — and on the convs
// of the 32x32 level (3 % over the ping-pong kernel, which needs split-K there).  N = C GEMMs (HBM-bound or too few
// tiles), K >= 2560 (split-K shapes) and the 8x8 level stay where they were.
bool pick_16(const IgemmArgs& a, PlanFlags f) {
  static const int mode = rcdm_env_int("RCDM_I16", 1);  // RCDM_I16=0: never (A/B switch)
  if (!mode) return false;
  const int taps = taps_of(a);
  if (taps == 1) {
    // plain projections (no epilogue work: the staged halfs are copied out) that split into whole rounds of 160x160 tiles:
    // the cross-attention queries of the 32x32 level and of the shared-prefix half batch (tools/autotune.py: 17.3 -> 13.8 us)
    const bool plain = a.epi == 0 || (f.consumer && !(a.epi & (RCDM_EPI_RESIDUAL | RCDM_EPI_GELU | RCDM_EPI_GEGLU)));
    if (plain && a.out_scale == 1.0f && a.M % 160 == 0 && a.N % 160 == 0 && (a.M / 160) * (a.N / 160) >= 256 &&
        a.Cin <= 640 && a.N <= 640)
      return true;
    return a.N >= 960 && a.N >= 3 * a.Cin && a.M >= 2048 && a.Cin <= 1280;  // wide N only: qkv (3C), GEGLU (8C)
  }
  return a.M >= 5120 && a.M < 20480 && a.N >= 640 && a.N <= 1280;
}

// Per-shape overrides of the heuristics below: {taps, M, N, C_in} -> tile variant (1 .. 10) and split-K factor (0 = that
// variant's own heuristic).  kShapeRules holds what tools/autotune.py found AND a same-box A/B of the whole step
// confirmed; RCDM_SHAPE_RULES="taps,M,N,Cin,variant,split;..." adds rules at run time (first match wins: the environment's
// rules are looked at first), RCDM_SHAPE_RULES=off ignores the table — for tuning another chip or another model without
// a rebuild.  A rule is skipped where its variant cannot run the launch (row statistics: variants 1 .. 5; deferred-
// LayerNorm consumers: not the ping-pong kernel).
struct ShapeRule { int taps, M, N, Cin, variant, split; };
const ShapeRule kShapeRules[] = {
    // the headline workload (b = 2 x 5 frames, 64x64 latents), round 4: profiles/r4_autotune.txt, profiles/r4_shape_rules_ab.txt
    {9, 40960, 320, 320, kVar160, 1},   // the convs of the 64x64 level on 160x160 tiles, two blocks per CU, instead of the
    {9, 40960, 320, 640, kVar160, 1},   //   160x320 ping-pong tile (-3 % back to back, -0.15 ms per step together in the graph)
    {9, 40960, 320, 960, kVar160, 1},
    {9, 20480, 320, 320, kVar160, 0},   // ... and of the shared-prefix half batch
    {1, 2560, 1280, 1280, 10, 0},      // the N = C projections of the 16x16 level (to_out, proj_in, to_q) on the three-slot 128x64 ring: -0.09 ms
    {1, 640, 1280, 2560, 3, 3},        // 1x1 shortcuts of the 8x8 up blocks: 64x64 tiles split 3 ways
    // tools/tune_rules.py (every shape timed inside the step's launch sequence), then tools/ab_rules.sh: -0.07 ms together
    {1, 2560, 1280, 6400, kVar160, 0},  // proj_out-composed feed-forward GEMMs (K = 5C): 16x16 level on 160x160 tiles,
    {1, 10240, 640, 3200, 1, 0},       //   32x32 level on 128x128, 8x8 level on the three-slot 128x64 ring
    {1, 640, 1280, 6400, 10, 0},
    {1, 2560, 1280, 2560, 10, 0},      // 1x1 shortcuts / downsample-level projections of the 16x16 level: three-slot 128x64 ring
    {1, 2560, 1280, 1920, 10, 0},
    {1, 2560, 1280, 640, 10, 0},
    {1, 40960, 320, 640, kVar160, 0},   // 1x1 shortcuts of the 64x64 up blocks on 160x160 tiles
    {1, 40960, 320, 960, kVar160, 0},
    // the shapes only BASELINE config 1's plan has (b = 2 x 5 frames, 32x32 latents): tools/tune_rules.py --latent 32, confirmed
    // together in the graph (183.1 -> 173.9 ms per 20-step story; profiles/r4_shape_rules_ab.txt)
    {1, 2560, 640, 3200, 4, 0}, {1, 10240, 320, 1600, 10, 0}, {1, 2560, 640, 640, 4, 0}, {9, 160, 1280, 1280, 5, 0},
    {1, 160, 1280, 6400, 10, 0}, {1, 160, 10240, 1280, 4, 0}, {9, 10240, 320, 640, kVar160, 0},
    {1, 160, 1280, 2560, 10, 4}, {9, 10240, 320, 960, kVar160, 4}, {9, 2560, 640, 1920, kVar160, 0},
    {1, 10240, 320, 320, 10, 0}, {9, 2560, 640, 1280, kVar160, 0}, {9, 2560, 640, 960, kVar160, 8},
    {9, 5120, 320, 320, 1, 4}, {9, 640, 1280, 640, 1, 8}, {9, 2560, 640, 320, 1, 4}, {9, 640, 640, 640, 1, 8},
    {9, 2560, 320, 320, kVar160, 8}, {1, 2560, 640, 1920, 4, 0}, {1, 640, 1280, 1920, 10, 4},
    {9, 10240, 8, 320, kVar160, 8}, {1, 10240, 320, 960, 10, 0}, {1, 2560, 640, 1280, 4, 0}, {9, 5120, 320, 64, 5, 0},
    {1, 2560, 640, 960, 4, 0}, {1, 5120, 320, 320, 4, 0}, {1, 640, 1280, 640, 4, 0}, {1, 2560, 640, 320, 4, 0},
    // the shapes only BASELINE config 3's plan has (4 stories = b 8, 64x64 latents, L = 91): --stories 4 --ctx-len 91, confirmed
    // together (2741 -> 2683 ms per story batch): at this batch the 160x160 two-blocks-per-CU kernel beats the ping-pong tiles on
    // every conv of the 64x64 / 32x32 levels in the step's own sequence, not back to back
    {1, 40960, 5120, 640, 2, 0}, {1, 10240, 1280, 6400, kVar160, 1}, {9, 40960, 640, 640, kVar160, 0},
    {9, 163840, 320, 640, kVar160, 1}, {9, 163840, 320, 960, kVar160, 0}, {9, 40960, 640, 1920, kVar160, 1},
    {9, 40960, 640, 1280, kVar160, 1}, {9, 40960, 640, 960, kVar160, 0}, {1, 10240, 1280, 1280, kVar160, 1},
    {9, 40960, 640, 320, kVar160, 1}, {1, 10240, 1280, 2560, kVar160, 1}, {1, 40960, 640, 1920, kVar160, 0},
    {1, 40960, 640, 1280, kVar160, 1}, {9, 81920, 320, 64, kVar160, 1}, {1, 10240, 1280, 1920, kVar160, 0},
    {1, 40960, 640, 320, 5, 1}, {1, 81920, 320, 320, 5, 1}, {1, 10240, 1280, 640, kVar160, 0},
    // BASELINE config 5 (stage-1 prior, 970 token rows): tools/tune_rules.py --prior, confirmed with tools/bench_prior.py (1.83 -> 1.92 stories/s)
    {1, 970, 2048, 2048, 4, 0}, {1, 970, 6144, 2048, 5, 1}, {1, 10, 1280, 2048, 10, 4},
    {0, 0, 0, 0, 0, 0},   // (terminator)
};
constexpr int kMaxEnvRules = 128;
ShapeRule g_env_rules[kMaxEnvRules];
int g_n_env = -1;            // -1: RCDM_SHAPE_RULES not parsed yet
bool g_rule_table_on = true;
char g_rules_text[8192] = "";
bool g_rules_from_api = false;
const ShapeRule* find_shape_rule(const IgemmArgs& a, PlanFlags f) {
  ShapeRule* env_rules = g_env_rules;
  int& n_env = g_n_env;
  bool& table_on = g_rule_table_on;
  if (n_env < 0) {
    int n = 0;
    const char* e = g_rules_from_api ? g_rules_text : getenv("RCDM_SHAPE_RULES");
    table_on = true;
    if (e && !strcmp(e, "off")) {
      table_on = false;
    } else if (e) {
      while (*e && n < kMaxEnvRules) {
        ShapeRule r{};
        int used = 0;
        if (sscanf(e, "%d,%d,%d,%d,%d,%d%n", &r.taps, &r.M, &r.N, &r.Cin, &r.variant, &r.split, &used) == 6 && r.variant >= 1 &&
            r.variant < kNumVariants && r.split >= 0)
          env_rules[n++] = r;
        e += used;
        while (*e && *e != ';') ++e;
        if (*e == ';') ++e;
        if (!used) break;
      }
    }
    n_env = n;
  }
  if (a.ph_rows) return nullptr;
  const int taps = taps_of(a);
  auto fits = [&](const ShapeRule& r) {
    if (r.taps != taps || r.M != a.M || r.N != a.N || r.Cin != a.Cin) return false;
    if (f.producer && !is_dma(r.variant)) return false;
    if (f.consumer && is_pp(r.variant)) return false;
    if ((f.producer || f.consumer) && r.split > 1) return false;
    return true;
  };
  for (int i = 0; i < n_env; ++i)
    if (fits(env_rules[i])) return &env_rules[i];
  if (table_on)
    for (const ShapeRule* r = kShapeRules; r->variant; ++r)
      if (fits(*r)) return r;
  return nullptr;
}

// rule_split: the split-K factor of the shape rule that chose the variant (0: no rule, or the rule leaves it to the heuristic)
int pick_variant(const IgemmArgs& a, PlanFlags f, int& rule_split) {
  rule_split = 0;
  const int forced = forced_variant();
  if (forced != kHeuristic) return forced == 0 ? kVar128 : forced;
  if (const ShapeRule* r = find_shape_rule(a, f)) {
    rule_split = r->split;
    return r->variant;
  }
  if (g_pp_mode < 0) g_pp_mode = rcdm_env_int("RCDM_PP", 1);
  if (g_pp_mode && !f.producer) {   // row statistics come out of the igemm_dma epilogue only
    if (pick_16(a, f)) return kVar160;
    const int pp = pick_pp(a);
    if (pp >= 0) return kVarPP + pp;
  }
  // measured (tools/kbench.py, MI355X).  128x128 with two blocks per CU is the default.  Shapes that leave most CUs
  // without a 128x128 tile (8x8 / 16x16 levels, context K/V projections) run as 64x64 or 128x64 tiles so that several
  // blocks per CU keep more DMA in flight; N = 320 / 960 (half a 128-wide tile wasted) with a short K take 128x64;
  // the deep-K convs of the 32x32 / 16x16 levels take 256x256.
  const int nk = (a.Cin + BK - 1) / BK * taps_of(a) + (a.Cin2 + BK - 1) / BK;
  if (a.Ktot != a.Cin) {
    if (a.N <= 64) return kVar128x64;  // conv_out (4 -> 8 channels): half the weight tile of 128x128 is padding (51 -> 28 us)
    return kVar128;   // (the 256x256 LDS-DMA tile's conv instantiation spills 48 B: only when forced; the ping-pong 256x256 tile covers its shapes)
  }
  const int t128 = ((a.M + 127) / 128) * ((a.N + 127) / 128);
  if (t128 <= 64 && nk <= 24) return kVar64Deep;  // (the two-slot 64x64 ring is 8-10 % faster back to back, tools/autotune.py, but +0.1 ms per step in the graph)
  if (nk >= 20 && nk < 40 && a.N >= 512 && a.M >= 512) {
    // 256x256 (staggered 8-wave loop, ~8 % faster per flop) when its last round of tiles is not emptier than 128x128's
    const int cus = rcdm_num_cus();
    const int t256 = ((a.M + 255) / 256) * ((a.N + 255) / 256);
    const float e1 = (float)t128 / (float)(((t128 + 2 * cus - 1) / (2 * cus)) * 2 * cus);
    const float e2 = (float)t256 / (float)(((t256 + cus - 1) / cus) * cus);
    if (1.08f * e2 > e1 + 0.01f) return kVar256;
  }
  if (nk >= 40) return kVar128;  // deep K: split-K over 128x128 tiles fills the chip
  if (t128 <= 160) return kVar64;
  if (t128 <= 256) return kVar128x64;
  if ((a.N % 128) == 64 && nk <= 10) return kVar128x64;
  return kVar128;
}

// Split-K only pays when (a) all tiles x splits still run as ONE round of resident blocks (a second, partly filled
// round costs more than the idle CUs it fills) and (b) every slice keeps >= ~20 k-steps, because the fp32 slabs and
// the reduce pass are not free (measured with tools/splitk_test.py: e.g. M=2560 N=1280 K=1280 is 21 us unsplit and
// 33 us split 3 ways; the 8x8-level convs (50 tiles, 180 k-steps) drop from 150 us to 40 us split 8 ways).
int plan_splits(int tiles, int slots, int nk, int requested) {
  if (requested == 1) return 1;
  if (requested > 1) return requested < nk ? requested : nk;
  int s = slots / (tiles > 0 ? tiles : 1);
  if (s > nk / 20) s = nk / 20;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  return s;
}

// tiles and split-K of `a` (shape fields set): with the variant the switches, the rules and the heuristics choose, or with
// `use_variant` (>= 0)
void fill_common(IgemmArgs& a, int requested_split, PlanFlags f, int& variant, int use_variant = -1) {
  int rule_split = 0;
  variant = use_variant >= 0 ? use_variant : pick_variant(a, f, rule_split);
  // a launch the tile has no instantiation for (kVariants: the 256x256 LDS-DMA tile with statistics, a consumer or quick-GELU)
  const int needs = (f.producer ? kNoStats : 0) | (f.consumer ? kNoConsumer : 0) | ((a.epi & RCDM_EPI_QUICK_GELU) ? kNoQuickGelu : 0);
  if ((kVariants[variant].cannot & needs) && kVariants[variant].instead) variant = kVariants[variant].instead;
  const VariantRow& tc = kVariants[variant];
  a.tilesM = (a.M + tc.bm - 1) / tc.bm;
  a.tilesN = (a.N + tc.bn - 1) / tc.bn;
  a.kc = (a.Cin + BK - 1) / BK;
  const int taps = taps_of(a);
  a.nk = taps * a.kc;
  a.nk1 = kNoSeg2;
  if (a.Cin2 > 0) {          // second input: its k-steps follow the nine taps' (from_conv: Cin and Cin2 are multiples of BK)
    a.nk1 = a.nk;
    a.nk += a.Cin2 / BK;
  }
  int s;
  if (rule_split > 0 && requested_split <= 0) {
    s = rule_split;
  } else if (is_pp(variant) && requested_split <= 0) {
    const int tiles = a.tilesM * a.tilesN;
    s = tiles < rcdm_num_cus() ? pp_splits(tiles, a.nk) : 1;
  } else {
    s = plan_splits(a.tilesM * a.tilesN, rcdm_num_cus() * tc.blocks_per_cu, a.nk, requested_split);
  }
  if (s > a.nk) s = a.nk;
  a.nk_per_split = (a.nk + s - 1) / s;
  a.splits = (a.nk + a.nk_per_split - 1) / a.nk_per_split;
}

int from_conv(const rcdm_conv3x3_desc* d, IgemmArgs& a) {
  if (d->stride != 1 && d->stride != 2) return RCDM_ESHAPE;
  if (d->upsample != 0 && d->upsample != 1) return RCDM_ESHAPE;
  if (d->n_img <= 0 || d->h_in <= 0 || d->w_in <= 0) return RCDM_EINVAL;
  const int hv = d->h_in << d->upsample, wv = d->w_in << d->upsample;
  a.Ho = (hv - 1) / d->stride + 1;
  a.Wo = (wv - 1) / d->stride + 1;
  a.Hi = d->h_in; a.Wi = d->w_in; a.stride = d->stride; a.up = d->upsample;
  if (d->pad_after_only != 0 && d->pad_after_only != 1) return RCDM_ESHAPE;
  // F.pad(x, (0,1,0,1)) + a stride-2 conv without padding: (h + 1 - 3) / 2 + 1 = h / 2 rows for even h — the same
  // count as the symmetric form; odd sizes would differ, and the form only exists for stride 2
  if (d->pad_after_only && (d->stride != 2 || d->upsample || (d->h_in & 1) || (d->w_in & 1))) return RCDM_ESHAPE;
  a.pad = d->pad_after_only ? 0 : 1;
  a.M = d->n_img * a.Ho * a.Wo; a.N = d->c_out; a.Cin = d->c_in; a.Ktot = 9 * d->c_in;
  a.lda = d->lda; a.ldc = d->ldc; a.ldr = d->ldr; a.ldt = d->ldt;
  a.rows_per_sample = d->rows_per_sample; a.epi = d->epilogue; a.out_scale = d->out_scale;
  a.dup = (long long)d->dup_rows * d->ldc;
  if (d->c_in2 < 0) return RCDM_EINVAL;
  if (d->c_in2 > 0) {   // rcdm_conv3x3_add1x1: a 1x1 convolution of a second input in the same accumulators
    if (d->stride != 1 || d->upsample || d->pad_after_only) return RCDM_ESHAPE;
    if ((d->c_in % BK) || (d->c_in2 % BK) || (d->lda2 & 7) || d->lda2 < d->c_in2) return RCDM_ESHAPE;
    if ((size_t)a.M * (size_t)d->lda2 * 2 >= 0x7FFFFFFFull) return RCDM_ESHAPE;
    a.Cin2 = d->c_in2; a.lda2 = d->lda2; a.Ktot += d->c_in2;
  }
  return RCDM_OK;
}

// upsample = 2: the nearest-2x upsample + conv3x3 as four 2x2 phase convolutions over the source grid (igemm_args.h,
// IgemmArgs::ph_rows; weights in the rcdm.h phase layout).  4/9 of the flops of the upsample = 1 form.  Runs on the
// ping-pong kernel only, unsplit: returns the tile shape, or -1 when the shape does not fill the chip that way (the caller
// keeps the upsample = 1 form — at the 8x8 -> 16x16 level the plain form with split-K is faster).
int plan_up2(const rcdm_conv3x3_desc* d, IgemmArgs& a) {
  if (d->upsample != 2 || d->stride != 1 || d->pad_after_only || d->dup_rows) return -1;
  if (d->epilogue & ~RCDM_EPI_BIAS) return -1;
  if (d->n_img <= 0 || d->h_in <= 0 || d->w_in <= 0 || d->c_in <= 0 || d->c_out <= 0 || (d->c_in % BK)) return -1;
  const long long src = (long long)d->n_img * d->h_in * d->w_in;
  if (4 * src >= 0x7FFFFFFFll || 4ll * d->c_out * 4 * d->c_in * 2 >= 0x7FFFFFFFll) return -1;   // virtual rows are ints; weight offsets 32-bit
  a.Hi = a.Ho = d->h_in; a.Wi = a.Wo = d->w_in; a.stride = 1; a.up = 0; a.pad = 1;
  a.ph_rows = (int)src; a.M = 4 * a.ph_rows; a.N = d->c_out; a.Cin = d->c_in; a.Ktot = 4 * d->c_in;
  a.lda = d->lda; a.ldc = d->ldc; a.ldr = 0; a.ldt = 0; a.rows_per_sample = 1; a.epi = d->epilogue; a.out_scale = d->out_scale;
  a.dup = 0;
  const int cus = rcdm_num_cus();
  int best = -1;
  float best_score = 0.70f;
  const int fv = forced_variant();
  const int forced = (fv > 0 && is_pp(fv)) ? fv - kVarPP : -1;
  for (int sh = 0; sh < kNumPPShapes; ++sh) {
    const int bm = kPPShapes[sh].bm, bn = kPPShapes[sh].bn;
    if (a.ph_rows % bm) continue;
    const int tm = a.M / bm, tn = (a.N + bn - 1) / bn, tiles = tm * tn;
    if (forced >= 0) {   // rcdm_set_igemm_variant(6 | 7 | 8): that tile shape whatever the fill (tests)
      if (sh == forced) best = sh;
      continue;
    }
    const int sp = tiles < cus ? pp_splits(tiles, 4 * (a.Cin / BK)) : 1;   // few tiles (the 8x8 -> 16x16 upsampler): cut K like the plain form does
    const int work = tiles * sp, rounds = (work + cus - 1) / cus;
    const float score = ((float)a.N / (float)(tn * bn)) * ((float)work / (float)(rounds * cus)) * (sp > 1 ? 0.90f : 1.0f);
    if (score > best_score) {
      best_score = score;
      best = sh;
    }
  }
  if (best < 0) return -1;
  a.tilesM = a.M / kPPShapes[best].bm;
  a.tilesN = (a.N + kPPShapes[best].bn - 1) / kPPShapes[best].bn;
  a.kc = a.Cin / BK;
  a.nk = 4 * a.kc;
  int s = d->split_k > 0 ? d->split_k : (a.tilesM * a.tilesN < cus ? pp_splits(a.tilesM * a.tilesN, a.nk) : 1);
  if (s > a.nk) s = a.nk;
  a.nk_per_split = (a.nk + s - 1) / s;
  a.splits = (a.nk + a.nk_per_split - 1) / a.nk_per_split;
  return best;
}

}  // namespace

void from_gemm(const rcdm_gemm_desc* d, IgemmArgs& a) {
  a.M = d->M; a.N = d->N; a.Cin = d->K; a.Ktot = d->K;
  a.Hi = a.Wi = a.Ho = a.Wo = 1; a.stride = 1; a.up = 0; a.pad = 1;
  a.lda = d->lda; a.ldc = d->ldc; a.ldr = d->ldr; a.ldt = d->ldt;
  a.rows_per_sample = d->rows_per_sample; a.epi = d->epilogue; a.out_scale = d->out_scale;
  a.dup = (long long)d->dup_rows * d->ldc;
}

int slab16_mode() {
  if (g_slab16 < 0) g_slab16 = rcdm_env_int("RCDM_SLAB16", 1) != 0;   // (five same-box pairs: -0.11 ms per step, whole-UNet error unchanged)
  return g_slab16;
}

// statistics geometry of the norm behind a split-K launch (rcdm_*_gnstat): 0 when the pair qualifies — `a` planned (splits
// known), the norm reads exactly the rows this launch writes (same row count, width, row stride), takes the three-launch
// form, and the epilogue has no GEGLU / second row copy / phase rows.  With gn_ws: also points a.gn_partial into it.
int attach_gnstat(IgemmArgs& a, const rcdm_groupnorm_desc* gn, void* gn_ws, size_t gn_ws_bytes, bool need_ws) {
  if (!gn) return RCDM_EINVAL;
  if (a.epi & RCDM_EPI_QUICK_GELU) return RCDM_ESHAPE;   // (the encoders' activation: plain rcdm_gemm only)
  if (a.splits <= 1 || (a.epi & RCDM_EPI_GEGLU) || a.dup || a.ph_rows) return RCDM_ESHAPE;
  GnArgs g{};
  int rc = rcdm_gn_plan(gn, g);
  if (rc) return rc;
  if (!rcdm_gn_three_launch(g)) return RCDM_ESHAPE;
  if ((long long)g.samples * g.P != a.M || g.C != a.N || gn->ldx != a.ldc) return RCDM_ESHAPE;
  if (g.CH * g.RPB > 512 || (size_t)(g.CH * g.RPB + g.CH) * 16 * sizeof(float) > 64 * 1024) return RCDM_ESHAPE;   // (the kernel's launch bound; C <= 4096)
  const size_t need = ((size_t)g.samples * g.splits * g.G * 3 + (size_t)g.samples * g.G * 2) * sizeof(float);
  if (need_ws) {
    if (!gn_ws || gn_ws_bytes < need) return RCDM_EWORKSPACE;
    a.gn_partial = (float*)gn_ws;
  }
  a.gn_samples = g.samples; a.gn_P = g.P; a.gn_G = g.G; a.gn_cg = g.cg; a.gn_CH = g.CH; a.gn_RPB = g.RPB;
  a.gn_splits = g.splits; a.gn_rps = g.rows_per_split;
  return RCDM_OK;
}

// A statistics producer whose caller asks for another slot count than this shape's own tile choice gives (two producers
// that fill ONE statistics buffer — e.g. the same projection run on all rows and on a row subset — must agree on it): the
// LDS-DMA tile whose column-tile count is `parts` (64- or 128-wide tiles), -1 when there is none.
int variant_for_parts(const IgemmArgs& a, int parts) {
  const int n64 = (a.N + 63) / 64, n128 = (a.N + 127) / 128;
  if (parts == n128) return kVar128;
  if (parts == n64) return ((a.M + 127) / 128) * n64 < rcdm_num_cus() ? kVar64Deep : kVar128x64;
  return -1;
}

int check_common(const IgemmArgs& a) {
  if (!a.A || !a.W || !a.out) return RCDM_EINVAL;
  if (a.M <= 0 || a.N <= 0 || a.Cin <= 0) return RCDM_EINVAL;
  if ((a.Cin & 7) || (a.N & 7) || (a.lda & 7) || (a.ldc & 7)) return RCDM_ESHAPE;
  if (a.epi & ~(RCDM_EPI_BIAS | RCDM_EPI_ROWVEC | RCDM_EPI_RESIDUAL | RCDM_EPI_GEGLU | RCDM_EPI_GELU | RCDM_EPI_QUICK_GELU))
    return RCDM_ESHAPE;   // a bit these kernels do not know (RCDM_EPI_RELU is rcdm_conv2d's)
  if ((a.epi & RCDM_EPI_BIAS) && !a.bias) return RCDM_EINVAL;
  if ((a.epi & RCDM_EPI_ROWVEC) && (!a.rowvec || a.rows_per_sample <= 0 || (a.ldt & 3))) return RCDM_EINVAL;
  if ((a.epi & RCDM_EPI_RESIDUAL) && (!a.res || (a.ldr & 7))) return RCDM_EINVAL;
  if ((a.epi & RCDM_EPI_GEGLU) && (a.N % 32)) return RCDM_ESHAPE;
  if ((a.epi & RCDM_EPI_GEGLU) && (a.epi & RCDM_EPI_GELU)) return RCDM_EINVAL;
  if ((a.epi & RCDM_EPI_QUICK_GELU) && (a.epi & (RCDM_EPI_GELU | RCDM_EPI_GEGLU))) return RCDM_EINVAL;
  if (a.dup < 0) return RCDM_EINVAL;
  // buffer-load offsets are 32-bit with 0x80000000 reserved as "out of range"
  const size_t in_rows = (a.Ktot == a.Cin) ? (size_t)a.M : (size_t)(a.M / (a.Ho * a.Wo)) * a.Hi * a.Wi;
  if (in_rows * (size_t)a.lda * 2 >= 0x7FFFFFFFull || (size_t)a.N * a.Ktot * 2 >= 0x7FFFFFFFull) return RCDM_ESHAPE;
  return RCDM_OK;
}

int plan_gemm(const rcdm_gemm_desc* d, PlanFlags f, IgemmArgs& a, int& variant) {
  if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0) return RCDM_EINVAL;
  from_gemm(d, a);
  fill_common(a, d->split_k, f, variant);
  if (f.producer && f.parts > 0 && f.parts != a.tilesN) {   // the caller's slot count, where an LDS-DMA tile has it
    const int alt = variant_for_parts(a, f.parts);
    if (alt < 0) return RCDM_ESHAPE;
    fill_common(a, 1, f, variant, alt);                     // (a statistics launch is never split)
  }
  return RCDM_OK;
}

int plan_conv(const rcdm_conv3x3_desc* d, IgemmArgs& a, int& variant) {
  if (!d) return RCDM_EINVAL;
  if (d->upsample == 2) {
    const int shape = plan_up2(d, a);
    if (shape < 0) return RCDM_ESHAPE;
    variant = kVarPP + shape;
    return RCDM_OK;
  }
  const int rc = from_conv(d, a);
  if (rc) return rc;
  if (a.Cin <= 0 || a.N <= 0) return RCDM_EINVAL;
  fill_common(a, d->split_k, PlanFlags{}, variant);
  return RCDM_OK;
}

extern "C" {

int rcdm_set_igemm_variant(int32_t v) {
  if (v < -1 || v >= kNumVariants) return RCDM_EINVAL;
  g_force_variant = v < 0 ? kHeuristic : v;
  return RCDM_OK;
}

int rcdm_set_shape_rules(const char* rules) {
  if (rules && strlen(rules) >= sizeof(g_rules_text)) return RCDM_EINVAL;
  g_rules_from_api = rules != nullptr;
  if (rules) strcpy(g_rules_text, rules);
  g_n_env = -1;   // parsed again at the next launch
  return RCDM_OK;
}

int rcdm_set_splitk_slab_f16(int32_t on) {
  g_slab16 = on < 0 ? -1 : (on ? 1 : 0);
  return RCDM_OK;
}

int rcdm_set_igemm_pingpong(int32_t on) {
  g_pp_mode = on ? 1 : 0;
  return RCDM_OK;
}

}  // extern "C"
