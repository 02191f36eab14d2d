"""GroupNorm inputs whose groups lie far from zero, their float64 reference and the error budgets: shared by
tests/test_gn_cond_host.py (CPU: the inputs are fair to the reference's operation and discriminate against raw one-pass sums) and
tests/test_hip_gn_cond.py (GPU: the kernels stay inside the budgets).  Needs numpy only.

A one-pass statistic M2 = sum(x^2) - sum(x) mean in fp32 loses about (mean / std)^2 2^-24 (a few) of the variance; inputs drawn
as randn * 2 + 0.7 (mean / std = 0.35) never show it.  Here every (sample, group) has its own offset mu (both signs) and its own
sigma, the ratio |mu| / sigma being what a case fixes:

  control   mu / sigma = 0.35: the draw of the other GroupNorm tests
  r64, r128, r256   mu / sigma = 64, 128, 256 with |mu| log-uniform in [4, 1000].  Not beyond 256: f16 values near mu are
            |mu| 2^-11 .. |mu| 2^-10 apart, so at 256 a sigma is only 4 .. 8 representable steps.  The ratio is that of the
            float64 mean and std of the f16-ROUNDED values and is asserted here (RATIO_BAND).
  spread    every channel of a group at its own mean: channel means spread by 0.5 .. 4 sigma of the channel's own noise, the
            noise at |mu| / 64 (what a ResNet output + time-embedding row + residual looks like); a per-column pivot has to
            combine the columns correctly
  mixed     groups alternate control / r256 / constant inside one tensor: an error (or a fix) must not leak into neighbours
  constant  every value of a group is one f16 number c != 0 (variance exactly 0, rstd = eps^-1/2): CONSTANTS in the first
            groups, then +-[0.1, 1000) log-uniform with whatever mantissa the rounding leaves

All values are float32 arrays holding f16-representable numbers.

Budgets.  They come from the f16 OUTPUT, not from any kernel: y = (x - mean) rstd gamma + beta is stored as f16, relative
spacing 2^-10, half-ulp 2^-11 relative.
  RSTD_REL = 2^-14   |rstd / rstd64 - 1|: an eighth of an f16 half-ulp in every output of the group — the statistics never show
            in the stored halfs.
  MEAN_SIG = 2^-13   |mean - mean64| / std64: an error of 2^-13 in normalised units.  fp32's own representation of a mean at
            ratio 256 costs up to 256 * 2^-24 = 2^-16 of it, so the budget leaves room for 8 such roundings.
  output    |y - y64| <= 2^-10 |y64| + 2^-12 |gamma_c| (the absolute term x 1.1 with SiLU, |silu'| <= 1.1): twice the sum of
            the f16 rounding of y (2^-11 |y|), the rstd budget (2^-14 |y - beta|), the mean budget (2^-13 |gamma|) and the fp32
            rounding of x * scale + shift at ratio 256 (numbers of size 256 |gamma| rounded to 2^-24: 2^-16 |gamma| each).
  constant  mean within 2 fp32 ulps of c, rstd within 2^-14 (relative) of eps^-1/2; outputs only finite: the reference's own
            fp32 x * scale + shift form loses c * rstd * 2^-24 there (rstd = 316 .. 1000), which is not the statistics' error."""
import numpy as np

CASES = ("control", "r64", "r128", "r256", "spread", "mixed", "constant")
RATIO = {"r64": 64.0, "r128": 128.0, "r256": 256.0}
RATIO_BAND = (0.93, 1.07)             # measured ratio / intended ratio of the f16-rounded values
CONSTANTS = (3.3, -100.0, 0.1, 1000.0, -7.77, 48.5)
GROUPS = 32
EPS = (1e-5, 1e-6)                    # cross-frame, per-frame

RSTD_REL = 2.0 ** -14
MEAN_SIG = 2.0 ** -13
OUT_REL = 2.0 ** -10
OUT_ABS = 2.0 ** -12

# (samples, rows, C): the stand-alone statistics / norm shapes of the GPU test, by the form the library takes for them (the GPU
# test asserts the form through rcdm_groupnorm_prestat_ok).  The single-launch kernel needs samples * (groups / bundle) >= 48
# blocks: 2 x 1280 channels (one group per block) or 4 x 640 channels (two groups per block).
SINGLE_LAUNCH = [(2, 320, 1280), (4, 256, 640), (2, 315, 1280)]
THREE_LAUNCH = [(1, 1280, 320), (1, 1280, 1280), (1, 5120, 64), (1, 1283, 320),    # cg = 10 / 40 / 2; 1283: a short last split
                (1, 320, 1280), (2, 256, 640), (1, 315, 1280)]     # the single-launch shapes with too few samples for that form
FOLD_SHAPE = (4, 600, 320)            # >= 4 samples, three launches: the apply kernel that finalises by itself
SHAPES = SINGLE_LAUNCH + THREE_LAUNCH + [FOLD_SHAPE]


def f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float32)


def group_kinds(samples, groups, case):
    """[samples][groups] array of strings: what each (sample, group) of `case` holds."""
    k = np.empty((samples, groups), dtype=object)
    k[:] = case
    if case == "mixed":
        cyc = ("control", "r256", "constant")
        for s in range(samples):
            for g in range(groups):
                k[s, g] = cyc[(s + g) % 3]
    return k


def _group(g, kind, rows, cg, idx):
    """rows x cg float64 values of one (sample, group), before the f16 rounding."""
    sign = 1.0 if g.random() < 0.5 else -1.0
    if kind == "constant":
        c = CONSTANTS[idx] if idx < len(CONSTANTS) else sign * np.exp(g.uniform(np.log(0.1), np.log(1000.0)))
        return np.full((rows, cg), float(f16(c)))
    noise = g.standard_normal((rows, cg))
    chan = g.standard_normal(cg) if cg > 1 else np.zeros(1)
    if kind == "control":
        mu, sigma, spread = 0.7 * sign, 2.0, 0.3
    elif kind in RATIO:
        mu = sign * np.exp(g.uniform(np.log(4.0), np.log(1000.0)))
        sigma, spread = abs(mu) / RATIO[kind], 0.3
    elif kind == "spread":
        mu = sign * np.exp(g.uniform(np.log(4.0), np.log(100.0)))
        spread = g.uniform(0.5, 4.0)
        return mu + (abs(mu) / 64.0) * (noise + spread * chan[None, :])
    else:
        raise ValueError(kind)
    dev = noise + spread * chan[None, :]
    dev = (dev - dev.mean()) / dev.std()          # the group's deviations: mean 0, std 1 exactly (before rounding)
    return mu + sigma * dev


def make_input(samples, rows, C, groups, case, seed=0):
    """f16-rounded rows [samples * rows][C] (float32) of `case`; asserts what the case promises about the ROUNDED values."""
    assert case in CASES and C % groups == 0
    cg = C // groups
    g = np.random.default_rng([17, samples, rows, C, groups, CASES.index(case), seed])
    kinds = group_kinds(samples, groups, case)
    x = np.empty((samples, rows, groups, cg), dtype=np.float64)
    for s in range(samples):
        for gi in range(groups):
            x[s, :, gi, :] = _group(g, kinds[s, gi], rows, cg, s * groups + gi)
    x = f16(x)
    assert np.isfinite(x).all()
    mean, var = x.astype(np.float64).mean(axis=(1, 3)), x.astype(np.float64).var(axis=(1, 3))
    for kind in set(kinds.reshape(-1)):
        sel = kinds == kind
        if kind == "constant":
            assert (var[sel] == 0).all() and (mean[sel] != 0).all()
            continue
        ratio = np.abs(mean[sel]) / np.sqrt(var[sel])
        if kind in RATIO:
            lo, hi = RATIO_BAND[0] * RATIO[kind], RATIO_BAND[1] * RATIO[kind]
            assert (ratio >= lo).all() and (ratio <= hi).all(), (kind, ratio.min(), ratio.max())
            assert (np.abs(mean[sel]) >= 3.9).all() and (np.abs(mean[sel]) <= 1010).all()
        elif kind == "control":
            assert (ratio > 0.3).all() and (ratio < 0.4).all(), (ratio.min(), ratio.max())
        elif kind == "spread":
            assert (ratio > 8).all() and (ratio < 70).all(), (ratio.min(), ratio.max())     # 64 / sqrt(1 + spread^2), cg = 2 included
            cm, cs = x.astype(np.float64).mean(axis=1), x.astype(np.float64).std(axis=1)     # [samples][groups][cg]
            assert (np.abs(cm) / cs)[sel].min() > 40                                          # every COLUMN is far from zero
    if case != "constant" and case != "control":
        assert (mean > 0).any() and (mean < 0).any(), "offsets of one sign only"
    return x.reshape(samples * rows, C)


def reference(x, samples, rows, C, groups, eps, gamma=None, beta=None, silu=False):
    """float64 (mean, var, rstd) [samples][groups] (biased variance) and, with gamma / beta, y [samples * rows][C]."""
    cg = C // groups
    v = np.asarray(x, dtype=np.float64).reshape(samples, rows, groups, cg)
    mean = v.mean(axis=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = (var + eps) ** -0.5
    if gamma is None:
        return mean, var, rstd
    return mean, var, rstd, apply64(x, samples, rows, C, groups, mean, rstd, gamma, beta, silu)


def apply64(x, samples, rows, C, groups, mean, rstd, gamma, beta, silu=False):
    """float64 y = (x - mean) rstd gamma + beta (then SiLU) with the given statistics [samples][groups]."""
    v = np.asarray(x, dtype=np.float64).reshape(samples, rows, groups, C // groups)
    y = (v - np.asarray(mean, dtype=np.float64)[:, None, :, None]) * np.asarray(rstd, dtype=np.float64)[:, None, :, None]
    y = y.reshape(samples * rows, C) * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)
    if silu:
        y = y / (1.0 + np.exp(-y))
    return y


def _ulp32(c):
    c = np.abs(np.asarray(c, dtype=np.float32))
    return (np.nextafter(c, np.float32(np.inf)) - c).astype(np.float64)


def stat_errors(mean, rstd, x, samples, rows, C, groups, eps, kinds):
    """Worst figures of (mean, rstd) [samples][groups] against float64, each in units of its budget's scale:
    rstd: |rstd / rstd64 - 1| over all groups (constant groups: against eps^-1/2, the same number);
    mean: |mean - mean64| / std64 over the non-constant groups; const_ulps: |mean - c| in fp32 ulps of c over the constant ones."""
    m64, v64, r64 = reference(x, samples, rows, C, groups, eps)
    mean, rstd = np.asarray(mean, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    assert mean.shape == m64.shape and rstd.shape == r64.shape
    assert np.isfinite(mean).all() and np.isfinite(rstd).all(), "non-finite statistics"
    const = kinds == "constant"
    out = {"rstd": float(np.abs(rstd / r64 - 1).max()), "mean": 0.0, "const_ulps": 0.0}
    if (~const).any():
        out["mean"] = float((np.abs(mean - m64)[~const] / np.sqrt(v64[~const])).max())
    if const.any():
        out["const_ulps"] = float((np.abs(mean - m64)[const] / _ulp32(m64[const])).max())
    return out


def within_stat_budgets(e):
    return e["rstd"] <= RSTD_REL and e["mean"] <= MEAN_SIG and e["const_ulps"] <= 2.0


def assert_stats(mean, rstd, x, samples, rows, C, groups, eps, kinds, what=""):
    e = stat_errors(mean, rstd, x, samples, rows, C, groups, eps, kinds)
    print(f"gn_cond {what}: rstd rel err {e['rstd']:.3e} (budget {RSTD_REL:.3e}), mean err / std {e['mean']:.3e} "
          f"(budget {MEAN_SIG:.3e}), constant groups' mean {e['const_ulps']:.2f} ulp (budget 2)")
    assert e["rstd"] <= RSTD_REL, f"{what}: rstd off by {e['rstd']:.3e} relative > 2^-14"
    assert e["mean"] <= MEAN_SIG, f"{what}: mean off by {e['mean']:.3e} std > 2^-13"
    assert e["const_ulps"] <= 2.0, f"{what}: mean of a constant group off by {e['const_ulps']:.2f} fp32 ulps > 2"
    return e


def output_excess(y, y64, gamma, C, groups, kinds, samples, rows, silu):
    """max of |y - y64| / (2^-10 |y64| + 2^-12 |gamma_c| (x 1.1 with SiLU)) over the non-constant groups (<= 1: inside the
    budget); every value, constant groups included, must be finite."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == y64.shape and np.isfinite(y).all(), "non-finite output"
    tol = OUT_REL * np.abs(y64) + OUT_ABS * (1.1 if silu else 1.0) * np.abs(np.asarray(gamma, dtype=np.float64))[None, :]
    cg = C // groups
    ex = (np.abs(y - y64) / tol).reshape(samples, rows, groups, cg).max(axis=(1, 3))
    live = kinds != "constant"
    return float(ex[live].max()) if live.any() else 0.0


def assert_output(y, y64, gamma, C, groups, kinds, samples, rows, silu, what=""):
    ex = output_excess(y, y64, gamma, C, groups, kinds, samples, rows, silu)
    print(f"gn_cond {what}: worst output error {ex:.3f} of its budget")
    assert ex <= 1.0, f"{what}: output error {ex:.3f} x the budget 2^-10 |y| + 2^-12 |gamma|"
    return ex


def affine(C, seed=0):
    """gamma in +-[0.5, 1.5], beta ~ N(0, 1): float32."""
    g = np.random.default_rng([19, C, seed])
    gamma = (g.uniform(0.5, 1.5, C) * g.choice([-1.0, 1.0], C)).astype(np.float32)
    return gamma, g.standard_normal(C).astype(np.float32)


def emulate_onepass(x, samples, rows, C, groups, eps, row_threads=51):
    """numpy fp32 model of the raw one-pass statistic: row_threads threads per column take rows t, t + row_threads, ... each and
    add x and x^2 row by row, the threads' sums are added in order, then the group's cg columns in order; mean = gs / n,
    M2 = gq - gs mean clamped at 0.  (A fixed order of the kernels' kind, not their exact thread geometry: only the conditioning.)"""
    cg = C // groups
    v = np.asarray(x, dtype=np.float32).reshape(samples, rows, C)
    pad = (-rows) % row_threads
    v = np.concatenate([v, np.zeros((samples, pad, C), dtype=np.float32)], axis=1).reshape(samples, -1, row_threads, C)
    ts = np.zeros((samples, row_threads, C), dtype=np.float32)
    tq = np.zeros((samples, row_threads, C), dtype=np.float32)
    for r in range(v.shape[1]):
        ts += v[:, r]
        tq += v[:, r] * v[:, r]
    s = np.zeros((samples, C), dtype=np.float32)
    q = np.zeros((samples, C), dtype=np.float32)
    for t in range(row_threads):
        s += ts[:, t]
        q += tq[:, t]
    s, q = s.reshape(samples, groups, cg), q.reshape(samples, groups, cg)
    gs = np.zeros((samples, groups), dtype=np.float32)
    gq = np.zeros((samples, groups), dtype=np.float32)
    for c in range(cg):
        gs += s[:, :, c]
        gq += q[:, :, c]
    n = np.float32(rows * cg)
    mean = gs / n
    m2 = np.maximum(gq - gs * mean, np.float32(0))
    rstd = (np.float32(1) / np.sqrt(m2 / n + np.float32(eps))).astype(np.float32)
    return mean, rstd


# ---- producers: a GEMM / convolution whose epilogue places the offsets --------------------------------------------------------
PRODUCER_BAND = (0.85, 1.25)          # stored rows' ratio / intended ratio (zero padding at the image border lowers the std a little)


def producer_plan(samples, C, groups, case, per_sample, seed=0):
    """What a producer needs for its stored rows to be a `case` tensor: offset [samples][C] (the epilogue's bias, row vector or
    residual: per channel mu_g + the channel's own shift; with per_sample the sign of mu differs from sample to sample, else
    every sample gets the same row), scale [C] (the std the GEMM part must contribute: its weight rows are scaled by it) and
    kinds [samples][groups] (by group only: the weights are shared by the samples)."""
    cg = C // groups
    g = np.random.default_rng([23, samples, C, groups, CASES.index(case), seed])
    cyc = ("control", "r256", "constant")
    kinds = np.empty((samples, groups), dtype=object)
    offset = np.zeros((samples, C))
    scale = np.zeros(C)
    for gi in range(groups):
        kind = cyc[gi % 3] if case == "mixed" else case
        kinds[:, gi] = kind
        sl = slice(gi * cg, (gi + 1) * cg)
        sign = 1.0 if g.random() < 0.5 else -1.0
        chan = g.standard_normal(cg)
        chan -= chan.mean()           # the channels' shifts leave the group's offset where it was put
        if kind == "constant":
            mu = np.full(cg, CONSTANTS[gi] if gi < len(CONSTANTS) else sign * np.exp(g.uniform(np.log(0.1), np.log(1000.0))))
            sig = 0.0
        elif kind == "control":
            mu, sig = 0.7 * sign + 2.0 * 0.3 * chan / 1.09 ** 0.5, 2.0 / 1.09 ** 0.5
        elif kind in RATIO:
            m = sign * np.exp(g.uniform(np.log(4.0), np.log(1000.0)))
            sig = abs(m) / RATIO[kind] / 1.09 ** 0.5
            mu = m + 0.3 * sig * chan
        else:   # spread
            m = sign * np.exp(g.uniform(np.log(4.0), np.log(100.0)))
            sig = abs(m) / 64.0
            mu = m + g.uniform(0.5, 4.0) * sig * chan
        scale[sl] = sig
        for s in range(samples):
            flip = -1.0 if per_sample and kind != "constant" and s % 2 else 1.0
            offset[s, sl] = flip * mu
    return offset.astype(np.float32), scale.astype(np.float32), kinds


def assert_stored_band(rows_, samples, rows, C, groups, kinds):
    """The rows a producer STORED (f16) hold what the case intends: group ratios in the band, constant groups constant."""
    m, v, _ = reference(rows_, samples, rows, C, groups, 0.0 + 1e-30)
    for kind in set(kinds.reshape(-1)):
        sel = kinds == kind
        if kind == "constant":
            assert (v[sel] == 0).all() and (m[sel] != 0).all(), "a constant group is not constant in the stored rows"
            continue
        ratio = np.abs(m[sel]) / np.sqrt(v[sel])
        if kind in RATIO:
            lo, hi = PRODUCER_BAND[0] * RATIO[kind], PRODUCER_BAND[1] * RATIO[kind]
        elif kind == "control":
            lo, hi = 0.25, 0.5
        else:
            lo, hi = 8.0, 75.0
        assert (ratio >= lo).all() and (ratio <= hi).all(), (kind, float(ratio.min()), float(ratio.max()), lo, hi)
