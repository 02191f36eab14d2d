"""LayerNorm rows that lie far from zero, their float64 reference, the error budgets and fp32 models of the statistic: shared by
tests/test_ln_cond_host.py (CPU: the inputs are fair to the reference's operation and discriminate against the raw one-pass
E[x^2] - mean^2) and tests/test_hip_ln_cond.py (GPU: rcdm_layernorm, rcdm_gemm_ln and rcdm_gemm_lnx stay inside the budgets).
Needs numpy only.  Built like tests/gn_cond.py, whose helpers it reuses: one LayerNorm row plays the part of one (sample, group).

Cases (every value an f16-representable float32):
  control   mean / sigma = 0.35: the draw of the other LayerNorm tests
  r64, r128, r256   |mean| / sigma = 64, 128, 256 with |mean| log-uniform in [4, 1000], both signs; the ratio is that of the
            float64 mean and std of the f16-ROUNDED row and is asserted (gn_cond.RATIO_BAND)
  spread    the row's columns in blocks of 64, block means spread by 0.5 .. 4 sigma of the noise, the noise at |mean| / 64: the
            per-tile pivots of the deferred form differ, and its merge has to combine them
  mixed     consecutive rows cycle control / r256 / constant: an error must not leak to the neighbours inside a tile
  constant  every value of a row is one f16 number c != 0: gn_cond.CONSTANTS in the first rows, then +-[0.1, 1000)

Shapes (M, C), the smallest that reach every code path of the deferred form: (300, 64) one statistics slot; (97, 200) a ragged
last column tile (72 columns behind a 128-wide producer tile, 8 behind a 64-wide one) and a ragged M; (1000, 640) 5 or 10
slots, ragged M; (640, 1280) 10 or 20 slots: the short and the long form of the consumer's merge.

Budgets, GroupNorm's and for the same reasons (gn_cond.py): they come from the f16 OUTPUT, not from any kernel.
  statistics   |rstd / rstd64 - 1| <= RSTD_REL = 2^-14, |mean - mean64| / std64 <= MEAN_SIG = 2^-13.
               Constant rows: mean within 2 fp32 ulps of c, and |rstd eps^1/2 - 1| <= 2^-14 + (2 ulp32(c))^2 / (2 eps): what a
               mean off by 2 ulps turns into through var <= delta^2.
  plain LayerNorm output (rcdm_layernorm, rcdm_gemm_ln)
               non-constant rows |y - y64| <= 2^-10 |y64| + 2^-12 |gamma_c|;
               constant rows |y - beta_c| <= 2^-10 |beta_c| + 2 ulp32(c) eps^-1/2 |gamma_c|: two-pass fp32 at a mean off by 2 ulps.
  deferred consumer (rcdm_gemm_lnx): y = rstd (x W'^T) - rstd mean S + b'.  W' has 32 non-zeros per row from {+-1/8, +-1/4}
               and gamma is from {+-1, +-1/2}, so f16(W gamma) = W' exactly.  A row at ratio >= 64 spans at most two binades, so
               every partial sum of x W'^T is a multiple of 2^-3 ulp16(x) below 2^24 of them: the fp32 accumulator is exact in
               any order (asserted on the CPU by summing in three orders) and the budget has no accumulation term:
               |y - y64| <= 2^-10 |y64| + 2^-12 |y64 - b'_n| + 2^-11 |S_n|: twice the sum of the f16 rounding, RSTD_REL on
               (y - b') and (MEAN_SIG + 2 * 274 * 2^-24) on S_n (the fp32 rounding of the two terms of size 274 |S_n|).
               Constant rows: |y - b'_n| <= 2^-10 |b'_n| + 2 ulp32(c) eps^-1/2 A_n, A_n = sum_c |W'_nc|.
               GEGLU: out = h gelu(g); with the budgets bh, bg of the two halves and |gelu'| <= 1.13:
               |out - out64| <= 2^-10 |out64| + bh |gelu(g64)| + 1.13 bg (|h64| + bh); the first term is twice the rounding of
               the stored f16.
  `control` rows are not exact in the accumulator and keep test_hip_lnx.py's close(rel = 4e-3, abs_frac = 6e-3).

Models (fp32 numpy, a fixed order of the kernels' kind; only the conditioning matters):
  emulate_onepass   slots of (sum x, sum x^2) per column tile, var = E[x^2] - mean^2 clamped at 0: the rule this suite retired
  emulate_tiles     the library's rule (igemm_args.h): per column tile t of n_t columns the pivot k = the row's first value of
                    the tile, d = x - k (exact), slot = (sum d + n_t k, max(0, sum d^2 - (sum d)^2 / n_t)) = (sum_t, M2_t);
                    merge about K = sum_0 / n_0: U = sum_t n_t (sum_t / n_t - K), Q = sum_t [M2_t + n_t (sum_t / n_t - K)^2],
                    mean = K + U / C, var = max(0, Q - U^2 / C) / C
  emulate_twopass   mean = sum / C, var = sum (x - mean)^2 / C"""
import numpy as np

from tests import gn_cond as G

CASES = G.CASES
SHAPES = [(300, 64), (97, 200), (1000, 640), (640, 1280)]
EPS = 1e-5
RSTD_REL, MEAN_SIG, OUT_REL, OUT_ABS = G.RSTD_REL, G.MEAN_SIG, G.OUT_REL, G.OUT_ABS
GELU_SLOPE = 1.13
f16 = G.f16
_f32 = np.float32


def ulp32(c):
    return G._ulp32(c)


def row_kinds(M, case):
    k = np.empty(M, dtype=object)
    k[:] = case
    if case == "mixed":
        cyc = ("control", "r256", "constant")
        for m in range(M):
            k[m] = cyc[m % 3]
    return k


def make_input(M, C, case, seed=0):
    """f16-rounded rows [M][C] (float32) of `case`; asserts what the case promises about the ROUNDED values."""
    assert case in CASES
    g = np.random.default_rng([29, M, C, CASES.index(case), seed])
    kinds = row_kinds(M, case)
    x = np.empty((M, C), dtype=np.float64)
    nconst = 0
    for m in range(M):
        kind = kinds[m]
        if kind == "spread":
            sign = 1.0 if g.random() < 0.5 else -1.0
            mu = sign * np.exp(g.uniform(np.log(4.0), np.log(100.0)))
            blk = g.standard_normal((C + 63) // 64)
            blk = (blk - blk.mean()) / blk.std() if blk.size > 1 else np.zeros(1)     # block means: std 1 exactly
            noise = g.standard_normal(C)
            noise = (noise - noise.mean()) / noise.std()                              # the noise: std 1 exactly
            x[m] = mu + (abs(mu) / 64.0) * (noise + g.uniform(0.5, 4.0) * blk[np.arange(C) // 64])
        else:
            x[m] = G._group(g, kind, 1, C, nconst)[0]     # one row = one (sample, group) of gn_cond
            nconst += kind == "constant"
    x = f16(x)
    assert np.isfinite(x).all()
    x64 = x.astype(np.float64)
    mean, var = x64.mean(axis=1), x64.var(axis=1)
    for kind in set(kinds):
        sel = kinds == kind
        if kind == "constant":
            assert (var[sel] == 0).all() and (mean[sel] != 0).all()
            continue
        ratio = np.abs(mean[sel]) / np.sqrt(var[sel])
        if kind in G.RATIO:
            lo, hi = G.RATIO_BAND[0] * G.RATIO[kind], G.RATIO_BAND[1] * G.RATIO[kind]
            assert (ratio >= lo).all() and (ratio <= hi).all(), (kind, ratio.min(), ratio.max())
            assert (np.abs(mean[sel]) >= 3.9).all() and (np.abs(mean[sel]) <= 1010).all()
        elif kind == "control":
            assert (ratio > 0.3).all() and (ratio < 0.4).all(), (ratio.min(), ratio.max())
        else:   # spread: 64 / sqrt(1 + spread^2) (a ragged last block shifts it a little), 64 with one block (C = 64)
            assert (ratio > 8).all() and (ratio < 70).all(), (ratio.min(), ratio.max())
    if case not in ("constant", "control"):
        live = kinds != "constant"
        assert (mean[live] > 0).any() and (mean[live] < 0).any(), "offsets of one sign only"
    return x


def reference(x, eps=EPS):
    """float64 (mean, var, rstd) per row (biased variance)."""
    v = np.asarray(x, dtype=np.float64)
    mean = v.mean(axis=1)
    var = ((v - mean[:, None]) ** 2).mean(axis=1)
    return mean, var, (var + eps) ** -0.5


def layernorm64(x, gamma, beta, eps=EPS, shift=None):
    """float64 y = (x - mean) rstd gamma + beta (+ shift[m][c]: the positional-encoding row of m)."""
    mean, _, rstd = reference(x, eps)
    y = (np.asarray(x, dtype=np.float64) - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64) \
        + np.asarray(beta, dtype=np.float64)
    return y if shift is None else y + np.asarray(shift, dtype=np.float64)


# ---- statistics -------------------------------------------------------------------------------------------------------------
def const_rstd_budget(c, eps=EPS):
    return RSTD_REL + (2.0 * ulp32(c)) ** 2 / (2.0 * eps)


def stat_figures(mean, rstd, x, kinds, eps=EPS, res_rstd=0.0, res_mean=0.0):
    """Worst figure of each statistics budget as a fraction of the budget (<= 1: inside).  res_rstd (relative) and res_mean
    (in sigma) are what the MEASUREMENT adds (the probe consumer of the GPU test): they widen the budgets explicitly."""
    m64, v64, r64 = reference(x, eps)
    mean, rstd = np.asarray(mean, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    assert mean.shape == m64.shape and rstd.shape == r64.shape
    assert np.isfinite(mean).all() and np.isfinite(rstd).all(), "non-finite statistics"
    const = kinds == "constant"
    out = {"rstd": 0.0, "mean": 0.0, "const_mean": 0.0, "const_rstd": 0.0}
    if (~const).any():
        out["rstd"] = float((np.abs(rstd / r64 - 1)[~const]).max() / (RSTD_REL + res_rstd))
        out["mean"] = float((np.abs(mean - m64)[~const] / np.sqrt(v64[~const])).max() / (MEAN_SIG + res_mean))
    if const.any():
        c = m64[const]
        out["const_mean"] = float((np.abs(mean[const] - c) / (2.0 * ulp32(c) + res_mean * eps ** 0.5)).max())
        out["const_rstd"] = float((np.abs(rstd[const] * eps ** 0.5 - 1) / (const_rstd_budget(c, eps) + res_rstd)).max())
    return out


def assert_stats(mean, rstd, x, kinds, what="", **kw):
    e = stat_figures(mean, rstd, x, kinds, **kw)
    print(f"ln_cond {what}: of the budgets: rstd {e['rstd']:.3f}, mean {e['mean']:.3f}, constant rows' mean {e['const_mean']:.3f}, "
          f"constant rows' rstd {e['const_rstd']:.3f}")
    for k, v in e.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} x its budget"
    return e


# ---- plain LayerNorm output -------------------------------------------------------------------------------------------------
def plain_output_excess(y, x, gamma, beta, kinds, eps=EPS, shift=None):
    """max |y - y64| / budget over all rows (constant rows against beta_c (+ shift) with their own budget); everything finite."""
    y = np.asarray(y, dtype=np.float64)
    y64 = layernorm64(x, gamma, beta, eps, shift)
    assert y.shape == y64.shape and np.isfinite(y).all(), "non-finite output"
    ag = np.abs(np.asarray(gamma, dtype=np.float64))[None, :]
    tol = OUT_REL * np.abs(y64) + OUT_ABS * ag
    const = kinds == "constant"
    if const.any():
        c = np.asarray(x, dtype=np.float64)[const, :1]
        tol[const] = OUT_REL * np.abs(y64[const]) + 2.0 * ulp32(c) * eps ** -0.5 * ag      # y64 = beta_c (+ shift) there
    return float((np.abs(y - y64) / tol).max())


def assert_plain_output(y, x, gamma, beta, kinds, what="", **kw):
    ex = plain_output_excess(y, x, gamma, beta, kinds, **kw)
    print(f"ln_cond {what}: worst output error {ex:.3f} of its budget")
    assert ex <= 1.0, f"{what}: output error {ex:.3f} x its budget"
    return ex


def affine(C, seed=0):
    return G.affine(C, seed)


# ---- deferred consumer ------------------------------------------------------------------------------------------------------
def consumer_weights(N, C, seed=0):
    """W' [N][C] (32 non-zeros per row from {+-1/8, +-1/4}), gamma [C] from {+-1, +-1/2}, beta [C] from {0, +-1/4}, bias [N]:
    W = W' / gamma is what the reference's Linear holds; f16(W gamma) = W' exactly.  Returns float64 arrays and
    S = row sums of W', b' = fl32(bias + W beta), A = row sums of |W'|."""
    g = np.random.default_rng([31, N, C, seed])
    Wp = np.zeros((N, C))
    for n in range(N):
        cols = g.choice(C, 32, replace=False)
        Wp[n, cols] = g.choice([0.125, 0.25], 32) * g.choice([-1.0, 1.0], 32)
    gamma = g.choice([1.0, 0.5], C) * g.choice([-1.0, 1.0], C)
    beta = g.choice([0.0, 0.25, -0.25], C)
    bias = 0.1 * g.standard_normal(N)
    W = Wp / gamma[None, :]
    assert (f16(W * gamma[None, :]) == Wp).all()
    bp = (bias + W @ beta).astype(np.float32).astype(np.float64)
    return {"Wp": Wp, "gamma": gamma, "beta": beta, "bias": bias, "W": W, "S": Wp.sum(axis=1), "bp": bp, "A": np.abs(Wp).sum(axis=1)}


def consumer64(x, w, eps=EPS, shift=None):
    """float64 LayerNorm(x) W^T + bias in the folded form, exactly: (x - mean) rstd W'^T + b' (+ shift[m][n]: a row vector)."""
    mean, _, rstd = reference(x, eps)
    y = ((np.asarray(x, dtype=np.float64) - mean[:, None]) * rstd[:, None]) @ w["Wp"].T + w["bp"][None, :]
    return y if shift is None else y + np.asarray(shift, dtype=np.float64)


def consumer_budget(y64, w, x, kinds, eps=EPS, shift=None):
    """[M][N] budget of a plain / row-vector consumer; NaN on control rows (they keep test_hip_lnx.py's tolerance)."""
    bp = w["bp"][None, :] + (0.0 if shift is None else np.asarray(shift, dtype=np.float64))
    tol = OUT_REL * np.abs(y64) + 2.0 ** -12 * np.abs(y64 - bp) + 2.0 ** -11 * np.abs(w["S"])[None, :]
    const = kinds == "constant"
    if const.any():
        c = np.asarray(x, dtype=np.float64)[const, :1]
        tol[const] = (OUT_REL * np.abs(bp) * np.ones_like(y64))[const] + 2.0 * ulp32(c) * eps ** -0.5 * w["A"][None, :]
    tol[kinds == "control"] = np.nan
    return tol


def gelu64(v):
    from math import erf
    return 0.5 * v * (1.0 + np.vectorize(erf)(v / np.sqrt(2.0)))


def geglu_budget(h64, g64, bh, bg):
    """Budget of out = h gelu(g) from the budgets of its halves (|gelu'| <= 1.13) and the f16 rounding of the stored value."""
    gl = gelu64(g64)
    return OUT_REL * np.abs(h64 * gl) + bh * np.abs(gl) + GELU_SLOPE * bg * (np.abs(h64) + bh)


def control_close(got, ref, rel=4e-3, abs_frac=6e-3):
    """test_hip_lnx.py's close() on the control rows: |got - ref| <= abs_frac max |ref| + rel |ref|; returns the worst fraction."""
    if not got.size:
        return 0.0
    tol = abs_frac * np.abs(ref).max() + rel * np.abs(ref)
    return float((np.abs(got - ref) / tol).max())


# ---- fp32 models of the statistic -------------------------------------------------------------------------------------------
def _rsqrt32(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(_f32)


def _tiles(C, bn):
    return [(c0, min(bn, C - c0)) for c0 in range(0, C, bn)]


def emulate_onepass(x, bn, eps=EPS):
    x = np.asarray(x, dtype=_f32)
    M, C = x.shape
    S, Q = np.zeros(M, _f32), np.zeros(M, _f32)
    for c0, n in _tiles(C, bn):
        s, q = np.zeros(M, _f32), np.zeros(M, _f32)
        for c in range(c0, c0 + n):
            s = s + x[:, c]
            q = q + x[:, c] * x[:, c]
        S, Q = S + s, Q + q
    invC = _f32(1.0) / _f32(C)
    mean = S * invC
    var = np.maximum((Q * invC).astype(np.float64) - mean.astype(np.float64) ** 2, 0).astype(_f32)     # one fma
    return mean, _rsqrt32(var + _f32(eps))


def emulate_tiles(x, bn, eps=EPS):
    x = np.asarray(x, dtype=_f32)
    M, C = x.shape
    slots = []
    for c0, n in _tiles(C, bn):
        k = x[:, c0]
        s, q = np.zeros(M, _f32), np.zeros(M, _f32)
        for c in range(c0, c0 + n):
            d = x[:, c] - k
            s = s + d
            q = q + d * d
        nf = _f32(n)
        slots.append((s + nf * k, np.maximum(q - s * (s * (_f32(1) / nf)), _f32(0)), nf))
    invC = _f32(1.0) / _f32(C)
    K = slots[0][0] * (_f32(1) / slots[0][2])
    U, Q = np.zeros(M, _f32), np.zeros(M, _f32)
    for st, m2, nf in slots:
        dlt = st * (_f32(1) / nf) - K
        w = nf * dlt
        U = U + w
        Q = Q + (w * dlt + m2)
    um = U * invC
    mean = K + um
    var = np.maximum(Q - U * um, _f32(0)) * invC
    return mean, _rsqrt32(var + _f32(eps))


def emulate_twopass(x, eps=EPS):
    x = np.asarray(x, dtype=_f32)
    M, C = x.shape
    s = np.zeros(M, _f32)
    for c in range(C):
        s = s + x[:, c]
    mean = s * (_f32(1.0) / _f32(C))
    q = np.zeros(M, _f32)
    for c in range(C):
        d = x[:, c] - mean
        q = q + d * d
    return mean, _rsqrt32(q * (_f32(1.0) / _f32(C)) + _f32(eps))


def twopass_output(x, gamma, beta, eps=EPS):
    """f16 output of a two-pass fp32 LayerNorm: ((x - mean) rstd) gamma + beta with fp32 roundings."""
    x = np.asarray(x, dtype=_f32)
    mean, rstd = emulate_twopass(x, eps)
    y = ((x - mean[:, None]) * rstd[:, None]) * np.asarray(gamma, _f32)[None, :] + np.asarray(beta, _f32)[None, :]
    return f16(y)


def deferred_output(x, w, mean, rstd, staged=False):
    """f16 output of the deferred consumer from fp32 statistics: f16(fl32(acc rstd - (mean rstd) S + b')) — the accumulator
    acc = x W'^T is exact (float64 here).  staged: the LDS-DMA tiles' order, which rounds acc rstd - (mean rstd) S to f16
    BEFORE b' is added in fp32 and the sum is rounded again."""
    acc = (np.asarray(x, dtype=np.float64) @ w["Wp"].T).astype(_f32)
    mr = (mean * rstd).astype(_f32)
    t = (acc.astype(np.float64) * rstd[:, None].astype(np.float64)
         - (mr[:, None] * w["S"].astype(_f32)[None, :]).astype(np.float64)).astype(_f32)      # one fma
    if staged:
        t = f16(t)
    return f16(t + w["bp"].astype(_f32)[None, :])
