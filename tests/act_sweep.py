"""Pointwise functions on every f16 input against float64, site by site: the erf GELU in its two polynomial forms (three-term
Abramowitz & Stegun 7.1.25: gelu2 of csrc/common.h behind gelu8 / act8 / geglu8; five-term 7.1.26: geglu_slice of rowff.hip),
quick-GELU (quick_gelu2), SiLU (silu_f), Mish (mish_kernel) and the sinusoidal timestep embedding (timestep_embed_kernel).
Shared by tests/test_act_sweep_host.py (CPU: fp32 models of the forms stay inside their budgets on the whole grid, a model
with one misplaced term does not, and the facts the comment above gelu2 states) and tests/test_hip_act_sweep.py (GPU: every
site that evaluates one of them, fed so that the pre-activation reaches the function exactly).  Needs numpy only.

Grids.  GRID16: every f16 value that is zero or normal, both signs (2 + 2 * 30 * 1024 = 61 442 values; f16 subnormals are left
out because most sites take the value through an MFMA).  GRID_FF, for the fused feed-forward (320 values per launch): every
f16 value in [-6.5, -0.5] short of -6.5 — the gates on which the two GELU forms differ — plus every 16th value of GRID16
with |x| <= 16.  No comparison skips or masks a value of its grid.

References (float64).  gelu: x / 2 * erfc(-x / sqrt 2) for x < 0 (no cancellation in the tail), x - x / 2 * erfc(x / sqrt 2)
otherwise; math.erfc, value by value.  quick-GELU x / (1 + exp(-1.702 x)), SiLU x / (1 + exp(-x)), both as
x e^-|a| / (1 + e^-|a|) on the negative side; Mish x tanh(log1p(e^x)); the embedding cos | sin (t exp(-ln(1e4) i / half)).

Budget.  |out - ref| <= rounding + form + evaluation, every term derived, none measured:

  rounding    ulp16(y) = 2^(max(floor(log2 |y|), -14) - 10).  n * ulp16(ref) / 2 for the n roundings to f16 the site performs
              on the way (each site of the GPU test states its n; every site here has n = 1: where a tile is staged through
              LDS as f16 first, the staged value is the f16 pre-activation itself, exactly), but never less than one
              subnormal step 2^-24, so that neither keeping nor flushing f16 subnormals fails.  fp32 outputs: no term.
  form        three-term GELU 1.25e-5 |x|: A&S 7.1.25 bounds |erf error| by 2.5e-5 and gelu = x (1 + erf) / 2.  Five-term
              0.75e-7 |x| (7.1.26: 1.5e-7).  0 for the others, which evaluate their definition.
  evaluation  fp32, v_exp_f32 and v_rcp_f32 at 1 ulp (u = 2^-24 below is the relative error of one correctly rounded fp32
              operation, 2 u that of a 1-ulp instruction):
              GELU  max(x, 0) - |x| q, q = poly(t) t 2^(-x^2 log2(e) / 2).  t: fma + rcp, 3 u.  poly by Horner in t <= 1, at
              most five fmas on coefficients below 1: 5 u absolute on a value <= 1/2.  The exponent x^2 c is rounded twice
              and scaled by ln 2 |x^2 c| <= x^2 / 2 in the result, where q <= exp(-x^2 / 2) / 2 makes x^2 / 2 * q <= 0.19:
              below 1 u absolute.  exp2 2 u, two products 2 u, the final fma 1 u of the result.  |x| q collects less than
              8 u |x| times q <= 1/2 plus 1 u |ref|: inside 8 u (|x| + |ref|), used for both forms.
              quick-GELU  max(x, 0) - |x| q, q = 1 / (1 + 2^(k |x|)), k = 1.702 log2(e) as an fp32 constant (0.5 u).  The
              exponent's relative error 1.5 u is an absolute 1.5 u k |x| ln 2 <= 1.702 u |x| (the factor 1 - q <= 1 that
              carries it into q taken as 1); exp2 2 u and the sum 1 u reach q with the same factor, rcp 2 u directly:
              q (1 + (4 + 1.702 |x|) u) with room for one more u; the final fma 1 u of the result:
              (4 + 1.702 |x|) u |x| q + u |ref|.
              Both GELU families: fp32 arithmetic flushes below 2^-126 (q, and the result): 2^-126 (1 + |x|) on top.
              SiLU  x rcp(1 + 2^(-x log2 e)): the exponent's two roundings, 2 u |x| ln2 log2(e) = 2 u |x| in the
              result; exp2 2 u, sum 1 u, rcp 2 u, product 1 u: (6 + 2 |x|) u |ref|.  Where exp overflows to infinity
              (x < -88.7) the result is -0 for a true value below 1e-36: an absolute floor of 1e-30.
              Mish  x tanhf(log1pf(__expf(x))): as SiLU for the exponential, log1pf and tanhf at 2 u each and the
              product: (8 + 2 |x|) u |ref|, floor 1e-30.
              embedding  w = expf(-(9.2103 i) / half): the argument's three roundings give 3 u |arg| w, expf 2 u w, the
              constant and the product t w 2 u: |t| w (4 + 3 |arg|) u in the angle, whose derivative is at most 1;
              cosf / sinf and the result's own rounding 2^-22.
  GroupNorm   the self-finalising apply kernel forms the pre-activation itself: f = fma(x, rstd gamma, shift), rstd =
              rsqrtf(var + eps) — sum, rsqrt (2 u), product, fma: 4 u |f| — and |silu'| <= 1.1: 1.1 * 4 u |f| more.

The Winograd input transform (wino.hip: silu_f on the GroupNorm output inside the 4x4 input transform) is left out on
purpose: it calls the same silu_f, and its values are summed by the transform before anything can be observed.

MUTATIONS: fp32 models with one misplaced term each, for the host test to show that the budgets reject them and how much of
each close() of tests/test_hip_kernels.py lets through on random normal operands."""
import math

import numpy as np

U = 2.0 ** -24
LN1E4 = math.log(10000.0)
F32 = np.float32


# ---- grids --------------------------------------------------------------------------------------------------------------
def _grid16():
    bits = np.arange(1 << 16, dtype=np.uint16)
    e = (bits >> 10) & 31
    keep = ((e >= 1) & (e <= 30)) | ((bits & 0x7FFF) == 0)
    g = bits[keep].view(np.float16)
    return g[np.argsort(g.astype(np.float64), kind="stable")]


GRID16 = _grid16()
assert GRID16.size == 61442 and np.isfinite(GRID16).all()


def _grid_ff():
    g = GRID16.astype(np.float64)
    dense = GRID16[(g < 0) & (np.abs(g) >= 0.5) & (np.abs(g) < 6.5)]
    coarse = GRID16[::16]
    coarse = coarse[np.abs(coarse.astype(np.float64)) <= 16]
    both = np.concatenate([dense, coarse]).view(np.uint16)
    return np.unique(both).view(np.float16)


GRID_FF = _grid_ff()


def off_grid(x16):
    """The fp32 arguments of the fp32-in sites: the f16 values, and the same values times 1 + 2^-13 (exact in fp32, never an
    f16 value)."""
    x = x16.astype(np.float32)
    y = x * F32(1.0 + 2.0 ** -13)
    assert (y.astype(np.float64) == x.astype(np.float64) * (1.0 + 2.0 ** -13)).all()
    return np.concatenate([x, y])


def ulp16(y):
    y = np.abs(np.asarray(y, dtype=np.float64))
    e = np.full(y.shape, -14.0)
    nz = y > 0
    e[nz] = np.maximum(np.floor(np.log2(y[nz])), -14.0)
    return 2.0 ** (e - 10.0)


def f16r(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


# ---- float64 references ---------------------------------------------------------------------------------------------------
def _per_value(fn, x):
    x = np.asarray(x, dtype=np.float64)
    u, inv = np.unique(x, return_inverse=True)
    return np.array([fn(float(t)) for t in u])[inv].reshape(x.shape)


def _gelu1(t):
    r = math.sqrt(0.5)
    return 0.5 * t * math.erfc(-t * r) if t < 0 else t - 0.5 * t * math.erfc(t * r)


def gelu64(x):
    return _per_value(_gelu1, x)


def _sig_neg(a):
    """sigmoid(-|a|) and |a| -> e^-|a| / (1 + e^-|a|), no overflow."""
    e = np.exp(-np.abs(a))
    return e / (1.0 + e)


def quick64(x):
    x = np.asarray(x, dtype=np.float64)
    q = _sig_neg(1.702 * x)
    return np.where(x < 0, x * q, x * (1.0 - q))


def silu64(x):
    x = np.asarray(x, dtype=np.float64)
    q = _sig_neg(x)
    return np.where(x < 0, x * q, x * (1.0 - q))


def mish64(x):
    x = np.asarray(x, dtype=np.float64)
    sp = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    return x * np.tanh(sp)


def temb64(t, dim, swap=False, half_minus_one=False):
    """[rows][dim]: cos | sin (t w_i), w_i = exp(-ln(1e4) i / half)."""
    half = dim // 2
    i = np.arange(half, dtype=np.float64)
    den = (half - 1) if half_minus_one else half
    a = np.asarray(t, dtype=np.float64)[:, None] * np.exp(-LN1E4 * i / max(den, 1))[None, :]
    c, s = np.cos(a), np.sin(a)
    return np.concatenate([s, c] if swap else [c, s], axis=1)


# ---- budgets ------------------------------------------------------------------------------------------------------------
def rounding(ref, n=1):
    """n roundings to f16 on the way to an f16 output; one subnormal step at the least."""
    return np.maximum(n * ulp16(ref) / 2.0, 2.0 ** -24)


FORM = {"gelu3": 1.25e-5, "gelu5": 0.75e-7}


FTZ = 2.0 ** -126


def eval_gelu(x, ref):
    return 8.0 * U * (np.abs(x) + np.abs(ref)) + FTZ * (1.0 + np.abs(x))


def eval_quick(x, ref):
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return (4.0 + 1.702 * ax) * U * ax * _sig_neg(1.702 * ax) + U * np.abs(ref) + FTZ * (1.0 + ax)


def eval_silu(x, ref):
    return (6.0 + 2.0 * np.abs(x)) * U * np.abs(ref) + 1e-30


def eval_mish(x, ref):
    return (8.0 + 2.0 * np.abs(x)) * U * np.abs(ref) + 1e-30


def budget(kind, x, ref, n_round=0, scale=1.0, extra=0.0):
    """The budget of one site.  kind: gelu3 | gelu5 | quick | silu | mish; n_round: roundings to f16 (0: an fp32 output);
    scale: |factor| the function's value is multiplied by in fp32 before it is rounded (GEGLU's hidden value; the product
    costs one more u of the result); ref: the float64 value that is stored (the factor included); extra: a further absolute
    term the site's docstring derives."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(scale)
    if kind in FORM:
        b = scale * (FORM[kind] * np.abs(x) + eval_gelu(x, ref / np.where(scale == 0, 1.0, scale)))
    elif kind == "quick":
        b = scale * eval_quick(x, ref / np.where(scale == 0, 1.0, scale))
    elif kind == "silu":
        b = eval_silu(x, ref)
    else:
        assert kind == "mish", kind
        b = eval_mish(x, ref)
    b = b + np.where(np.asarray(scale) != 1.0, U * np.abs(ref), 0.0) + extra
    if n_round:
        b = b + rounding(ref, n_round)
    return b


def budget_temb(t, dim):
    half = dim // 2
    arg = LN1E4 * np.arange(half, dtype=np.float64) / half
    w = np.exp(-arg)
    b = np.abs(np.asarray(t, dtype=np.float64))[:, None] * (w * (4.0 + 3.0 * arg) * U)[None, :] + 2.0 ** -22
    return np.concatenate([b, b], axis=1)


def worst(err, bud, where):
    """(largest err / budget, the entry of `where` it occurs at).  Every element takes part."""
    err, bud = np.asarray(err, dtype=np.float64), np.asarray(bud, dtype=np.float64)
    assert err.shape == bud.shape and (bud >= 0).all()
    assert np.isfinite(err).all(), "a non-finite result"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bud > 0, err / bud, np.where(err == 0, 0.0, np.inf))     # a budget of 0 (x = 0, unrounded): only 0 passes
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), float(np.broadcast_to(np.asarray(where, dtype=np.float64), err.shape).reshape(-1)[i])


# ---- fp32 models: numpy float32, step by step in the order of the source ------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64; its sum with c is rounded there first, which differs
    from the single rounding in rare ties only."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _rcp(d):
    return (F32(1.0) / d).astype(F32)


def _exp2(z):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(z.astype(np.float64)).astype(F32)


GELU3 = dict(p=0.3326725, c=(0.3739278, -0.0479399, 0.1740121), k=-0.72134752044)
GELU5 = dict(p=0.2316418882, c=(0.5307027145, -0.7265760135, 0.7107068705, -0.142248368, 0.127414796), k=-0.72134752044)


def gelu_f32(x, form=GELU3):
    """gelu2 of common.h (form GELU3) / geglu_slice of rowff.hip (GELU5): max(x, 0) - |x| poly(t) t exp2(k x^2)."""
    x = np.asarray(x, dtype=F32)
    ax = np.abs(x)
    t = _rcp(_fma(ax, F32(form["p"]), F32(1.0)))
    c = [F32(v) for v in form["c"]]
    p = _fma(t, c[0], c[1])
    for v in c[2:]:
        p = _fma(p, t, v)
    # gelu2: xx = x * x * k, q = p * t * e; geglu_slice: ex = exp2(x * x * k), t = pl * t, t = t * ex — the same order
    e = _exp2(((x * x).astype(F32) * F32(form["k"])).astype(F32))
    q = ((p * t).astype(F32) * e).astype(F32)
    return _fma(-ax, q, np.maximum(x, F32(0.0)))


QUICK_K = 2.45546696          # 1.702 * log2(e), as quick_gelu2 writes it


def quick_f32(x, k=QUICK_K):
    x = np.asarray(x, dtype=F32)
    ax = np.abs(x)
    with np.errstate(over="ignore"):
        d = (F32(1.0) + _exp2((ax * F32(k)).astype(F32))).astype(F32)
    return _fma(-ax, _rcp(d), np.maximum(x, F32(0.0)))


def silu_f32(x, sign=-1.0):
    """silu_f: x * rcp(1 + __expf(-x)), __expf(a) = exp2(a * log2(e))."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore"):
        e = _exp2(((F32(sign) * x) * F32(1.4426950408889634)).astype(F32))
        return (x * _rcp((F32(1.0) + e).astype(F32))).astype(F32)


# ---- mutations ----------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "gelu3_coef": "the first A&S 7.1.25 coefficient of gelu2 off by 1e-4 (0.3739278 -> 0.3740278)",
    "gelu5_coef": "the last A&S 7.1.26 coefficient of geglu_slice off by 1e-6 (0.127414796 -> 0.127415796)",
    "gelu5_under_gelu3_budget": "the same five-term mutant judged by the three-term budget: accepted, which is why each form has its own",
    "quick_1p7": "quick-GELU with 1.7 in place of 1.702",
    "quick_digits": "quick-GELU's exponent constant with two digits transposed (2.45548296 for 2.45546696: what quick_gelu2 held)",
    "gelu_no_log2e": "exp2(-x^2 / 2) without the factor log2(e): -0.5 in place of -0.72134752",
    "silu_sigmoid_plus": "SiLU as x * (1 - sigmoid(x)): exp(+x) in the denominator",
    "geglu_swap": "GEGLU with hidden and gate swapped: gate * gelu(hidden)",
    "mish_no_softplus": "Mish without the softplus: x * tanh(x)",
    "temb_swap": "the embedding's halves swapped: sin | cos",
    "temb_half_minus_one": "the embedding's exponent over half - 1 (freq_shift = 1)",
}


def _with(form, **kw):
    f = dict(form)
    f.update(kw)
    return f


def mutant(name, x, hidden=None):
    """(values, float64 reference, budget) of the mutated fp32 model on the arguments x — before any rounding to f16, so a
    mutant the budget rejects here is rejected by more than any rounding term.  geglu_swap takes the hidden value too."""
    x64 = np.asarray(x, dtype=np.float64)
    if name == "gelu3_coef":
        got, ref, kind = gelu_f32(x, _with(GELU3, c=(0.3740278, -0.0479399, 0.1740121))), gelu64(x64), "gelu3"
    elif name in ("gelu5_coef", "gelu5_under_gelu3_budget"):
        got, ref = gelu_f32(x, _with(GELU5, c=GELU5["c"][:4] + (0.127415796,))), gelu64(x64)
        kind = "gelu5" if name == "gelu5_coef" else "gelu3"
    elif name == "quick_1p7":
        got, ref, kind = quick_f32(x, 1.7 * 1.4426950408889634), quick64(x64), "quick"
    elif name == "quick_digits":
        got, ref, kind = quick_f32(x, 2.45548296), quick64(x64), "quick"
    elif name == "gelu_no_log2e":
        got, ref, kind = gelu_f32(x, _with(GELU3, k=-0.5)), gelu64(x64), "gelu3"
    elif name == "silu_sigmoid_plus":
        got, ref, kind = silu_f32(x, +1.0), silu64(x64), "silu"
    elif name == "geglu_swap":
        h = np.full(x64.shape, float(hidden))
        got = (np.asarray(x, F32) * gelu_f32(h.astype(F32))).astype(F32)
        ref = h * gelu64(x64)
        return got.astype(np.float64), ref, budget("gelu3", x64, ref, scale=h)
    elif name == "mish_no_softplus":
        got, ref, kind = (np.asarray(x, F32) * np.tanh(np.asarray(x, F32))).astype(F32), mish64(x64), "mish"
    else:
        raise KeyError(name)
    return got.astype(np.float64), ref, budget(kind, x64, ref)


TEMB_T = [0.0, 1.0, 0.5, 499.75, 981.0, 999.0, -3.0]
TEMB_DIMS = [2, 6, 320, 1280]
TEMB_ROWS = [1, 3, 64]


def temb_rows(rows):
    """rows timesteps: TEMB_T over and over."""
    return np.array([TEMB_T[i % len(TEMB_T)] for i in range(rows)], dtype=np.float32)


def close_accepts(got, ref, rel=2e-3, abs_frac=4e-3):
    """Elementwise: would close() of tests/test_hip_kernels.py accept got against ref?"""
    tol = abs_frac * np.abs(ref).max() + rel * np.abs(ref)
    return np.abs(got - ref) <= tol


# ---- the fused feed-forward's operands ------------------------------------------------------------------------------------
FF_C, FF_M, FF_SCALE = 320, 160, 2.0 ** 13
FF_ZERO = 2.0 ** -120        # a true |gelu| below this is "0": no fp32 hidden bias lifts it to [1, 2)


def ff_case(vals):
    """One launch of the fused feed-forward on up to 320 gate values (f16).  Token rows +-1 (LayerNorm: mean 0, variance 1,
    gamma 1, beta 0: y = +-1 exactly), all rows with the SAME sign pattern s: the gate row of hidden unit j is one-hot with
    the swept value at a column where s = +1, so gate = w_j in every row (with independent patterns a column would also see
    -w_j under the same hidden bias, and for the tail values that product overflows f16: an infinity times the zeros of
    GEMM2 would destroy the row).  Hidden rows zero, hidden bias p_j = a power of two with |p_j gelu(w_j)| in [1, 2); W2
    selects unit j into output column j with the entry 2^13: acc = 2^13 h in [8192, 16384), where f16 is spaced 8 apart and
    the +-1 residual and b2 = 0 are rounded away: h = out / 2^13 bit for bit.  Where the true gelu is 0 (below 2^-120):
    p = 1 and out = tok."""
    C, M = FF_C, FF_M
    n = len(vals)
    assert 0 < n <= C
    w = np.zeros(C)
    w[:n] = np.asarray(vals, dtype=np.float64)
    g = np.random.default_rng([41, n, int(np.asarray(vals[:1]).view(np.uint16)[0])])
    s = g.permutation(np.repeat([1.0, -1.0], C // 2))
    plus = np.nonzero(s > 0)[0]
    col = plus[g.integers(0, plus.size, size=C)]
    gel = gelu64(w)
    zero = np.abs(gel) < FF_ZERO
    p = np.where(zero, 1.0, 2.0 ** -np.floor(np.log2(np.where(zero, 1.0, np.abs(gel)))))
    w1, b1 = np.zeros((8 * C, C)), np.zeros(8 * C)
    w1[4 * C + np.arange(C), col] = w
    b1[:C] = p
    w2 = np.zeros((C, 4 * C))
    w2[np.arange(C), np.arange(C)] = FF_SCALE
    tok = np.tile(s, (M, 1))
    h_ref = p * gel
    c = dict(vals=w, n=n, s=s, col=col, p=p, zero=zero, w1=w1, b1=b1, w2=w2, b2=np.zeros(C), tok=tok, h_ref=h_ref,
             ln_g=np.ones(C), ln_b=np.zeros(C))
    # the conditions, on the reference alone
    assert (np.abs(tok) == 1).all() and (tok.sum(axis=1) == 0).all()
    assert (s[col] == 1).all() and (f16r(w1) == w1).all() and (f16r(w2) == w2).all()
    assert (b1.astype(np.float32) == b1).all() and np.isfinite(b1.astype(np.float32)).all()
    gate = tok @ w1[4 * C:5 * C].T
    assert (gate == w[None, :]).all(), "the gate pre-activation is not the swept value"
    live = ~zero
    assert ((np.abs(h_ref[live]) >= 1) & (np.abs(h_ref[live]) < 2)).all()
    assert (np.abs(h_ref[zero]) < FF_ZERO).all()
    h16 = f16r(h_ref)
    acc = FF_SCALE * h16
    assert (f16r(acc) == acc).all() and ((np.abs(acc[live]) >= 8192) & (np.abs(acc[live]) <= 16384)).all()
    for d in (-1.0, 1.0):        # the residual cannot change what is stored
        assert (f16r(acc[live] + d) == acc[live]).all()
        lo = FF_SCALE * (np.abs(h16[live]) - 2.0 ** -10) * np.sign(h16[live])      # ... nor one step below, across 8192
        assert (f16r(lo + d) == lo).all()
    return c
