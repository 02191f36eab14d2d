"""Shared by the guidance-rescale tests (numpy only): the input generator, the float64 reference of the per-story factor
k_s = phi std(e_c) / std(e) + (1 - phi),  e = e_u + g (e_c - e_u),  two fp32 emulations of how the statistics can be
accumulated, and the budget the device result is held to.

K_REL = 2^-17 on |k / k64 - 1|.  Where it comes from: k is a ratio of two standard deviations of f16 data accumulated in
fp32.  Sums SHIFTED by the story's first element keep every term at the size of the deviations, and their error stays
at a few fp32 ulps of the variance whatever the mean is (measured on the cases below: <= 2^-19.3, test_guidance_host
prints it); raw one-pass sums  sum(x), sum(x^2)  cancel |mean|^2 / std^2 times over and are already 2^-15 off at
|mean| / std = 64.  2^-17 sits between the two with room on both sides, so a kernel passes with shifted (or Welford /
Chan) statistics and fails with raw ones.  It is far below what the loop needs (the f16 UNet's own error is 1e-3)."""
import numpy as np

K_REL = 2.0 ** -17

# (S, f, H, W, ld): tails and three different stories; two stories at 8 x 8; the real accumulation length (5 x 64 x 64)
SHAPES = [(3, 3, 5, 7, 8), (2, 5, 8, 8, 32), (1, 5, 64, 64, 32)]
RATIOS = [0.35, 16, 64, 256]          # |mean| / std of every half
SCALES = [7.5, 2.5]                   # guidance scale g
PHIS = [0.7, 1.0]
LANES = 256


def make_eps(S, f, H, W, ratio, seed):
    """float32 (2 S, f H W, 4) of f16-representable values, unconditional block first.  Story s: offset mu_s, the sign
    alternating by story, |mu_s| log-uniform in [4, 1000] (ratio 0.35: mu = +-0.35 and std 1), std |mu_s| / ratio; each half
    gets its own deviations, normalised to mean 0 / std 1 before the f16 rounding, around the story's offset — the two
    halves of a story have the same sign."""
    rng = np.random.default_rng(seed)
    n = f * H * W
    out = np.empty((2 * S, n, 4), dtype=np.float32)
    for s in range(S):
        sign = 1.0 if s % 2 == 0 else -1.0
        if ratio == 0.35:
            mu, sd = 0.35 * sign, 1.0
        else:
            mu = sign * float(np.exp(rng.uniform(np.log(4.0), np.log(1000.0))))
            sd = abs(mu) / ratio
        for half in range(2):
            z = rng.standard_normal((n, 4))
            z = (z - z.mean()) / z.std(ddof=1)
            out[half * S + s] = (mu + sd * z).astype(np.float16).astype(np.float32)
    return out


def k64(eps, g, phi):
    """float64 reference: (S,) factors from eps (2 S, n, 4)."""
    S = eps.shape[0] // 2
    u, c = eps[:S].astype(np.float64).reshape(S, -1), eps[S:].astype(np.float64).reshape(S, -1)
    e = u + g * (c - u)
    sc, se = c.std(axis=1, ddof=1), e.std(axis=1, ddof=1)
    return np.where(se == 0, 1.0, phi * sc / np.where(se == 0, 1.0, se) + (1.0 - phi))


def _strided_sum32(x):
    """fp32 sum of a 1-D fp32 array: LANES accumulators, accumulator j takes elements j, j + LANES, ... in order; the
    accumulators are then added in order."""
    n = x.shape[0]
    pad = (-n) % LANES
    rows = np.concatenate([x, np.zeros(pad, dtype=np.float32)]).reshape(-1, LANES)
    acc = np.zeros(LANES, dtype=np.float32)
    for r in rows:
        acc = (acc + r).astype(np.float32)
    tot = np.float32(0.0)
    for a in acc:
        tot = np.float32(tot + a)
    return tot


def _var32(x, shifted):
    """Unbiased variance of fp32 x from fp32 sums (one pass raw, or shifted by x[0]); the last few operations in float64 so
    that only the accumulation is under test."""
    d = (x - x[0]).astype(np.float32) if shifted else x
    s = float(_strided_sum32(d))
    q = float(_strided_sum32((d * d).astype(np.float32)))
    n = x.shape[0]
    return max((q - s * s / n) / (n - 1), 0.0)


def k32(eps, g, phi, shifted):
    """The factor from fp32 statistics: `shifted` False is the raw one-pass form, True the form shifted by the first element."""
    S = eps.shape[0] // 2
    g32 = np.float32(g)
    out = np.empty(S)
    for s in range(S):
        u, c = eps[s].reshape(-1), eps[S + s].reshape(-1)
        e = (u + g32 * (c - u).astype(np.float32)).astype(np.float32)
        vc, ve = _var32(c, shifted), _var32(e, shifted)
        out[s] = 1.0 if ve == 0 else phi * (vc / ve) ** 0.5 + (1.0 - phi)
    return out


def rel(k, ref):
    return float(np.max(np.abs(np.asarray(k, dtype=np.float64) / ref - 1.0)))


def seed_of(shape, ratio):
    return 1000 * SHAPES.index(shape) + RATIOS.index(ratio) + 7
