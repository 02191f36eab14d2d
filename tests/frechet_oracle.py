"""The Fréchet distance of rcdms_amd.frechet restated in numpy float64, for the tests and for tools/mint_frechet_golden.py.

  model       `distance` / `distance_from_moments`: the algorithm of csrc/frechet_core.h operation for operation — the
              round-robin pairing, the rotation and its two rules, rule 3 of the factor step, and `fixed_sum`, the one order
              every reduction has (256 strided partial sums, then a binary tree).  Nothing in it goes through BLAS or a
              library reduction, so it gives the same bits on every machine, and the same bits as tools/frechet_host.cpp.
  definition  `distance_definition`: |dmu|^2 + tr Sa + tr Sb - 2 sum svd(Fb^T Fa) with F = V sqrt(lambda) from eigh, eigenvalues at
              rounding level (rule 3's cut) taken as zero.
  sqrtm       `distance_sqrtm`: what FID scripts compute (scipy.linalg.sqrtm of Sa Sb), for comparison only.
  budget      `budget(d, s, model_error)`: the larger of 4 d 2^-52 s and 8 x the error the model shows against the 60-digit
              value of the case, s = tr Sa + tr Sb + |dmu|^2.  MODEL_ERROR holds those errors: measured against mpmath by
              tools/mint_frechet_golden.py, never against a kernel.  The factor 8 covers another, equally valid summation
              order inside the reductions (the matrix pipe's order within a k-step of four is its own)."""
import os

import numpy as np

LANES = 256
EPS = 2.0 ** -52
RULE1 = 2.0 ** -50
MAX_SWEEPS = 30
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# case -> |model - mpmath| (tools/mint_frechet_golden.py prints this table; the files carry the same numbers)
MODEL_ERROR = {
    "d1": 1.012739533654554e-15,               # d 1, n 5 / 7
    "d2_n2": 2.220446049250313e-16,            # d 2, n 2 / 2: both covariances of rank 1
    "d31_odd": 6.110984822705476e-12,          # d 31, n 40 / 50: one zero vector of padding
    "d48_full": 2.8787116316983903e-12,        # d 48, n 96 / 80: full rank, eigenvalues falling by 0.9 a step
    "n_lt_d_one": 1.051653086968918e-11,       # d 24, n 10 / 60: rank 9 against rank 24
    "n_lt_d_both": 1.6577732525571687e-12,     # d 24, n 10 / 12: ranks 9 and 11
    "self": 2.2737367544323206e-13,            # d 16, a set against itself: the 60-digit value is 0
    "mean_offset": 6.307490090324354e-13,      # d 16, the second set is the first plus a vector
    "merge": 3.251696142748702e-16,            # d 12, n 33 / 20: the first set is also accumulated in two halves
}
CASES = tuple(MODEL_ERROR)


def load(name):
    with np.load(os.path.join(GOLDEN, f"frechet_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def budget(d, s, model_error):
    return max(4.0 * d * EPS * s, 8.0 * model_error)


def fixed_sum(x):
    """Sum over the last axis in the order of fr (frechet_core.h): lane t adds elements t, t + 256, ... from +0.0, then the
    tree part[t] += part[t + s], s = 128 .. 1."""
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    chunks = max(1, -(-L // LANES))
    pad = np.zeros(x.shape[:-1] + (chunks * LANES,))
    pad[..., :L] = x
    pad = pad.reshape(x.shape[:-1] + (chunks, LANES))
    part = np.zeros(x.shape[:-1] + (LANES,))
    for c in range(chunks):
        part = part + pad[..., c, :]
    s = LANES // 2
    while s:
        part = part[..., :s] + part[..., s:2 * s]
        s //= 2
    return part[..., 0]


def pairs(rows, rnd):
    """The rows / 2 disjoint pairs (p < q) of round rnd = 0 .. rows - 2."""
    m = rows - 1
    i = np.arange(rows // 2)
    a = np.where(i == 0, rnd, (rnd + i) % m)
    b = np.where(i == 0, m, (rnd - i + m) % m)
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(W, dim):
    """One-sided Jacobi over the rows of W (an even number of them) until a sweep rotates nothing.  -> (W, rotations per sweep)."""
    W = np.array(W, np.float64)
    rows = W.shape[0]
    assert rows % 2 == 0
    counts = []
    for _ in range(MAX_SWEEPS):
        t = dim * EPS
        thr = (t * t) * fixed_sum(W * W).max()
        count = 0
        for rnd in range(rows - 1):
            p, q = pairs(rows, rnd)
            P, Q = W[p], W[q]
            a, b, g = fixed_sum(P * P), fixed_sum(Q * Q), fixed_sum(P * Q)
            with np.errstate(all="ignore"):
                rot = (a > thr) & (b > thr) & (np.abs(g) > RULE1 * (np.sqrt(a) * np.sqrt(b)))
                zeta = (b - a) / (2.0 * g)
                t_ = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t_ * t_)
                s = c * t_
            k = np.nonzero(rot)[0]
            if k.size:
                ck, sk = c[k, None], s[k, None]
                W[p[k]] = ck * P[k] - sk * Q[k]
                W[q[k]] = sk * P[k] + ck * Q[k]
                count += int(k.size)
        counts.append(count)
        if count == 0:
            return W, counts
    raise RuntimeError(f"no convergence in {MAX_SWEEPS} sweeps: rotations {counts}")


def moments(x, shift=None):
    """x (n, d) float32 / float16 -> (mean, cov or None, n): sums about `shift` (default: the float32-rounded mean), rows in
    ascending order; the three operations of the finalize step."""
    x = np.asarray(x)
    n, d = x.shape
    k = (x.astype(np.float64).mean(axis=0).astype(np.float32) if shift is None else np.asarray(shift, np.float32)).astype(np.float64)
    xc = x.astype(np.float64) - k
    s = np.zeros(d)
    outer = np.zeros((d, d))
    for r in range(n):
        s = s + xc[r]
        outer = outer + np.outer(xc[r], xc[r])
    return finalize(k, s, outer, n)


def finalize(k, s, outer, n):
    mean = k + s / n
    cov = (outer - np.outer(s, s) / n) / (n - 1) if n >= 2 else None
    return mean, cov, n


def factor(cov):
    """-> (F (d, rows) with cov = F F^T up to rule 3, rank, rotations per sweep)."""
    d = cov.shape[0]
    rows = d + (d & 1)
    W = np.zeros((rows, d))
    W[:d] = cov
    W, counts = jacobi(W, d)
    lam = np.sqrt(fixed_sum(W * W))
    keep = lam > (d * EPS) * lam.max()
    F = np.zeros((d, rows))
    F[:, keep] = (W[keep] / np.sqrt(lam[keep])[:, None]).T
    return F, int(keep.sum()), counts


def gemm_tn(A, B):
    """A^T B with k ascending, one rounding per product and per sum."""
    C = np.zeros((A.shape[1], B.shape[1]))
    for k in range(A.shape[0]):
        C = C + np.outer(A[k], B[k])
    return C


def distance_from_moments(mu_a, cov_a, mu_b, cov_b):
    d = mu_a.shape[0]
    Fa, rank_a, ca = factor(cov_a)
    Fb, rank_b, cb = factor(cov_b)
    M, cm = jacobi(gemm_tn(Fb, Fa), d)
    sqrt_trace = float(fixed_sum(np.sqrt(fixed_sum(M * M))))
    df = mu_a - mu_b
    mean_term = float(fixed_sum(df * df))
    trace_a, trace_b = float(fixed_sum(np.diag(cov_a))), float(fixed_sum(np.diag(cov_b)))
    return dict(distance=((mean_term + trace_a) + trace_b) - 2.0 * sqrt_trace, mean_term=mean_term, trace_a=trace_a, trace_b=trace_b,
                sqrt_trace=sqrt_trace, rank_a=rank_a, rank_b=rank_b, sweeps=(len(ca), len(cb), len(cm)), counts=(ca, cb, cm))


def distance(xa, xb):
    ma, ca, _ = moments(xa)
    mb, cb, _ = moments(xb)
    return distance_from_moments(ma, ca, mb, cb)


def scale(mu_a, cov_a, mu_b, cov_b):
    """s = tr Sa + tr Sb + |dmu|^2, what the budget is relative to."""
    return float(np.trace(cov_a) + np.trace(cov_b) + ((mu_a - mu_b) ** 2).sum())


def distance_definition(mu_a, cov_a, mu_b, cov_b):
    def f(c):
        lam, v = np.linalg.eigh(c)
        # eigenvalues at rounding level are cut as rule 3 cuts them: the root of a noise eigenvalue 1e-16 lmax is 1e-8
        # sqrt(lmax), which is how the eigh and sqrtm routes lose half their digits on a rank-deficient covariance
        return v * np.sqrt(np.where(lam > c.shape[0] * EPS * lam.max(), lam, 0.0))
    sv = np.linalg.svd(f(cov_b).T @ f(cov_a), compute_uv=False)
    return float(((mu_a - mu_b) ** 2).sum() + np.trace(cov_a) + np.trace(cov_b) - 2.0 * sv.sum())


def distance_sqrtm(mu_a, cov_a, mu_b, cov_b):
    from scipy import linalg
    root = linalg.sqrtm(cov_a @ cov_b)
    return float(((mu_a - mu_b) ** 2).sum() + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.trace(root).real)
