"""The pivoted-Cholesky route of rcdms_amd.frechet (frechet_distance(..., factor="cholesky")) restated in numpy float64, operation
for operation from csrc/frechet_core.h, on tests/frechet_oracle.py's fixed_sum, gemm_tn and jacobi.

  pivoted_cholesky       rcdm_cholesky_pivoted_f64: step j takes the largest remaining diagonal (np.argmax: the lowest index on a
                         tie), stops when it is not above d 2^-52 x the largest diagonal of the input, and forms the column and
                         the next diagonals lazily inside a panel of NB columns; after a full panel the work matrix takes
                         work -= gemm_tn(P, P).  tools/frechet_host.cpp gives the same bits; the kernel differs inside the
                         trailing update only (the matrix pipe's order within a k-step of four), and not at all where every
                         value is exact.
  distance_from_moments  both factors that way, the rank_b (rounded up to even) x rank_a block of Fb^T Fa, the existing Jacobi on it
                         with dim = d.  A rank of 0 gives sqrt_trace = 0.0 without a Jacobi run.
  MODEL_ERROR            |this model - the 60-digit value| per case, the nine of frechet_oracle and the three of
                         tools/mint_frechet_chol_golden.py, measured against mpmath by that tool, never against a kernel.
  integer_factor         the exact-answer cases: L0 lower triangular, diagonal 2 (d - k) + 8, entries of {-1, 0, 1} below it.  Every
                         Schur complement of L0 L0^T is a matrix of small integers, so any summation order returns L0 itself."""
import numpy as np

from tests import frechet_oracle as O

NB = 16                     # fr::CHOL_NB
PANELS = (16, 32, 64, 128)     # fr::chol_nb_ok

# case -> |model - mpmath| (tools/mint_frechet_chol_golden.py prints this table)
MODEL_ERROR = {
    "d1": 1.012739533654554e-15,
    "d2_n2": 2.220446049250313e-16,
    "d31_odd": 3.6098743928299237e-12,
    "d48_full": 1.628156416760614e-12,
    "n_lt_d_one": 4.6048153081651466e-12,
    "n_lt_d_both": 7.482785507842403e-13,
    "self": 2.8421709430404007e-13,
    "mean_offset": 4.033753335892033e-13,
    "merge": 2.8096539816129138e-14,
    "illcond": 8.832540723708509e-14,              # d 64, n 256 / 256, spectrum k^-4: conditions 4.0e10 and 3.5e11
    "illcond_deficient": 7.368118526352103e-13,    # d 48, n 20 / 30, the same spectrum: ranks 19 and 29
    "tie": 2.7295234147482564e-14,                 # d 15: five copies of one 3 x 3 block, every diagonal five times over
}
NEW_CASES = ("illcond", "illcond_deficient", "tie")
CASES = O.CASES + NEW_CASES


def load(name):
    """The nine cases of frechet_oracle as they are; the new ones from frechet_chol_<name>.npz."""
    if name in O.CASES:
        return O.load(name)
    import os
    with np.load(os.path.join(O.GOLDEN, f"frechet_chol_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def pivoted_cholesky(cov, nb=NB):
    """-> (F (d, d) with column j = column j of P L in the original row order and zeros from the rank on, rank, pivots)."""
    assert nb in PANELS
    work = np.array(cov, np.float64)
    d = work.shape[0]
    F = np.zeros((d, d))
    done = np.zeros(d, bool)
    piv = []
    thr = 0.0
    for j0 in range(0, d, nb):
        j1 = min(j0 + nb, d)
        panel = np.zeros((nb, d))                    # panel[k][i] = F[i][j0 + k]
        base = np.diag(work).copy()
        diag = base.copy()
        for j in range(j0, j1):
            if j == 0:
                thr = (d * O.EPS) * max([0.0] + [v for v in diag if v == v])
            cand = np.where(done | (diag != diag), -np.inf, diag)
            p = int(np.argmax(cand))
            if not (cand[p] > -np.inf and cand[p] > thr):
                return F, j, piv
            cnt = j - j0
            ljj = np.sqrt(cand[p])
            piv.append(p)
            done[p] = True
            rows = panel[:cnt].T                     # (d, cnt): the panel's earlier columns, row by row
            dot = O.fixed_sum(rows * rows[p])
            with np.errstate(all="ignore"):
                c = (work[p] - dot) / ljj
            c[done] = 0.0
            c[p] = ljj
            panel[cnt] = c
            F[:, j] = c
            rows = panel[:cnt + 1].T
            diag = np.where(done, diag, base - O.fixed_sum(rows * rows))
        if j1 < d:
            work = work - O.gemm_tn(panel, panel)
    return F, d, piv


def distance_from_moments(mu_a, cov_a, mu_b, cov_b, nb=NB):
    d = mu_a.shape[0]
    Fa, rank_a, pa = pivoted_cholesky(cov_a, nb)
    Fb, rank_b, pb = pivoted_cholesky(cov_b, nb)
    rows_b = rank_b + (rank_b & 1)
    sqrt_trace, cm = 0.0, []
    if rank_a and rank_b:
        Fbp = np.zeros((d, rows_b))
        Fbp[:, :rank_b] = Fb[:, :rank_b]
        M, cm = O.jacobi(O.gemm_tn(Fbp, Fa[:, :rank_a]), d)
        sqrt_trace = float(O.fixed_sum(np.sqrt(O.fixed_sum(M * M))))
    df = mu_a - mu_b
    mean_term = float(O.fixed_sum(df * df))
    trace_a, trace_b = float(O.fixed_sum(np.diag(cov_a))), float(O.fixed_sum(np.diag(cov_b)))
    return dict(distance=((mean_term + trace_a) + trace_b) - 2.0 * sqrt_trace, mean_term=mean_term, trace_a=trace_a, trace_b=trace_b,
                sqrt_trace=sqrt_trace, rank_a=rank_a, rank_b=rank_b, sweeps=(0, 0, len(cm)), counts=cm, pivots=(pa, pb),
                block=(rows_b, rank_a), factors=(Fa, Fb))


def distance(xa, xb):
    ma, ca, _ = O.moments(xa)
    mb, cb, _ = O.moments(xb)
    return distance_from_moments(ma, ca, mb, cb)


def integer_factor(d, seed=0):
    """L0 (d, d): lower triangular, diagonal 2 (d - k) + 8, entries of {-1, 0, 1} below it."""
    rng = np.random.RandomState(1000 * d + seed)
    L = np.tril(rng.randint(-1, 2, size=(d, d)).astype(np.float64), -1)
    L[np.arange(d), np.arange(d)] = 2.0 * (d - np.arange(d)) + 8.0
    return L


def exact_cases(d):
    """-> [(name, sigma, the F to come back bit for bit, rank)]: full, the first d // 2 columns kept, identity, zero."""
    L = integer_factor(d)
    half = L.copy()
    half[:, d // 2:] = 0.0
    return [("full", L @ L.T, L, d), ("half", half @ half.T, half, d // 2), ("identity", np.eye(d), np.eye(d), d),
            ("zero", np.zeros((d, d)), np.zeros((d, d)), 0)]


def tie_covariance(copies=5):
    """Block-diagonal copies of one 3 x 3 block: every diagonal value occurs `copies` times, the lowest index must win."""
    b = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])
    return np.kron(np.eye(copies), b)
