"""The kernel distance of rcdms_amd.kid restated in numpy float64, for the tests and for tools/mint_kid_golden.py.

  definition  k(x, y) = (gamma <x, y> + c)^p.  One subset = index lists ia, ib of m >= 2 positions:
                Sxx = sum over positions i != j of k(x_ia[i], x_ia[j]), Syy the same over y, Sxy = sum over all i, j of
                k(x_ia[i], y_ib[j]);  mmd2 = (Sxx / (m (m - 1)) + Syy / (m (m - 1))) - 2 (Sxy / (m m)).
              KID = the mean of mmd2 over the subsets and their population standard deviation.
  model       `evaluate`: csrc/kid_core.h operation for operation.  The dot is summed with k ascending, one rounding per
              product and per sum (`dots`); t = gamma dot + c, k = ((t t) t) ...; every block is cut into 64 x 64 tiles whose
              4096 values are summed as the device holds them — thread t of 256 adds its 16 elements `element(t, e)` in order,
              then the tree part[t] += part[t + s] — the symmetric blocks from their upper-triangle tiles only, an off-diagonal
              tile counted twice, the others contributing +0.0; the tile partials in the order ti T + tj through `fixed_sum` of
              tests/frechet_oracle.py.  No ndarray.sum and no BLAS in any reduction: the same bits on every machine, and the bits
              of tools/kid_host.cpp.  The device differs in one place only, the order inside a dot product (the matrix pipe's).
  bound       `bound`: for ANY evaluation that follows the arithmetic rules, to first order
                |mmd2^ - mmd2| <= B = u (p (d + 2) + D + 4) s,    u = 2^-53,
              with T_ij = |gamma| sum_k |x_ik y_jk| + |c|, s = mean_{i != j} T_xx^p + mean_{i != j} T_yy^p + 2 mean T_xy^p and
              D = chain(m), the longest chain of additions of the reduction.  Derivation, to first order in u:
                dot     d exact products summed in any order: error <= (d - 1) u sum_k |x y|;
                t       one rounding for the product with gamma, one for the sum with c: |t^ - t| <= (d + 1) u T, and |t| <= T;
                k       an error of t enters the power p times, the p - 1 products add (p - 1) u:
                        |k^ - k| <= u (p (d + 1) + p - 1) T^p <= u p (d + 2) T^p;
                sums    chains of at most D additions: D u sum |k| <= D u sum T^p more (the doubling of a tile is exact);
                mmd2    a division per sum, the sum of the two symmetric terms, the product with 2 and the last difference:
                        at most four more roundings on any term.
              Dividing by m (m - 1) and m m turns the sums of T^p into the means of s.
              A-priori: nothing in it comes from a kernel's output.
  cases       CASES, the goldens tools/mint_kid_golden.py writes (tests/golden/kid_<case>.npz)."""
import os

import numpy as np

from tests.frechet_oracle import fixed_sum

U = 2.0 ** -53
TILE, THREADS, REGS = 64, 256, 16
XX, YY, XY = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# case -> what it is for (tools/mint_kid_golden.py has the generators)
CASES = {
    "m2_d1": "m 2, d 1: the smallest subset, one off-diagonal pair per symmetric block",
    "m17_d5": "m 17, d 5: one ragged tile, a ragged k-step",
    "m33_d48_relu": "m 33, d 48: non-negative features",
    "m65_d130": "m 65, d 130: four tiles per block, the off-diagonal one counted twice",
    "m40_d256_relu": "m 40, d 256: non-negative features, 16 full k-steps",
    "self": "m 24, d 16: a set against itself (x is y, ia is ib)",
    "mean_offset": "m 28, d 16: the second set is the first plus a vector",
    "f16": "m 20, d 24: float16-representable features",
    "subsets3": "3 subsets of 19 drawn by draw_subsets(31, 45, 3, 19, seed 7) from nx = 31, ny = 45 rows of d 12",
    "linear": "m 21, d 9: p = 1, c = 0 (the linear kernel)",
    "quadratic": "m 18, d 7: p = 2, gamma = 0.5",
}


def load(name):
    with np.load(os.path.join(GOLDEN, f"kid_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def tiles(m):
    return (m + TILE - 1) // TILE


def chain(m):
    """D: 16 additions in a thread, 8 levels of the tile's tree, the strided partial sums and the 8 levels of the fixed sum."""
    n = tiles(m) ** 2
    return REGS + 8 + (n + 255) // 256 + 8


def element_maps():
    """rows[t][e], cols[t][e]: kid::element."""
    t = np.arange(THREADS)[:, None]
    e = np.arange(REGS)[None, :]
    w, lane = t >> 6, t & 63
    rows = (w >> 1) * 32 + (e >> 3) * 16 + (lane >> 4) + 4 * (e & 3)
    cols = (w & 1) * 32 + ((e >> 2) & 1) * 16 + (lane & 15)
    return rows, cols


ROWS, COLS = element_maps()


def dots(A, B):
    """A B^T with k ascending from +0.0, one rounding per product and per sum."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    G = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        G = G + np.outer(A[:, k], B[:, k])
    return G


def kernel(G, gamma, coef0, degree):
    t = np.float64(gamma) * G + np.float64(coef0)
    k = t
    for _ in range(1, degree):
        k = k * t
    return k


def tile_sum(vals, keep):
    """vals, keep: 64 x 64.  The sum of the kept values in the order of one workgroup."""
    v = np.where(keep, vals, 0.0)[ROWS, COLS]          # [thread][register]; a skipped element leaves the sum as it is, as + 0.0 does
    part = np.zeros(THREADS)
    for e in range(REGS):
        part = part + v[:, e]
    s = THREADS // 2
    while s:
        part = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def block_sum(K, block):
    """K: m x m kernel values of one block -> its sum in the device's order."""
    m = K.shape[0]
    T = tiles(m)
    pad = np.zeros((T * TILE, T * TILE))
    pad[:m, :m] = K
    pos = np.arange(T * TILE)
    keep = (pos[:, None] < m) & (pos[None, :] < m)
    if block != XY:
        keep &= pos[:, None] != pos[None, :]
    partials = np.zeros(T * T)
    for ti in range(T):
        for tj in range(T):
            if block != XY and tj < ti:
                continue                                  # not computed: +0.0
            r, c = slice(ti * TILE, (ti + 1) * TILE), slice(tj * TILE, (tj + 1) * TILE)
            s = tile_sum(pad[r, c], keep[r, c])
            partials[ti * T + tj] = 2.0 * s if block != XY and tj > ti else s
    return float(fixed_sum(partials))


def mmd2(sxx, syy, sxy, m):
    off, both = np.float64(m * (m - 1)), np.float64(m * m)
    return float((np.float64(sxx) / off + np.float64(syy) / off) - np.float64(2.0) * (np.float64(sxy) / both))


def subset(xa, yb, gamma, coef0, degree):
    """xa, yb: the m gathered rows of each set -> (Sxx, Syy, Sxy, mmd2)."""
    m = xa.shape[0]
    sxx = block_sum(kernel(dots(xa, xa), gamma, coef0, degree), XX)
    syy = block_sum(kernel(dots(yb, yb), gamma, coef0, degree), YY)
    sxy = block_sum(kernel(dots(xa, yb), gamma, coef0, degree), XY)
    return sxx, syy, sxy, mmd2(sxx, syy, sxy, m)


def evaluate(x, y, ia, ib, gamma, coef0, degree):
    """x (nx, d), y (ny, d); ia, ib (subsets, m) -> (subsets, 4) float64."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    return np.array([subset(x[a], y[b], gamma, coef0, degree) for a, b in zip(np.asarray(ia), np.asarray(ib))])


def kid(values):
    """(mean, population standard deviation) of the subsets' mmd2, added in order."""
    n = len(values)
    total = 0.0
    for v in values:
        total = total + float(v)
    mean = total / n
    sq = 0.0
    for v in values:
        sq = sq + (float(v) - mean) * (float(v) - mean)
    return mean, float(np.sqrt(sq / n))


def bound(x, y, ia, ib, gamma, coef0, degree):
    """B of every subset -> (subsets,).  Magnitudes only: BLAS may form them."""
    x, y = np.abs(np.asarray(x).astype(np.float64)), np.abs(np.asarray(y).astype(np.float64))
    d = x.shape[1]
    out = []
    for a, b in zip(np.asarray(ia), np.asarray(ib)):
        m = len(a)
        xa, yb = x[a], y[b]
        off = ~np.eye(m, dtype=bool)
        txx = (abs(gamma) * (xa @ xa.T) + abs(coef0)) ** degree
        tyy = (abs(gamma) * (yb @ yb.T) + abs(coef0)) ** degree
        txy = (abs(gamma) * (xa @ yb.T) + abs(coef0)) ** degree
        s = txx[off].mean() + tyy[off].mean() + 2.0 * txy.mean()
        out.append(U * (degree * (d + 2) + chain(m) + 4) * s)
    return np.array(out)


# ---- exact integer cases --------------------------------------------------------------------------------------------------
def integer_gamma(d):
    """-> (gamma, its denominator): 1 / d where d is a power of two <= 64, else 1."""
    den = d if d <= 64 and d & (d - 1) == 0 else 1
    return 1.0 / den, den


def integer_reference(xi, yi, ia, ib, den, coef0, degree):
    """Integer features and gamma = 1 / den (a power of two), integer coef0, in Python-int arithmetic:
    k den^p = (dot + coef0 den)^p.  -> ((subsets, 3) float64 sums, exact; the kernel matrices of block xy, (subsets, m, m))."""
    xi, yi = np.asarray(xi).astype(np.int64), np.asarray(yi).astype(np.int64)       # small integers: the int64 dots are exact
    scale = den ** degree
    sums, grams = [], []
    for a, b in zip(np.asarray(ia), np.asarray(ib)):
        m = len(a)
        xa, yb = xi[a], yi[b]
        row = []
        for P, Q, sym in ((xa, xa, True), (yb, yb, True), (xa, yb, False)):
            K = (P.dot(Q.T).astype(object) + int(coef0) * den) ** degree     # object dtype: Python ints from here on
            total = sum(int(K[i, j]) for i in range(m) for j in range(m) if not (sym and i == j))
            assert abs(total) < 2 ** 53
            row.append(total / scale)                                   # a power of two: exact
            if not sym:
                grams.append(np.array([[int(K[i, j]) / scale for j in range(m)] for i in range(m)]))
        sums.append(row)
    return np.array(sums, np.float64), np.array(grams, np.float64)


def integer_features(n, d, seed):
    return np.random.RandomState(seed).randint(-3, 4, size=(n, d))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
