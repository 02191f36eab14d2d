"""The manifold figures of rcdms_amd.prdc restated in numpy float64, for the tests and for tools/mint_prdc_golden.py.

  definition  D2(a, b) = max(0, (|a|^2 + |b|^2) - 2 <a, b>); rX2[i] = the k-th smallest of { D2(X_i, X_j) : j != i } with
              multiplicity, the exclusion by position; rY2 the same over Y; closed balls:
                fake_count[j] = #{ i : D2(X_i, Y_j) <= rX2[i] }     real_hit[i] = any_j D2(X_i, Y_j) <= rY2[j]
                real_min2[i]  = min_j D2(X_i, Y_j)
                precision = #{ fake_count > 0 } / ny, recall = sum real_hit / nx, density = sum fake_count / (k ny),
                coverage = #{ real_min2 <= rX2 } / nx.
  model       `evaluate`: csrc/prdc_core.h operation for operation.  |a|^2 through `fixed_sum` of tests/frechet_oracle.py over the
              exact products, the dot with k ascending (`dots` of tests/kid_oracle.py), one rounding for the sum of the norms, an
              exact doubling, one rounding for the difference, the clamp.  What follows is selection, integer sums, ors and
              minima: order-free, so numpy's sort and reductions may do it.  The bits of tools/prdc_host.cpp.  The device differs
              in one place only, the order inside a dot product (the matrix pipe's).
  mistakes    `evaluate(..., strict=True)` (open balls, the prdc package's rule), `zero_rows=1` (one unmasked padded row per set:
              the zero vector as a point of both sets) and `strict_coverage=True` (< on coverage alone): what a kernel with one of
              those mistakes computes.  The tests show that each changes at least one count on every integer shape.
  bound       `bound`: |D2^ - D2| <= B = u (d + 2) (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|), u = 2^-53, to first order, for ANY
              evaluation inside the rules (csrc/prdc_core.h has the derivation); a radius is within the largest B of its row.
              A-priori: nothing in it comes from a kernel's output.
  cases       CASES, the goldens tools/mint_prdc_golden.py writes (tests/golden/prdc_<case>.npz)."""
import os

import numpy as np

from tests.frechet_oracle import fixed_sum
from tests.kid_oracle import dots, same_bits  # noqa: F401  (same_bits: for the tests)

U = 2.0 ** -53
MAX_K, MAX_N = 16, 65536
PRECISION, RECALL, DENSITY, COVERAGE = 0, 1, 2, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# case -> what it is for (tools/mint_prdc_golden.py has the generators)
CASES = {
    "n17_23_d5_k3": "nx 17, ny 23, d 5, k 3: one ragged tile, a ragged k-step",
    "n33_40_d48_k5": "nx 33, ny 40, d 48, k 5",
    "n65_70_d130_k5": "nx 65, ny 70, d 130, k 5: four tiles, a ragged k-step",
    "n300_300_d256_k5": "nx = ny 300, d 256, k 5: five tile rows and columns",
    "f16": "nx 40, ny 36, d 24, k 5: float16-representable features on a 2^-4 grid",
    "relu": "nx 48, ny 50, d 64, k 5: non-negative rows",
    "self": "n 40, d 16, k 5: a set against itself (exact ties at the radius by construction; not margin-safe)",
    "mean_offset": "nx = ny 36, d 16, k 5: the second set is the first plus a vector",
    "clusters": "nx 30, ny 34, d 8, k 3: two disjoint clusters, all four figures 0",
    "k1": "nx 20, ny 25, d 6, k 1",
    "k16": "nx 40, ny 45, d 12, k 16",
}


def load(name):
    with np.load(os.path.join(GOLDEN, f"prdc_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def norms2(x):
    x = np.asarray(x).astype(np.float64)
    return fixed_sum(x * x)


def dist2(na, nb, G):
    t = (na[:, None] + nb[None, :]) - 2.0 * G
    return np.where(t > 0.0, t, 0.0)


def kth_smallest(D, k):
    """The k-th smallest of every row, with multiplicity."""
    return np.sort(D, axis=1)[:, k - 1].copy()


def radii2(x, k):
    """(n,) float64: the model's rX2."""
    x = np.asarray(x).astype(np.float64)
    n = x.shape[0]
    nn = norms2(x)
    D = dist2(nn, nn, dots(x, x))
    D[np.arange(n), np.arange(n)] = np.inf          # by position
    return kth_smallest(D, k)


def figures(D, rx2, ry2, strict=False, strict_coverage=False):
    """D (nx, ny), radii -> dict of fake_count, real_hit, real_min2 and the four numerators."""
    inside = (lambda a, b: a < b) if strict else (lambda a, b: a <= b)
    fake_count = inside(D, rx2[:, None]).sum(axis=0).astype(np.int32)
    real_hit = inside(D, ry2[None, :]).any(axis=1).astype(np.int32)
    real_min2 = D.min(axis=1)
    covered = (real_min2 < rx2) if (strict or strict_coverage) else (real_min2 <= rx2)
    counts = np.array([int((fake_count > 0).sum()), int(real_hit.sum()), int(fake_count.astype(np.int64).sum()), int(covered.sum())],
                      np.int64)
    return {"fake_count": fake_count, "real_hit": real_hit, "real_min2": real_min2, "counts": counts}


def evaluate(x, y, k, strict=False, zero_rows=0, strict_coverage=False):
    """x (nx, d), y (ny, d) -> dict: radii2_real, radii2_fake, fake_count, real_hit, real_min2, counts (4 int64)."""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    nx, ny = x.shape[0], y.shape[0]
    if zero_rows:                                    # what a dropped mask lets in: padded rows are the zero vector
        x = np.concatenate([x, np.zeros((zero_rows, x.shape[1]))])
        y = np.concatenate([y, np.zeros((zero_rows, y.shape[1]))])
    rx2, ry2 = radii2(x, k), radii2(y, k)
    D = dist2(norms2(x), norms2(y), dots(x, y))
    out = figures(D[:nx], rx2[:nx], ry2, strict, strict_coverage)
    out["fake_count"] = out["fake_count"][:ny]
    if zero_rows:
        out["counts"][PRECISION] = int((out["fake_count"] > 0).sum())
        out["counts"][DENSITY] = int(out["fake_count"].astype(np.int64).sum())
    out["radii2_real"], out["radii2_fake"] = rx2[:nx], ry2[:ny]
    return out


def ratios(counts, nx, ny, k):
    """precision, recall, density, coverage: the host's four divisions."""
    c = [int(v) for v in counts]
    return c[0] / float(ny), c[1] / float(nx), c[2] / float(k * ny), c[3] / float(nx)


def bound(x, y):
    """B of every D2(x_i, y_j) -> (nx, ny).  Magnitudes only: BLAS may form them."""
    x, y = np.abs(np.asarray(x).astype(np.float64)), np.abs(np.asarray(y).astype(np.float64))
    d = x.shape[1]
    na, nb = (x * x).sum(axis=1), (y * y).sum(axis=1)
    return U * ((d + 2) * ((na[:, None] + nb[None, :]) + 2.0 * (x @ y.T)))


def radius_bound(x):
    """(n,): the largest B of each row of a set against itself."""
    return bound(x, x).max(axis=1)


# ---- exact integer cases --------------------------------------------------------------------------------------------------
def integer_features(n, d, seed):
    """Integers in -3 .. 3, centred: the origin lies inside the cloud, so an unmasked padded row is a near neighbour."""
    return np.random.RandomState(seed).randint(-3, 4, size=(n, d))


def integer_distances(a, b):
    """Exact squared distances of integer rows as Python ints, (na, nb) object array (formed in int64, which small integers
    cannot overflow; every comparison downstream is on Python ints)."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert max(np.abs(a).max(), np.abs(b).max()) < 2 ** 20
    diff = a[:, None, :] - b[None, :, :]
    return (diff * diff).sum(axis=2).astype(object)


def integer_reference(xi, yi, k):
    """Integer features in Python-int arithmetic -> the dict of `evaluate`, every float an exact integer."""
    nx, ny = len(xi), len(yi)

    def radii(z):
        D = integer_distances(z, z)
        return [sorted(int(D[i, j]) for j in range(len(z)) if j != i)[k - 1] for i in range(len(z))]

    rx, ry = radii(xi), radii(yi)
    D = integer_distances(xi, yi)
    fake_count = [sum(1 for i in range(nx) if int(D[i, j]) <= rx[i]) for j in range(ny)]
    real_hit = [int(any(int(D[i, j]) <= ry[j] for j in range(ny))) for i in range(nx)]
    real_min = [min(int(D[i, j]) for j in range(ny)) for i in range(nx)]
    counts = [sum(1 for c in fake_count if c > 0), sum(real_hit), sum(fake_count), sum(1 for i in range(nx) if real_min[i] <= rx[i])]
    return {"radii2_real": np.array(rx, np.float64), "radii2_fake": np.array(ry, np.float64),
            "fake_count": np.array(fake_count, np.int32), "real_hit": np.array(real_hit, np.int32),
            "real_min2": np.array(real_min, np.float64), "counts": np.array(counts, np.int64)}


def same_result(a, b):
    """Two result dicts agree element by element, the floats bit for bit."""
    return (same_bits(a["radii2_real"], b["radii2_real"]) and same_bits(a["radii2_fake"], b["radii2_fake"]) and
            same_bits(a["real_min2"], b["real_min2"]) and np.array_equal(a["fake_count"], b["fake_count"]) and
            np.array_equal(a["real_hit"], b["real_hit"]) and np.array_equal(a["counts"], b["counts"]))


# (nx, ny, d, k): sizes around the 64-wide tile, ragged 16-wide k-steps, k = 1 and k = 16
INTEGER_SHAPES = [(4, 6, 1, 3), (17, 23, 3, 3), (63, 70, 5, 5), (64, 65, 16, 5), (65, 64, 48, 1), (97, 130, 130, 16), (130, 97, 16, 5)]
INTEGER_SALT = {(4, 6, 1): 16, (17, 23, 3): 3, (130, 97, 16): 1}     # the first seeds at which all three mistakes of `evaluate` show
PLANTED = {(97, 130, 130): 16}             # iid rows of this width have no tie at a radius: one is planted (see integer_pair)


def integer_pair(nx, ny, d):
    """The two integer sets of one shape (fixed seeds).  Where PLANTED names the shape with k: rows 1 .. k of X become row 0 with
    one coordinate moved by 1 (another coordinate each), so rX2[0] = 1, and row 0 of Y the same with yet another coordinate:
    real_min2[0] = 1 = rX2[0], a tie that only the closed ball covers."""
    salt = INTEGER_SALT.get((nx, ny, d), 0)
    x, y = integer_features(nx, d, 1000 * nx + ny + salt), integer_features(ny, d, 2000 * ny + nx + salt)
    k = PLANTED.get((nx, ny, d))
    if k:
        for c in range(k + 1):
            row = x[0].copy()
            row[c] += -1 if row[c] == 3 else 1
            if c < k:
                x[1 + c] = row
            else:
                y[0] = row
    return x, y
