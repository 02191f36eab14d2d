"""Write tests/golden/kid_<case>.npz: two small sets of features, the index lists of the subsets, the three kernel sums and mmd^2
of every subset at 60 digits (mpmath), and what the numpy model of the device algorithm (tests/kid_oracle.py) gives on them.

  python tools/mint_kid_golden.py [case ...]

The features are float32 values on a grid of 2^-20 below 8 in magnitude (float16-representable ones: 2^-8 below 4), so that
every dot product is an exact int64 of the scaled features: the 60-digit values start from exact integers, never from a
float64 dot.  gamma and coef0 enter as the float64 values the kernel gets.
A case is refused (nothing written, exit status 1) when the model misses the 60-digit mmd^2 of a subset by more than the
a-priori bound B of tests/kid_oracle.py: the model is then not a reference worth pinning a kernel to.
Needs mpmath; the tests and the GPU do not, the files carry the numbers.  Prints the model's error over B per case."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import kid_oracle as O  # noqa: E402

DIGITS = 60
GRID32, GRID16 = 20, 8


def features(seed, n, d, relu=False, centre=0.0, grid=GRID32):
    rng = np.random.RandomState(seed)
    limit = 7.5 if grid == GRID32 else 3.5
    x = np.clip(rng.standard_normal((n, d)) + centre, -limit, limit)
    if relu:
        x = np.maximum(x, 0.0)
    x = np.round(x * 2.0 ** grid) / 2.0 ** grid
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)
    if grid == GRID16:
        assert np.array_equal(out.astype(np.float16).astype(np.float64), x)
    return out


def lists(m, subsets=1):
    a = np.tile(np.arange(m, dtype=np.int32), (subsets, 1))
    return a, a.copy()


def cases():
    """name -> (x, y, ia, ib, degree, gamma or None for 1 / d, coef0, grid)."""
    from rcdms_amd.kid import draw_subsets
    c = {}

    def plain(name, seeds, m, d, degree=3, gamma=None, coef0=1.0, **kw):
        c[name] = (features(seeds[0], m, d, **kw), features(seeds[1], m, d, centre=0.25, **kw), *lists(m), degree, gamma, coef0,
                   kw.get("grid", GRID32))

    plain("m2_d1", (1, 2), 2, 1)
    plain("m17_d5", (3, 4), 17, 5)
    plain("m33_d48_relu", (5, 6), 33, 48, relu=True)
    plain("m65_d130", (7, 8), 65, 130)
    plain("m40_d256_relu", (9, 10), 40, 256, relu=True)
    xs = features(11, 24, 16)
    c["self"] = (xs, xs.copy(), *lists(24), 3, None, 1.0, GRID32)
    xo = features(12, 28, 16)
    yo = xo.astype(np.float64) + np.round(np.linspace(-1.0, 1.0, 16) * 2.0 ** 10) / 2.0 ** 10
    assert np.array_equal(yo.astype(np.float32).astype(np.float64), yo)
    c["mean_offset"] = (xo, yo.astype(np.float32), *lists(28), 3, None, 1.0, GRID32)
    plain("f16", (13, 14), 20, 24, grid=GRID16)
    ia, ib = draw_subsets(31, 45, 3, 19, 7)
    c["subsets3"] = (features(15, 31, 12), features(16, 45, 12, centre=-0.25), ia, ib, 3, None, 1.0, GRID32)
    plain("linear", (17, 18), 21, 9, degree=1, coef0=0.0)
    plain("quadratic", (19, 20), 18, 7, degree=2, gamma=0.5)
    assert list(c) == list(O.CASES)
    return c


def mp_subset(mp, xi, yi, grid, gamma, coef0, degree):
    """xi, yi: int64 scaled rows of one subset -> [Sxx, Syy, Sxy, mmd2] as mpf."""
    m = xi.shape[0]
    unit = mp.mpf(2) ** (-2 * grid)
    g, c = mp.mpf(gamma), mp.mpf(coef0)
    sums = []
    for P, Q, sym in ((xi, xi, True), (yi, yi, True), (xi, yi, False)):
        G = P @ Q.T                                            # int64, exact: |entries| < 2^24, d <= 256
        sums.append(mp.fsum((g * (int(G[i, j]) * unit) + c) ** degree for i in range(m) for j in range(m) if not (sym and i == j)))
    off, both = mp.mpf(m * (m - 1)), mp.mpf(m * m)
    return sums + [(sums[0] / off + sums[1] / off) - 2 * (sums[2] / both)]


def main(argv):
    import mpmath as mp
    mp.mp.dps = DIGITS
    todo = cases()
    bad = 0
    for name in argv or list(todo):
        x, y, ia, ib, degree, gamma, coef0, grid = todo[name]
        d = x.shape[1]
        gamma = 1.0 / d if gamma is None else gamma
        xi, yi = np.round(x.astype(np.float64) * 2.0 ** grid).astype(np.int64), np.round(y.astype(np.float64) * 2.0 ** grid).astype(np.int64)
        assert np.abs(xi).max() < 2 ** 24 and np.abs(yi).max() < 2 ** 24 and d <= 256
        want = [mp_subset(mp, xi[a], yi[b], grid, gamma, coef0, degree) for a, b in zip(ia, ib)]
        model = O.evaluate(x, y, ia, ib, gamma, coef0, degree)
        B = O.bound(x, y, ia, ib, gamma, coef0, degree)
        err = np.array([float(abs(mp.mpf(float(model[s, 3])) - want[s][3])) for s in range(len(want))])
        print(f"{name}: m {ia.shape[1]}, d {d}, subsets {len(want)}, mmd2 {float(want[0][3]):.17g}, B {B[0]:.3e}, "
              f"|model - mp| / B {np.max(err / B):.2e}")
        if (err > B).any():
            print("  REFUSED: the model is outside its own bound")
            bad += 1
            continue
        np.savez(os.path.join(O.GOLDEN, f"kid_{name}.npz"), x=x, y=y, ia=ia, ib=ib, degree=np.int32(degree), gamma=np.float64(gamma),
                 coef0=np.float64(coef0), mp=np.array([[float(v) for v in row] for row in want], np.float64),
                 mp_digits=np.array([[mp.nstr(v, 50) for v in row] for row in want]), model=model, model_error=err, bound=B)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
