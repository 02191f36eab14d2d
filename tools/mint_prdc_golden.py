"""Write tests/golden/prdc_<case>.npz: two small sets of features, nearest_k, the exact radii, per-sample vectors and numerators
of the manifold figures (rcdms_amd/csrc/prdc_core.h), the radii at 60 digits (mpmath), the a-priori bounds and what the numpy
model of the device algorithm (tests/prdc_oracle.py) gives on them.

  python tools/mint_prdc_golden.py [case ...]

The features are float32 values on a grid of 2^-10 (float16-representable ones: 2^-4), so that every squared distance is an exact
Python int of the scaled features: the reference starts from exact integers, never from a float64 dot.
A case is refused (nothing written, exit status 1) unless EVERY comparison the definition makes has a margin above twice the
a-priori bound of tests/prdc_oracle.py:
  |D2(X_i, Y_j) - rX2[i]| and |D2(X_i, Y_j) - rY2[j]| for every (i, j), against 2 max(B_ij, the radius's bound);
  the gap between the k-th and the (k + 1)-th neighbour of every row of X and of Y, against 2 x the radius's bound.
Any evaluation inside the bound then returns the same integers.  One exemption, recorded in the file as margin_safe = 0: a set
against itself has exact ties at every radius by construction (D2(X_i, Y_j) IS the distance that defines the radius); there only
margins that are exactly zero between identical pairs of rows are let through, and any evaluation that computes D2(a, b) as one
function of the two rows gives the same value on both sides.
Needs mpmath; the tests and the GPU do not, the files carry the numbers.  Prints the smallest relative margin per case."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import prdc_oracle as O  # noqa: E402

DIGITS = 60
GRID32, GRID16 = 10, 4


def features(seed, n, d, relu=False, centre=0.0, grid=GRID32, scale=1.0):
    rng = np.random.RandomState(seed)
    x = np.clip(rng.standard_normal((n, d)) * scale + centre, -7.5, 7.5)
    if relu:
        x = np.maximum(x, 0.0)
    x = np.round(x * 2.0 ** grid) / 2.0 ** grid
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)
    if grid == GRID16:
        assert np.array_equal(out.astype(np.float16).astype(np.float64), x)
    return out


def cases():
    """name -> (x, y, k, grid)."""
    c = {}
    c["n17_23_d5_k3"] = (features(1, 17, 5), features(2, 23, 5), 3, GRID32)
    c["n33_40_d48_k5"] = (features(3, 33, 48), features(4, 40, 48), 5, GRID32)
    c["n65_70_d130_k5"] = (features(5, 65, 130), features(6, 70, 130), 5, GRID32)
    c["n300_300_d256_k5"] = (features(7, 300, 256), features(8, 300, 256), 5, GRID32)
    c["f16"] = (features(9, 40, 24, grid=GRID16), features(10, 36, 24, grid=GRID16, centre=0.25), 5, GRID16)
    c["relu"] = (features(11, 48, 64, relu=True), features(12, 50, 64, relu=True), 5, GRID32)
    xs = features(13, 40, 16)
    c["self"] = (xs, xs.copy(), 5, GRID32)
    xo = features(14, 36, 16)
    off = features(15, 1, 16, scale=0.5)
    yo = (xo.astype(np.float64) + off.astype(np.float64)).astype(np.float32)
    assert np.array_equal(yo.astype(np.float64), xo.astype(np.float64) + off.astype(np.float64))
    c["mean_offset"] = (xo, yo, 5, GRID32)
    c["clusters"] = (features(16, 30, 8, centre=-3.0, scale=0.25), features(17, 34, 8, centre=3.0, scale=0.25), 3, GRID32)
    c["k1"] = (features(18, 20, 6), features(19, 25, 6), 1, GRID32)
    c["k16"] = (features(20, 40, 12), features(21, 45, 12), 16, GRID32)
    assert list(c) == list(O.CASES)
    return c


def scaled(x, grid):
    q = np.asarray(x, np.float64) * 2.0 ** grid
    assert np.array_equal(q, np.round(q))
    return q.astype(np.int64)


def exact_distances(a, b):
    """int64 squared distances of the scaled features (exact: below 2^53 by far), as Python ints in an object array."""
    diff = a[:, None, :] - b[None, :, :]
    D = (diff * diff).sum(axis=2)
    assert D.max() < 2 ** 52
    return D.astype(object)


def mint(name, x, y, k, grid):
    import mpmath as mp
    mp.mp.dps = DIGITS + 10
    xq, yq = scaled(x, grid), scaled(y, grid)
    unit = 4 ** grid                                  # D2 = D / unit, exactly
    nx, ny = len(x), len(y)
    is_self = np.array_equal(x, y)

    def radii(D):
        n = len(D)
        srt = [sorted(int(D[i, j]) for j in range(n) if j != i) for i in range(n)]
        return [s[k - 1] for s in srt], [s[k] - s[k - 1] if len(s) > k else None for s in srt]

    Dxx, Dyy, Dxy = exact_distances(xq, xq), exact_distances(yq, yq), exact_distances(xq, yq)
    rx, gapx = radii(Dxx)
    ry, gapy = radii(Dyy)
    Bxy, Brx, Bry = O.bound(x, y), O.radius_bound(x), O.radius_bound(y)

    worst = np.inf                                    # the smallest margin / (2 x bound)
    for r, gap, Br in ((rx, gapx, Brx), (ry, gapy, Bry)):
        for i, g in enumerate(gap):
            if g is not None:
                worst = min(worst, (g / unit) / (2.0 * Br[i]))
    ties = 0
    for i in range(nx):
        for j in range(ny):
            dij = int(Dxy[i, j])
            for r, Br in ((rx[i], Brx[i]), (ry[j], Bry[j])):
                if is_self and dij == r:
                    ties += 1                         # the same pair of rows on both sides
                    continue
                worst = min(worst, (abs(dij - r) / unit) / (2.0 * max(Bxy[i, j], Br)))
    rel = min(abs(int(Dxy[i, j]) - r) / max(r, 1) for i in range(nx) for j in range(ny) for r in (rx[i], ry[j])
              if not (is_self and int(Dxy[i, j]) == r))
    print(f"{name}: smallest margin = {worst:.3e} x (2 x bound), smallest relative margin {rel:.3e}, largest bound "
          f"{max(Bxy.max(), Brx.max(), Bry.max()):.3e}, exact ties let through: {ties}")
    if not worst > 1.0:
        print(f"{name}: REFUSED, a comparison lies within twice the a-priori bound")
        return False

    fake_count = [sum(1 for i in range(nx) if int(Dxy[i, j]) <= rx[i]) for j in range(ny)]
    real_hit = [int(any(int(Dxy[i, j]) <= ry[j] for j in range(ny))) for i in range(nx)]
    real_min = [min(int(Dxy[i, j]) for j in range(ny)) for i in range(nx)]
    counts = [sum(1 for c in fake_count if c > 0), sum(real_hit), sum(fake_count), sum(1 for i in range(nx) if real_min[i] <= rx[i])]
    digits = lambda v: np.array([mp.nstr(mp.mpf(int(e)) / unit, DIGITS) for e in v])
    exact = lambda v: np.array([int(e) / unit for e in v], np.float64)        # exact: an integer below 2^53 over a power of two

    model = O.evaluate(x, y, k)
    if not (np.array_equal(model["counts"], counts) and np.array_equal(model["fake_count"], fake_count) and
            np.array_equal(model["real_hit"], real_hit)):
        print(f"{name}: REFUSED, the numpy model misses the exact integers")
        return False
    if not ((np.abs(model["radii2_real"] - exact(rx)) <= Brx).all() and (np.abs(model["radii2_fake"] - exact(ry)) <= Bry).all()):
        print(f"{name}: REFUSED, the numpy model's radii lie outside the bound")
        return False
    np.savez_compressed(
        os.path.join(O.GOLDEN, f"prdc_{name}.npz"), x=x, y=y, k=np.int32(k), grid=np.int32(grid), counts=np.array(counts, np.int64),
        fake_count=np.array(fake_count, np.int32), real_hit=np.array(real_hit, np.int32), real_min2=exact(real_min),
        radii2_real=exact(rx), radii2_fake=exact(ry), radii2_real_digits=digits(rx), radii2_fake_digits=digits(ry),
        bound_real=Brx, bound_fake=Bry, bound_min2=Bxy.max(axis=1), margin_safe=np.int32(0 if is_self else 1),
        worst_margin=np.float64(worst), model_radii2_real=model["radii2_real"], model_radii2_fake=model["radii2_fake"],
        model_real_min2=model["real_min2"])
    return True


def main(argv):
    todo = cases()
    names = argv or list(todo)
    ok = True
    for name in names:
        ok &= mint(name, *todo[name])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
