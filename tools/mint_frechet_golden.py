"""Write tests/golden/frechet_<case>.npz: two small sets of float32 features, the Fréchet distance between them at 60 digits
(mpmath, from the exact values of the features: exact means and covariances, tr (Sa Sb)^(1/2) through two symmetric
eigenproblems), and what the numpy model of the device algorithm (tests/frechet_oracle.py) gives on them.

  python tools/mint_frechet_golden.py [case ...]

A case is refused (nothing written, exit status 1)
  * when the model is further from the 60-digit value than 4 d 2^-52 s, the first term of the test budget (the second, 8 x the
    model's own error, cannot judge the model) and the bound tests/test_frechet_host.py holds the model to: the model is then
    not a reference worth pinning a kernel to;
  * when an eigenvalue of either covariance, or a singular value of Fb^T Fa, lies within a factor 2^10 of the threshold of
    rule 2 / rule 3 (d 2^-52 x the largest): there the cut is a coin toss and kernel and model may differ legitimately.  Exact
    zeros (rank deficiency) are far below the band and are the point of several cases.
Needs mpmath; the tests and the GPU need neither mpmath nor scipy, the files carry the numbers.  Prints the MODEL_ERROR table
of tests/frechet_oracle.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import frechet_oracle as O  # noqa: E402

DIGITS = 60
BAND = 2.0 ** 10


def features(seed, n, d, rank=None, spread=1.0, centre=0.0):
    """n rows of d float32 features: a random mixing of `rank` (default d) unit normals, singular values falling by `spread`."""
    rng = np.random.RandomState(seed)
    r = d if rank is None else rank
    mix = rng.standard_normal((r, d)) * (spread ** np.arange(r))[:, None]
    return (rng.standard_normal((n, r)) @ mix + centre + 0.1 * rng.standard_normal(d)).astype(np.float32)


def cases():
    c = {}
    c["d1"] = (features(1, 5, 1), features(2, 7, 1, centre=0.5))
    c["d2_n2"] = (features(3, 2, 2), features(4, 2, 2, centre=-0.25))
    c["d31_odd"] = (features(5, 40, 31), features(6, 50, 31, centre=0.2))
    c["d48_full"] = (features(7, 96, 48, spread=0.9), features(8, 80, 48, spread=0.93, centre=0.1))
    c["n_lt_d_one"] = (features(9, 10, 24), features(10, 60, 24, centre=0.3))
    c["n_lt_d_both"] = (features(11, 10, 24), features(12, 12, 24, centre=-0.3))
    xa = features(13, 30, 16)
    c["self"] = (xa, xa.copy())
    xo = features(14, 28, 16)
    c["mean_offset"] = (xo, (xo.astype(np.float64) + np.linspace(-1.0, 1.0, 16)).astype(np.float32))
    c["merge"] = (features(15, 33, 12, centre=1.0), features(16, 20, 12))
    return c


def mp_moments(mp, x):
    n, d = x.shape
    X = mp.matrix(x.astype(np.float64).tolist())
    mu = mp.matrix([mp.fsum(X[r, j] for r in range(n)) / n for j in range(d)])
    Xc = mp.matrix(n, d)
    for r in range(n):
        for j in range(d):
            Xc[r, j] = X[r, j] - mu[j]
    return mu, (Xc.T * Xc) / (n - 1)


def mp_distance(mp, xa, xb):
    """-> (distance, s, relative eigenvalues of Sa, of Sb, relative singular values of Fb^T Fa)."""
    d = xa.shape[1]
    mu_a, Sa = mp_moments(mp, xa)
    mu_b, Sb = mp_moments(mp, xb)
    la, Va = mp.eigsy(Sa)
    lb, _ = mp.eigsy(Sb)
    root = mp.matrix(d, d)
    for j in range(d):
        root[j, j] = mp.sqrt(max(la[j], mp.mpf(0)))
    Ra = Va * root * Va.T                                   # Sa^(1/2)
    P = Ra * Sb * Ra
    lp, _ = mp.eigsy((P + P.T) / 2, eigvals_only=False)
    sv = [mp.sqrt(max(v, mp.mpf(0))) for v in lp]
    tr = lambda S: mp.fsum(S[j, j] for j in range(d))
    dmu2 = mp.fsum((mu_a[j] - mu_b[j]) ** 2 for j in range(d))
    s = tr(Sa) + tr(Sb) + dmu2
    rel = lambda v: [float(abs(t) / max(abs(u) for u in v)) if max(abs(u) for u in v) > 0 else 0.0 for t in v]
    return dmu2 + tr(Sa) + tr(Sb) - 2 * mp.fsum(sv), s, rel(list(la)), rel(list(lb)), rel(sv)


def main(argv):
    import mpmath as mp
    mp.mp.dps = DIGITS
    todo = cases()
    names = argv or list(todo)
    table, bad = {}, 0
    for name in names:
        xa, xb = todo[name]
        d = xa.shape[1]
        want, s, ra, rb, rs = mp_distance(mp, xa, xb)
        ma, ca, _ = O.moments(xa)
        mb, cb, _ = O.moments(xb)
        model = O.distance_from_moments(ma, ca, mb, cb)
        err = float(abs(mp.mpf(model["distance"]) - want))
        s = float(s)
        cut = d * O.EPS
        near = [v for v in ra + rb + rs if cut / BAND <= v <= cut * BAND]
        unit = d * O.EPS * s
        print(f"{name}: d {d}, n {xa.shape[0]}/{xb.shape[0]}, distance {float(want):.17g}, s {s:.6g}, |model - mp| {err:.3e} = "
              f"{err / unit:.2f} d eps s, sweeps {model['sweeps']}, ranks {model['rank_a']}/{model['rank_b']}")
        if err > 4.0 * unit:
            print(f"  REFUSED: the model is {err / unit:.1f} d eps s from the {DIGITS}-digit value")
            bad += 1
            continue
        if near:
            print(f"  REFUSED: relative eigen / singular values {near} within 2^10 of the rank threshold {cut:.3e}")
            bad += 1
            continue
        table[name] = err
        np.savez(os.path.join(O.GOLDEN, f"frechet_{name}.npz"), xa=xa, xb=xb, mu_a=ma, cov_a=ca, mu_b=mb, cov_b=cb,
                 mp_distance=np.float64(float(want)), mp_distance_digits=np.array(mp.nstr(want, 50)), scale=np.float64(s),
                 model_distance=np.float64(model["distance"]), model_error=np.float64(err),
                 model_sqrt_trace=np.float64(model["sqrt_trace"]), model_ranks=np.array([model["rank_a"], model["rank_b"]]),
                 model_counts_a=np.array(model["counts"][0]), model_counts_b=np.array(model["counts"][1]),
                 model_counts_m=np.array(model["counts"][2]))
    print("MODEL_ERROR = {")
    for name, err in table.items():
        print(f'    "{name}": {err!r},')
    print("}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
