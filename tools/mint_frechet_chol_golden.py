"""Write tests/golden/frechet_chol_<case>.npz, the cases the pivoted-Cholesky route adds to tests/golden/frechet_*.npz, and print
the MODEL_ERROR table of tests/frechet_chol_oracle.py: the error of the numpy model of that route against the 60-digit value of
all twelve cases (for the nine older ones the value is read from their files).

  python tools/mint_frechet_chol_golden.py [case ...]

  illcond             d 64, n 256 / 256: unit normals scaled by k^-2 (a covariance spectrum k^-4) and mixed by a square Gaussian
                      matrix; condition about 1e11, two to three decades inside the cut 1 / (d 2^-52).
  illcond_deficient   d 48, n 20 / 30, the same spectrum: ranks n - 1, which the model must find (refused otherwise).
  tie                 d 15: five block-diagonal copies of one 3 x 3 covariance, so that every diagonal value occurs five times in
                      the same bits and the pivot rule's tie-break decides the order.

The fields are those of tools/mint_frechet_golden.py (the Jacobi model's figures included) plus chol_model_distance,
chol_model_error, chol_model_sqrt_trace, chol_model_ranks, chol_model_counts_m, chol_pivots_a and chol_pivots_b.  A case is
refused as that tool refuses one, with one difference: the band around the rank threshold that must hold no eigenvalue or singular
value is two decades wide (10^2, not 2^10) — the ill-conditioned cases are meant to come close, and within two decades both routes
lose digits (README, "Fréchet distance").  Needs mpmath."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import frechet_chol_oracle as C  # noqa: E402
from tests import frechet_oracle as O  # noqa: E402
from mint_frechet_golden import DIGITS, mp_distance  # noqa: E402

BAND = 100.0


def power_law(seed, n, d, centre=0.0):
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, d)) * np.arange(1, d + 1) ** -2.0
    return (z @ rng.standard_normal((d, d)) + centre).astype(np.float32)


def tied(seed, copies=5, rows=6, centre=0.0):
    """kron(I, Y) for integer Y (rows x 3) whose columns sum to zero, plus a constant: the sample covariance is block diagonal
    with `copies` bit-identical blocks."""
    rng = np.random.RandomState(seed)
    y = rng.randint(-4, 5, size=(rows, 3)).astype(np.float64)
    y[-1] -= y.sum(axis=0)
    return (np.kron(np.eye(copies), y) + centre).astype(np.float32)


def cases():
    return {
        "illcond": (power_law(21, 256, 64), power_law(22, 256, 64, centre=0.05)),
        "illcond_deficient": (power_law(23, 20, 48), power_law(24, 30, 48, centre=-0.05)),
        "tie": (tied(25), tied(26, centre=0.5)),
    }


def main(argv):
    import mpmath as mp
    mp.mp.dps = DIGITS
    todo = cases()
    names = argv or list(C.CASES)
    table, bad = {}, 0
    for name in names:
        if name in O.CASES:
            g = O.load(name)
            model = C.distance(g["xa"], g["xb"])
            err = float(abs(mp.mpf(model["distance"]) - mp.mpf(str(g["mp_distance_digits"]))))
            unit = g["xa"].shape[1] * O.EPS * float(g["scale"])
            print(f"{name}: |Cholesky model - mp| {err:.3e} = {err / unit:.2f} d eps s (Jacobi model {O.MODEL_ERROR[name] / unit:.2f}), "
                  f"sweeps {model['sweeps']}, ranks {model['rank_a']}/{model['rank_b']}, file {g['model_ranks'].tolist()}")
            table[name] = err
            continue
        xa, xb = todo[name]
        n_a, n_b, d = xa.shape[0], xb.shape[0], xa.shape[1]
        want, s, ra, rb, rs = mp_distance(mp, xa, xb)
        ma, ca, _ = O.moments(xa)
        mb, cb, _ = O.moments(xb)
        chol = C.distance_from_moments(ma, ca, mb, cb)
        jac = O.distance_from_moments(ma, ca, mb, cb)
        err, jerr = float(abs(mp.mpf(chol["distance"]) - want)), float(abs(mp.mpf(jac["distance"]) - want))
        s = float(s)
        cut = d * O.EPS
        unit = cut * s
        near = [v for v in ra + rb + rs if cut / BAND <= v <= cut * BAND]
        conds = [1.0 / min(v for v in r if v > cut) for r in (ra, rb)]
        print(f"{name}: d {d}, n {n_a}/{n_b}, distance {float(want):.17g}, s {s:.6g}, condition {conds[0]:.2e} / {conds[1]:.2e}\n"
              f"  Cholesky model {err:.3e} = {err / unit:.2f} d eps s, ranks {chol['rank_a']}/{chol['rank_b']}, sweeps {chol['sweeps']}\n"
              f"  Jacobi model   {jerr:.3e} = {jerr / unit:.2f} d eps s, ranks {jac['rank_a']}/{jac['rank_b']}, sweeps {jac['sweeps']}")
        reasons = []
        if err > 4.0 * unit or jerr > 4.0 * unit:
            reasons.append(f"a model is more than 4 d eps s from the {DIGITS}-digit value")
        if near:
            reasons.append(f"relative eigen / singular values {near} within two decades of the rank threshold {cut:.3e}")
        if name == "illcond_deficient" and [chol["rank_a"], chol["rank_b"]] != [n_a - 1, n_b - 1]:
            reasons.append(f"the Cholesky model's ranks are not n - 1 = {n_a - 1}/{n_b - 1}")
        if [chol["rank_a"], chol["rank_b"]] != [jac["rank_a"], jac["rank_b"]]:
            reasons.append("the two models disagree on a rank")
        if reasons:
            print("  REFUSED: " + "; ".join(reasons))
            bad += 1
            continue
        table[name] = err
        np.savez(os.path.join(O.GOLDEN, f"frechet_chol_{name}.npz"), xa=xa, xb=xb, mu_a=ma, cov_a=ca, mu_b=mb, cov_b=cb,
                 mp_distance=np.float64(float(want)), mp_distance_digits=np.array(mp.nstr(want, 50)), scale=np.float64(s),
                 model_distance=np.float64(jac["distance"]), model_error=np.float64(jerr),
                 model_sqrt_trace=np.float64(jac["sqrt_trace"]), model_ranks=np.array([jac["rank_a"], jac["rank_b"]]),
                 model_counts_a=np.array(jac["counts"][0]), model_counts_b=np.array(jac["counts"][1]),
                 model_counts_m=np.array(jac["counts"][2]),
                 chol_model_distance=np.float64(chol["distance"]), chol_model_error=np.float64(err),
                 chol_model_sqrt_trace=np.float64(chol["sqrt_trace"]), chol_model_ranks=np.array([chol["rank_a"], chol["rank_b"]]),
                 chol_model_counts_m=np.array(chol["counts"]), chol_pivots_a=np.array(chol["pivots"][0]),
                 chol_pivots_b=np.array(chol["pivots"][1]))
    print("MODEL_ERROR = {")
    for name, err in table.items():
        print(f'    "{name}": {err!r},')
    print("}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
