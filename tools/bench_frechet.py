#!/usr/bin/env python
"""Feature statistics and the Fréchet distance on one MI355X (rcdms_amd/frechet.py) against the host script they replace.
  hip    n = 10 000 synthetic float32 features of d = 1280 (CLIP-bigG) and d = 2048 resident on the device:
           update   FeatureStats.update per 1000 rows (two launches: column sums, the float64 MFMA outer product);
           cold     one frechet_distance with both factors to compute (three Jacobi runs);
           cached   one with the reference factor cached (two runs).
         Also the sweeps of every run, and the launches they amount to: a sweep is rows + 1 launches (norms, threshold, one per
         round), a factor step 4 more, the singular-value sum 2, the TN product 1.
  host   the download of the same features + numpy.cov + scipy.linalg.sqrtm of the d x d product on this box's CPU (the
         threads the environment allows), once per size: what an FID script does.  Skipped where scipy does not import.
  goldens  the kernel's error on tests/golden/frechet_*.npz against the 60-digit values, next to the model's and the budget.
Two kinds of synthetic features, because the sweep count of one-sided Jacobi grows with the logarithm of the covariance's
condition number: "power" (column k of unit normals scaled by k^-1/2, then mixed by a random Gaussian matrix: condition
number 1e8 at d = 256 and more above) and "white" (unit normals through the mixing alone; a square Gaussian matrix is itself
poorly conditioned, more so as d grows, so this set is milder, not white).  A run that does not stop within 30 sweeps is
reported as such, not timed.
--factor picks the way the factors are formed (rcdms_amd/frechet.py): jacobi (the default route, the description above), cholesky
(rcdm_cholesky_pivoted_f64: 1 + 2 d + (d - 1) / nb launches per factor, no sweeps, and the singular-value run over the
rank_b x rank_a block only) or both, one after the other in this process on the same statistics.  Per route: one factorisation alone,
the distance cold and with the reference factor cached, launches, ranks and the sweeps over Fb^T Fa.  --panels times the one
factorisation at other panel widths through the C entry.
Times are a host clock around calls that end in a device synchronise, median [min, max] of `--repeats` runs.  No pass / fail
threshold.
usage: python tools/bench_frechet.py [--repeats 3] [--sizes 1280 2048] [--rows 10000] [--spectra power white] [--no-host]
                                     [--factor jacobi|cholesky|both] [--panels 16 32 64 128]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1000


def fmt(v):
    if not v:
        return "not timed (--rows is one chunk)"
    return f"{statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]"


def features(n, d, seed, offset, spectrum):
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(n, d, generator=g, device="cuda")
    if spectrum == "power":
        z = z * torch.arange(1, d + 1, device="cuda").float().rsqrt()
    mix = torch.randn(d, d, generator=g, device="cuda") / d ** 0.5
    return (z @ mix + offset).contiguous()


def launches(d, sweeps):
    rows = d + (d & 1)
    return sum(s * (rows + 1) for s in sweeps) + 4 * sum(1 for s in sweeps[:2] if s) + 2 + 1 + 1


def launches_cholesky(d, factors, block, sweeps_m, nb):
    per_factor = 1 + 2 * d + (d - 1) // nb
    return factors * per_factor + (1 + sweeps_m * (block[0] + 1) + 2 if block else 0) + 1


def drop_factors(*stats):
    for st in stats:
        st._factor = st._factor_chol = None


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def panel_times(hip, a, panels, repeats):
    """One factorisation of a's covariance through the C entry at each panel width."""
    d, cov = a.d, a.cov()
    f = torch.empty(d, d, dtype=torch.float64, device="cuda")
    rank = torch.zeros(1, dtype=torch.int32, device="cuda")
    for nb in panels:
        desc = hip.CholeskyDesc(d, d, d, nb)
        ws = torch.empty(hip.cholesky_workspace_bytes(desc), dtype=torch.uint8, device="cuda")
        run = lambda: hip.cholesky_pivoted_f64(desc, cov.data_ptr(), f.data_ptr(), rank.data_ptr(), ws.data_ptr(), ws.numel())
        timed(run)
        t = [timed(run)[0] for _ in range(repeats)]
        print(f"  panel width {nb:3d}: one factorisation {fmt(t)} s, rank {int(rank.item())}, {1 + 2 * d + (d - 1) // nb} launches", flush=True)


def goldens():
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    from tests import frechet_oracle as O
    print("goldens: |kernel - mpmath|, |model - mpmath| and the test budget, in units of d 2^-52 s")
    worst = 0.0
    for name in O.CASES:
        g = O.load(name)
        d, s = g["xa"].shape[1], float(g["scale"])
        a = FeatureStats(d, "cuda").update(torch.from_numpy(g["xa"]).cuda())
        b = FeatureStats(d, "cuda").update(torch.from_numpy(g["xb"]).cuda())
        r = frechet_distance(a, b)
        unit = d * O.EPS * s
        err = abs(r.distance - float(g["mp_distance"]))
        worst = max(worst, err / unit)
        print(f"  {name:12s} d {d:3d}  kernel {err / unit:6.2f}  model {O.MODEL_ERROR[name] / unit:6.2f}  budget "
              f"{O.budget(d, s, O.MODEL_ERROR[name]) / unit:6.2f}  sweeps {r.sweeps}")
    print(f"  worst kernel error: {worst:.2f} d 2^-52 s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1280, 2048])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--spectra", nargs="+", default=["power", "white"], choices=["power", "white"])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--factor", default="jacobi", choices=["jacobi", "cholesky", "both"])
    ap.add_argument("--panels", type=int, nargs="*", default=[], choices=[16, 32, 64, 128])
    args = ap.parse_args()
    from rcdms_amd import hip
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    print(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}")
    goldens()
    for d, spectrum in ((d, sp) for d in args.sizes for sp in args.spectra):
        xa, xb = features(args.rows, d, 1, 0.0, spectrum), features(args.rows, d, 2, 0.01, spectrum)
        torch.cuda.synchronize()
        upd = []
        for rep in range(args.repeats + 1):
            a = FeatureStats(d, "cuda")
            for r0 in range(0, args.rows, CHUNK):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.update(xa[r0:r0 + CHUNK])
                torch.cuda.synchronize()
                if rep and r0:                       # the first call of a size and the shift's own reduction are not the update
                    upd.append(1e3 * (time.perf_counter() - t0))
        b = FeatureStats(d, "cuda").update(xb)
        print(f"d {d}, n {args.rows}, {spectrum} spectrum: update of {CHUNK} rows {fmt(upd)} ms", flush=True)
        res, by_route = None, {}
        if args.panels:
            panel_times(hip, a, args.panels, args.repeats)
        for route in (["jacobi", "cholesky"] if args.factor == "both" else [args.factor]):
            cold, cached, one = [], [], []
            try:
                for rep in range(args.repeats):
                    drop_factors(a, b)
                    one.append(timed(lambda: a.factor(route))[0])
                    drop_factors(a, b)
                    t, res = timed(lambda: frechet_distance(a, b, factor=route))
                    cold.append(t)
                    print(f"  {route}: cold run {rep}: {cold[-1]:.3f} s, sweeps {res.sweeps}", flush=True)
                    drop_factors(a)
                    t, res2 = timed(lambda: frechet_distance(a, b, factor=route))
                    cached.append(t)
                    assert res2.distance == res.distance and res2.sweeps[1] == 0
                sw = res.sweeps
                by_route[route] = res
                print(f"  {route}: distance {res.distance:.12g} (mean term {res.mean_term:.6g}, ranks {res.rank_a}/{res.rank_b}), "
                      f"sweeps {sw}, block {res.block}")
                if route == "jacobi":
                    print(f"  jacobi: one factorisation {fmt(one)} s, {sw[0] * (d + (d & 1) + 1) + 4} launches")
                    print(f"  jacobi: cold   (3 Jacobi runs) {fmt(cold)} s, {launches(d, sw)} launches")
                    print(f"  jacobi: cached (2 Jacobi runs) {fmt(cached)} s, {launches(d, (sw[0], 0, sw[2]))} launches", flush=True)
                else:
                    nb = hip.CHOLESKY_NB
                    print(f"  cholesky: one factorisation {fmt(one)} s, {1 + 2 * d + (d - 1) // nb} launches (panels of {nb})")
                    print(f"  cholesky: cold   (2 factorisations, 1 Jacobi run) {fmt(cold)} s, {launches_cholesky(d, 2, res.block, sw[2], nb)} launches")
                    print(f"  cholesky: cached (1 factorisation, 1 Jacobi run)  {fmt(cached)} s, {launches_cholesky(d, 1, res.block, sw[2], nb)} launches",
                          flush=True)
            except hip.RcdmError as e:
                print(f"  {route}: NOT MEASURED: {e}", flush=True)
        if len(by_route) == 2:
            rj, rc = by_route["jacobi"], by_route["cholesky"]
            print(f"  |cholesky - jacobi| {abs(rc.distance - rj.distance):.3e} "
                  f"({abs(rc.distance - rj.distance) / (rj.trace_a + rj.trace_b + rj.mean_term):.1e} s)", flush=True)
        if args.no_host:
            continue
        try:
            from scipy import linalg
        except ImportError:
            print("  host: scipy does not import here, not measured")
            continue
        t0 = time.perf_counter()
        ha, hb = xa.cpu().numpy().astype(np.float64), xb.cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()
        mu_a, mu_b, ca, cb = ha.mean(0), hb.mean(0), np.cov(ha, rowvar=False), np.cov(hb, rowvar=False)
        t2 = time.perf_counter()
        root = linalg.sqrtm(ca @ cb)
        t3 = time.perf_counter()
        fid = float(((mu_a - mu_b) ** 2).sum() + np.trace(ca) + np.trace(cb) - 2.0 * np.trace(root).real)
        print(f"  host: download {t1 - t0:.3f} s, numpy.cov x 2 {t2 - t1:.3f} s, scipy sqrtm {t3 - t2:.3f} s, total {t3 - t0:.3f} s (one run)")
        if res is not None:
            print(f"  host value {fid:.12g}, difference to the device {abs(fid - res.distance):.3e} "
                  f"({abs(fid - res.distance) / (res.trace_a + res.trace_b + res.mean_term):.1e} s)", flush=True)


if __name__ == "__main__":
    main()
