#!/usr/bin/env python
"""The kernel distance on one MI355X (rcdms_amd/kid.py) against the host script it replaces.
  hip    n = 10 000 synthetic float32 features of d = 1280 (CLIP-bigG) and d = 2048 resident on the device, 100 subsets of
         1000 rows (kernel_distance: the draw and one upload of the indices, one launch of the tile kernel, one of the reduce,
         one read-back of 100 doubles), and a story-sized 300 rows with subset_size=None (subsets of all 300).
         The achieved float64 rate is printed twice: `useful`, the operations the definition needs — 2 d per kernel value,
         m^2 values of block xy and m (m - 1) / 2 distinct pairs of each symmetric block — and `issued`, what the 64 x 64 tiles
         put through the matrix pipe (whole tiles, k rounded up to 16, the upper-triangle tiles of the symmetric blocks), both over
         the time of the whole call, and again over the two launches alone (indices already resident: what the draw of 200
         permutations on the host and the transfers cost is the difference).  Next to them the issued rate of
         rcdm_feature_stats_update (FeatureStats.update of 1000 rows: 2 n d^2 over its time), the project's other float64
         matrix-pipe kernel, on the same box.
  host   what a user runs today on this box's CPU threads: the download of the features, then per subset three float64 numpy
         products, the cube and the sums.  Once per size.
  goldens  the kernel's error on tests/golden/kid_*.npz against the 60-digit values over the a-priori bound B, next to the model's.
Times are a host clock around calls that end in a device synchronise, median [min, max] of `--repeats` runs after one warm-up.
No pass / fail threshold.
usage: python tools/bench_kid.py [--repeats 3] [--sizes 1280 2048] [--rows 10000] [--subsets 100] [--subset-size 1000]
                                 [--story-rows 300] [--no-host]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(v, scale=1.0):
    return f"{statistics.median(v) * scale:.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"


def features(n, d, seed, offset):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, d, generator=g, device="cuda") + offset).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def flops(subsets, m, d):
    """(useful, issued) float64 operations of one call."""
    t = (m + 63) // 64
    useful = subsets * 2.0 * d * (m * m + m * (m - 1))
    issued = subsets * 2.0 * ((d + 15) // 16 * 16) * 64 * 64 * (t * t + t * (t + 1))
    return useful, issued


def goldens():
    from rcdms_amd.kid import polynomial_mmd
    from tests import kid_oracle as O
    from tests.test_kid_host import error_to_digits
    print("goldens: |kernel - mpmath| and |model - mpmath| of mmd^2 over the a-priori bound B (worst subset)")
    worst = 0.0
    for name in O.CASES:
        g = O.load(name)
        x, y = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["y"]).cuda()
        out = polynomial_mmd(x, y, g["ia"], g["ib"], int(g["degree"]), float(g["gamma"]), float(g["coef0"])).cpu().numpy()
        err = max(error_to_digits(out[s, 3], g["mp_digits"][s, 3]) / g["bound"][s] for s in range(out.shape[0]))
        worst = max(worst, err)
        print(f"  {name:14s} m {g['ia'].shape[1]:3d} d {g['x'].shape[1]:3d}  kernel {err:.2e}  model {np.max(g['model_error'] / g['bound']):.2e}")
    print(f"  worst kernel error: {worst:.2e} B")


def host_kid(xa, xb, ia, ib, gamma):
    t0 = time.perf_counter()
    ha, hb = xa.cpu().numpy().astype(np.float64), xb.cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()
    vals = []
    for a, b in zip(ia, ib):
        X, Y = ha[a], hb[b]
        m = len(a)
        kxx, kyy, kxy = (gamma * (X @ X.T) + 1.0) ** 3, (gamma * (Y @ Y.T) + 1.0) ** 3, (gamma * (X @ Y.T) + 1.0) ** 3
        vals.append((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2.0 * kxy.mean())
    t2 = time.perf_counter()
    return np.array(vals), t1 - t0, t2 - t1


def measure(label, xa, xb, subsets, m, repeats, host):
    from rcdms_amd import kid
    from rcdms_amd.kid import draw_subsets, kernel_distance
    d = xa.shape[1]
    run = lambda: kernel_distance(xa, xb, subsets=subsets, subset_size=m, seed=0)
    timed(run)
    t, res = zip(*[timed(run) for _ in range(repeats)])
    assert all(r.values == res[0].values for r in res), "two runs of one call differ"
    r = res[0]
    useful, issued = flops(r.subsets, r.subset_size, d)
    med = statistics.median(t)
    print(f"{label}: kernel_distance, {r.subsets} subsets of {r.subset_size}: {fmt(t, 1e3)} ms; float64 rate useful {useful / med / 1e12:.2f} TFLOP/s, "
          f"issued {issued / med / 1e12:.2f} TFLOP/s (whole call: draw, upload, 2 launches, read-back)", flush=True)
    print(f"  KID {r.mean:.9g} +- {r.std:.3g}")
    # the two launches alone: the same subsets with their indices already on the device, no draw, no read-back
    xr, yr = kid._rows(xa, "a"), kid._rows(xb, "b")
    both = torch.from_numpy(np.stack(draw_subsets(xa.shape[0], xb.shape[0], r.subsets, r.subset_size, 0))).cuda()
    dev = lambda: kid._mmd(xr, yr, both[0], both[1], 3, None, 1.0)
    timed(dev)
    td, outs = zip(*[timed(dev) for _ in range(repeats)])
    assert tuple(outs[0][:, 3].tolist()) == r.values
    medd = statistics.median(td)
    print(f"  the two launches alone (indices resident): {fmt(td, 1e3)} ms; float64 rate useful {useful / medd / 1e12:.2f} TFLOP/s, "
          f"issued {issued / medd / 1e12:.2f} TFLOP/s", flush=True)
    if host:
        ia, ib = draw_subsets(xa.shape[0], xb.shape[0], r.subsets, r.subset_size, 0)
        vals, t_down, t_math = host_kid(xa, xb, ia, ib, 1.0 / d)
        print(f"  host: download {t_down:.3f} s, {r.subsets} x (3 float64 products, cube, sums) {t_math:.3f} s, total {t_down + t_math:.3f} s "
              f"(one run, {torch.get_num_threads()} threads); KID {vals.mean():.9g}, worst |host - device| of a subset "
              f"{np.max(np.abs(vals - np.array(r.values))):.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1280, 2048])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset-size", type=int, default=1000)
    ap.add_argument("--story-rows", type=int, default=300)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    from rcdms_amd.frechet import FeatureStats
    print(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}")
    goldens()
    for d in args.sizes:
        xa, xb = features(args.rows, d, 1, 0.0), features(args.rows, d, 2, 0.01)
        measure(f"d {d}, n {args.rows}", xa, xb, args.subsets, min(args.subset_size, args.rows), args.repeats, not args.no_host)
        measure(f"d {d}, n {args.story_rows} (story-sized)", xa[:args.story_rows], xb[:args.story_rows], args.subsets, None, args.repeats,
                not args.no_host)
        st = FeatureStats(d, "cuda").update(xa[:1000])
        upd = [timed(lambda: st.update(xa[1000:2000]))[0] for _ in range(args.repeats + 1)][1:]
        print(f"d {d}: rcdm_feature_stats_update of 1000 rows {fmt(upd, 1e3)} ms: float64 rate issued "
              f"{2.0 * 1000 * d * d / statistics.median(upd) / 1e12:.2f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
