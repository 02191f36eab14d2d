#!/usr/bin/env python
"""The manifold figures on one MI355X (rcdms_amd/prdc.py) against the host script they replace.
  hip    n synthetic float32 rows of d = 1280 and d = 2048 resident on the device, nearest_k = 5, at n = 10 000 and a story-sized
         n = 300:
           whole call     manifold_metrics on two tensors: two radius sweeps, the count sweep, one read-back of four int64;
           launches       the same three entries between device events, no read-back — each sweep on its own and their sum;
           cached         manifold_metrics with the reference set in a FeatureBank whose radii are already there: one radius sweep;
           rate           the float64 rate of the three distance sweeps, `useful` — 2 d per distance, n (n - 1) / 2 distinct pairs
                          per radius sweep and nx ny pairs of the count sweep — and `issued`, what the 64 x 64 tiles put through
                          the matrix pipe (whole tiles, k rounded up to 16, every tile of a set against itself: the symmetry is
                          not used), over the launches' time.
         First yardstick, in the same process: the issued rate of rcdm_poly_mmd on one subset of all n rows of the same two sets
         (the same tile product with a summing epilogue), and the ratio of the two issued rates.
  host   what a user runs today on this box's CPU threads, the route of the prdc package: the download,
         sklearn.metrics.pairwise_distances (Euclidean, float64, n_jobs = the threads), numpy.partition for the radii and the
         comparisons.  Once per size, with the equality of the four numerators.
Times are a host clock around calls that end in a device synchronise (device events for the launches), median [min, max] of
`--repeats` runs after one warm-up.  No pass / fail threshold.
usage: python tools/bench_prdc.py [--repeats 3] [--sizes 1280 2048] [--rows 10000 300] [--k 5] [--no-host] [--out profiles/prdc.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = None


def say(line):
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


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


def sweeps(x, y, k):
    """The three entries between device events -> (seconds of radii x, radii y, counts)."""
    from rcdms_amd import prdc
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    rx = prdc._radii2(x, k)
    ev[1].record()
    ry = prdc._radii2(y, k)
    ev[2].record()
    prdc._counts(x, y, rx, ry)
    ev[3].record()
    torch.cuda.synchronize()
    return tuple(ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(3))


def flops(nx, ny, d):
    """(useful, issued) float64 operations of the three sweeps."""
    tx, ty, dk = (nx + 63) // 64, (ny + 63) // 64, (d + 15) // 16 * 16
    useful = 2.0 * d * (nx * (nx - 1) / 2 + ny * (ny - 1) / 2 + nx * ny)
    issued = 2.0 * dk * 64 * 64 * (tx * tx + ty * ty + tx * ty)
    return useful, issued


def host_prdc(x, y, k, jobs):
    """The route of the prdc package: Euclidean distances (not squared) from sklearn on `jobs` threads, numpy.partition for the
    radii, the comparisons — closed here, as on the device."""
    from sklearn.metrics import pairwise_distances
    t0 = time.perf_counter()
    hx, hy = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()

    def radii(z):
        D = pairwise_distances(z, metric="euclidean", n_jobs=jobs)
        return np.partition(D, k, axis=1)[:, k]                  # the row itself is the smallest entry: the k-th other is at index k

    rx, ry = radii(hx), radii(hy)
    D = pairwise_distances(hx, hy, metric="euclidean", n_jobs=jobs)
    fake_count = (D <= rx[:, None]).sum(axis=0)
    counts = (int((fake_count > 0).sum()), int((D <= ry[None, :]).any(axis=1).sum()), int(fake_count.sum()), int((D.min(axis=1) <= rx).sum()))
    t2 = time.perf_counter()
    return counts, t1 - t0, t2 - t1


def measure(n, d, k, repeats, host):
    from rcdms_amd import kid
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.prdc import manifold_metrics
    x, y = features(n, d, 1, 0.0), features(n, d, 2, 0.01)
    run = lambda: manifold_metrics(x, y, nearest_k=k)
    timed(run)
    t, res = zip(*[timed(run) for _ in range(repeats)])
    assert all(r.counts == res[0].counts for r in res), "two runs of one call differ"
    r = res[0]
    say(f"d {d}, n {n}, k {k}: manifold_metrics {fmt(t, 1e3)} ms (whole call: 2 radius sweeps, count sweep, read-back); precision {r.precision:.4f} "
        f"recall {r.recall:.4f} density {r.density:.4f} coverage {r.coverage:.4f}, numerators {r.counts}")
    sweeps(x, y, k)
    parts = [sweeps(x, y, k) for _ in range(repeats)]
    total = [sum(p) for p in parts]
    useful, issued = flops(n, n, d)
    med = statistics.median(total)
    say(f"  the launches alone (device events): radii real {fmt([p[0] for p in parts], 1e3)} ms, radii generated {fmt([p[1] for p in parts], 1e3)} ms, "
        f"counts {fmt([p[2] for p in parts], 1e3)} ms, sum {fmt(total, 1e3)} ms; float64 rate useful {useful / med / 1e12:.2f} TFLOP/s, "
        f"issued {issued / med / 1e12:.2f} TFLOP/s")
    bank = FeatureBank(d, "cuda").append(x)
    bank.radii2(k)
    cached = lambda: manifold_metrics(bank, y, nearest_k=k)
    timed(cached)
    tc, rc = zip(*[timed(cached) for _ in range(repeats)])
    assert rc[0].counts == r.counts
    say(f"  with the reference radii cached (FeatureBank.radii2): {fmt(tc, 1e3)} ms")
    # first yardstick: the same tile product with KID's summing epilogue, one subset of all n rows
    xr, yr = kid._rows(x, "a"), kid._rows(y, "b")
    mmd = lambda: kid._mmd(xr, yr, None, None, 3, None, 1.0)
    timed(mmd)
    tm = [timed(mmd)[0] for _ in range(repeats)]
    tt = (n + 63) // 64
    mmd_issued = 2.0 * ((d + 15) // 16 * 16) * 64 * 64 * (tt * tt + tt * (tt + 1))
    mmd_rate = mmd_issued / statistics.median(tm)
    say(f"  rcdm_poly_mmd, one subset of {n} rows: {fmt(tm, 1e3)} ms, issued {mmd_rate / 1e12:.2f} TFLOP/s; issued rate of the three sweeps / "
        f"this: {issued / med / mmd_rate:.2f}")
    if host:
        counts, t_down, t_math = host_prdc(x, y, k, torch.get_num_threads())
        say(f"  host: download {t_down:.3f} s, 3 x pairwise_distances + partition + comparisons {t_math:.3f} s, total {t_down + t_math:.3f} s "
            f"(one run, {torch.get_num_threads()} threads); numerators {counts}, equal to the device's: {counts == r.counts}")


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1280, 2048])
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 300])
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        OUT = open(args.out, "w")
    say(f"# tools/bench_prdc.py --repeats {args.repeats}, one device; see README, \"Manifold figures\"")
    say(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}")
    for d in args.sizes:
        for n in args.rows:
            measure(n, d, args.k, args.repeats, not args.no_host)


if __name__ == "__main__":
    main()
