#!/usr/bin/env python
"""The scores from logits on one MI355X (rcdms_amd/scores.py) against the host route they replace.
  hip    logits resident on the device (synthetic, seeded):
           a story        5 x 9 logits and labels: LabelCounts.update (two launches, no read-back) and update + result() (the one
                          read-back);
           a test set     11 040 x 9 logits and labels (the 2 208 PororoSV test stories of five frames): the same two;
                          11 040 x 1008 logits, 10 splits: inception_score (three launches, one read-back of 10 doubles).
         Each is timed twice: the whole Python call by a host clock around work that ends in a device synchronise, and the
         launches alone by device events around the C-ABI call with every buffer already allocated.
  host   what a user runs today on this box's CPU threads: the download of the logits, then scikit-learn (accuracy_score and the
         four f1_score averages) or numpy (softmax, split means, KL) — once per size, with the figures compared.
  goldens  the kernel's error on tests/golden/isc_*.npz against the 60-digit values over the a-priori bound B.
Median [min, max] of `--repeats` runs after one warm-up.  A story's calls take microseconds: those rows measure launch and
synchronise overhead, which is the point of keeping the logits on the device, not a kernel rate.  No pass / fail threshold.
usage: python tools/bench_scores.py [--repeats 20] [--rows 11040] [--no-host]"""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def events(fn, repeats):
    """Seconds of fn()'s device work by events, `repeats` times after a warm-up."""
    fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def goldens():
    from rcdms_amd.scores import inception_score
    from tests import scores_oracle as O
    from tests.test_scores_host import error_to_digits
    print("goldens: |kernel - mpmath| of KL over the a-priori bound B (worst split), by class count")
    worst = {}
    for name, (C, n, splits, variant) in O.ISC_CASES.items():
        g = O.load_isc(name)
        z = torch.from_numpy(g["logits"]).cuda()
        r = inception_score(z.half() if variant == "f16" else z, splits=splits, order=g["order"])
        err = max(error_to_digits(r.kl[k], g["kl_digits"][k]) / g["bound"][k] for k in range(splits))
        worst[C] = max(worst.get(C, 0.0), err)
    for C in sorted(worst):
        print(f"  C {C:4d}  kernel {worst[C]:.2e} B")
    print(f"  worst kernel error: {max(worst.values()):.2e} B (exp / log assumed within {O.ULPS:g} ulp)")


def labels_case(label, n, C, repeats, host):
    from rcdms_amd import hip
    from rcdms_amd.scores import LabelCounts
    g = torch.Generator(device="cuda").manual_seed(n + C)
    z = torch.randn(n, C, generator=g, device="cuda")
    y = (torch.rand(n, C, generator=g, device="cuda") < 0.3).to(torch.uint8)
    lc = LabelCounts(C, "cuda")
    upd = [timed(lambda: lc.clear().update(z, y))[0] for _ in range(repeats + 1)][1:]
    res = [timed(lambda: lc.clear().update(z, y).result())[0] for _ in range(repeats + 1)][1:]
    r = lc.result()
    desc = hip.LabelDesc(C, C, n, C, hip.FSTATS_F32, 0)
    need = hip.label_counts_workspace_bytes(desc)
    ws, st = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.zeros(hip.label_state_len(C), dtype=torch.int64, device="cuda")
    dev = events(lambda: hip.label_counts(desc, z.data_ptr(), y.data_ptr(), 0, st.data_ptr(), ws.data_ptr(), need), repeats)
    print(f"{label}: {n} x {C} logits and labels: update {fmt(upd, 1e6)} us, update + result() {fmt(res, 1e6)} us (host clock, whole call); "
          f"the two launches alone {fmt(dev, 1e6)} us (device events)", flush=True)
    print(f"  Frm-Acc {r.frame_accuracy:.6f}  F1 micro {r.f1_micro:.6f} macro {r.f1_macro:.6f} weighted {r.f1_weighted:.6f} samples {r.f1_samples:.6f}")
    if host:
        from sklearn import metrics
        t0 = time.perf_counter()
        hz, hy = z.cpu().numpy(), y.cpu().numpy()
        t1 = time.perf_counter()
        pred = (hz > 0).astype(np.int64)
        sk = [metrics.accuracy_score(hy, pred)] + [metrics.f1_score(hy, pred, average=a, zero_division=0)
                                                   for a in ("micro", "macro", "weighted", "samples")]
        t2 = time.perf_counter()
        ours = [r.frame_accuracy, r.f1_micro, r.f1_macro, r.f1_weighted, r.f1_samples]
        print(f"  host: download {(t1 - t0) * 1e6:.0f} us, scikit-learn (accuracy_score, four f1_score) {(t2 - t1) * 1e6:.0f} us, total "
              f"{(t2 - t0) * 1e6:.0f} us (one run, {torch.get_num_threads()} threads); worst |host - device| {max(abs(a - b) for a, b in zip(sk, ours)):.3e}",
              flush=True)


def isc_case(label, n, C, splits, repeats, host):
    from rcdms_amd import hip
    from rcdms_amd.scores import inception_score
    g = torch.Generator(device="cuda").manual_seed(n + C)
    z = torch.randn(n, C, generator=g, device="cuda") * 3.0
    run = lambda: inception_score(z, splits=splits)
    timed(run)
    t, res = zip(*[timed(run) for _ in range(repeats)])
    assert all(r.kl == res[0].kl for r in res), "two runs of one call differ"
    r = res[0]
    desc = hip.IscDesc(C, n, C, splits, hip.FSTATS_F32, 0, 0)
    need = hip.inception_score_workspace_bytes(desc)
    ws, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.empty(splits, dtype=torch.float64, device="cuda")
    dev = events(lambda: hip.inception_score(desc, z.data_ptr(), 0, out.data_ptr(), 0, ws.data_ptr(), need), repeats)
    assert tuple(out.tolist()) == r.kl
    print(f"{label}: {n} x {C} logits, {splits} splits: inception_score {fmt(t, 1e3)} ms (host clock, whole call); the three launches alone "
          f"{fmt(dev, 1e3)} ms (device events); {2 * n * C / statistics.median(dev) / 1e9:.2f} G exp/s (two per logit, plus one per chunked read)",
          flush=True)
    print(f"  IS {r.mean:.9g} +- {r.std:.3g}")
    if host:
        t0 = time.perf_counter()
        hz = z.cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()
        lp = hz - hz.max(axis=1, keepdims=True)
        lp -= np.log(np.exp(lp).sum(axis=1, keepdims=True))
        p = np.exp(lp)
        kl = []
        for k in range(splits):
            b0, b1 = k * n // splits, (k + 1) * n // splits
            pb = p[b0:b1].mean(axis=0, keepdims=True)
            kl.append((p[b0:b1] * (lp[b0:b1] - np.log(pb))).sum(axis=1).mean())
        t2 = time.perf_counter()
        print(f"  host: download {(t1 - t0) * 1e3:.3f} ms, numpy float64 (softmax, split means, KL) {(t2 - t1) * 1e3:.3f} ms, total "
              f"{(t2 - t0) * 1e3:.3f} ms (one run, {torch.get_num_threads()} threads); worst |host - device| of a split's KL "
              f"{np.max(np.abs(np.array(kl) - np.array(r.kl))):.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rows", type=int, default=11040)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}")
    goldens()
    labels_case("a story", 5, 9, args.repeats, not args.no_host)
    labels_case("a test set", args.rows, 9, args.repeats, not args.no_host)
    isc_case("a test set", args.rows, 1008, 10, args.repeats, not args.no_host)


if __name__ == "__main__":
    main()
