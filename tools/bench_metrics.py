#!/usr/bin/env python
"""Frame metrics of a story on one MI355X (rcdms_amd/metrics.py) against the host path they replace.
  hip    5 S pairs of 512^2 uint8 frames resident on the device -> SSIM / MSE / PSNR / MAE tensors on the device: one
         rcdm_frame_metrics call (two launches) + the few elementwise ops that derive PSNR; S = 1 and S = 4, both windows.
  host   the download of the same 5 frame pairs (2 x 3.9 MB) + float64 SSIM per frame on this box's CPU: scipy.ndimage's
         uniform_filter / gaussian_filter where scipy imports (what scikit-image runs), else the numpy restatement
         tests/ssim_oracle.py.  One story only; it is linear in the frame count.
Times are a host clock around calls that end in a device synchronise, median [min, max] of `--repeats` windows of `--steps`
calls after `--warmup` calls; the launch pair alone comes from device events.  Also prints the bytes the tile kernel must
fetch and the time that takes at 8 TB/s (the floor: the call is far above it, it is latency and fp64 bound).  No pass / fail
threshold.
usage: python tools/bench_metrics.py [--steps 50] [--warmup 10] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
SIDE = 512


def timed(fn, warmup, steps, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)


def kernel_ms(fn, warmup, steps):
    from rcdms_amd import hip
    for _ in range(warmup):
        fn()
    a, b = hip.Event(), hip.Event()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    return round(a.elapsed_ms(b) / steps, 5)


def host_ssim(a, b, window):
    """Mean SSIM of one uint8 pair in float64 on the CPU, the arithmetic scikit-image runs."""
    from tests import ssim_oracle as O
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return O.ssim(a, b, window)
    win = O.WIN[window]
    f = (lambda t: ndi.gaussian_filter(t, sigma=1.5, truncate=3.5)) if window == "gaussian" else (lambda t: ndi.uniform_filter(t, size=7))
    cn = win * win / (win * win - 1.0)
    pad = (win - 1) // 2
    out = []
    for c in range(3):
        x, y = a[:, :, c].astype(np.float64), b[:, :, c].astype(np.float64)
        ux, uy = f(x), f(y)
        vx, vy, vxy = cn * (f(x * x) - ux * ux), cn * (f(y * y) - uy * uy), cn * (f(x * y) - ux * uy)
        S = ((2 * ux * uy + O.C1) * (2 * vxy + O.C2)) / ((ux * ux + uy * uy + O.C1) * (vx + vy + O.C2))
        out.append(S[pad:-pad, pad:-pad].mean(dtype=np.float64))
    return float(np.mean(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import metrics as M
    assert torch.cuda.is_available(), "bench_metrics.py measures on a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    res = {"metric": "frame metrics of S stories (5 S pairs of 512^2 uint8 RGB frames)", "unit": "ms", "n_gpus": 1, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "data": "synthetic", "timing_format": "[median, min, max] over the repeats"}
    try:
        import scipy  # noqa: F401
        res["host_filter"] = "scipy.ndimage float64"
    except ImportError:
        res["host_filter"] = "numpy float64 (tests/ssim_oracle.py)"
    for S in (1, 4):
        n = 5 * S
        ga = rng.randint(0, 256, size=(n, SIDE, SIDE, 3)).astype(np.uint8)
        gb = np.clip(ga.astype(np.int16) + rng.randint(-30, 31, size=ga.shape), 0, 255).astype(np.uint8)
        da, db = torch.from_numpy(ga).to(dev), torch.from_numpy(gb).to(dev)
        fm = M.frame_metrics_for(n, SIDE, SIDE, dev)
        ssim = torch.empty(n, 3, dtype=torch.float64, device=dev)
        sse, sad = (torch.empty(n, 3, dtype=torch.int64, device=dev) for _ in range(2))
        case = res[f"S{S}"] = {"pairs": n, "kernel_bytes": 2 * ga.nbytes, "kernel_floor_ms": round(1e3 * 2 * ga.nbytes / HBM_BYTES_PER_S, 5)}
        for window in ("uniform", "gaussian"):
            case[f"hip_{window}_ms"] = timed(lambda: M.frame_metrics(da, db, window=window), a.warmup, a.steps, a.repeats)
            case[f"hip_{window}_launch_pair_ms"] = kernel_ms(lambda: fm.launch(da, db, ssim, sse, sad, window), a.warmup, a.steps)
        if S == 1:
            for window in ("uniform", "gaussian"):
                def host():
                    ha, hb = da.cpu().numpy(), db.cpu().numpy()
                    return [host_ssim(ha[i], hb[i], window) for i in range(n)]
                case[f"host_{window}_ms"] = timed(host, 1, 1, 3)
                got = M.frame_metrics(da, db, window=window).ssim.cpu().numpy()
                case[f"max_abs_diff_vs_host_{window}"] = float(np.abs(got - np.array(host())).max())
            case["bytes_over_pcie"] = {"hip": 0, "host": 2 * ga.nbytes}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
