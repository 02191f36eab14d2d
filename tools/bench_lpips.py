#!/usr/bin/env python
"""LPIPS on one MI355X (rcdms_amd/lpips.py) against the same networks in torch on the same device, and the distance head
against its own byte floor.
  hip    P = 5 and 50 pairs of uint8 512 x 512 frames resident on the device -> (P, 5) float64 distances: the two input-row
         launches, every conv / pool launch of the plan and one rcdm_lpips_head call per tap; chunks of `--batch` pairs.
  torch  tests/lpips_oracle.py's fp32 tower (F.conv2d / F.max_pool2d, the direct 11 x 11 stride-4 stem) with the weights on
         the device, and a written-out torch head (normalise, difference, lin, spatial mean), same process, same chunks.
  head   rcdm_lpips_head alone on random post-ReLU f16 features of every tap's shape at P pairs, `--head-launches` calls between
         two device events.  Floor: 2 P h w C 2 bytes (every feature row once) at 6.3 TB/s, the rate a float4 copy reaches on
         this part (8.0 TB/s on paper); printed: microseconds per call, bytes / time, the fraction of the floor reached.  A tap
         whose rows fit the 256 MiB Infinity Cache is marked: its rate is not an HBM rate.
Synthetic weights (tests/lpips_oracle.synthetic_state_dict); the frames are random bytes.  Call times are a host clock around
calls that end in a device synchronise: a timed window is max(1, 100 / P) calls back to back, the figure its time per call;
median [min, max] of `--repeats` windows after one warm-up of every shape, the hip and torch windows alternating.
No pass / fail threshold.
usage: python tools/bench_lpips.py [--repeats 3] [--pairs 5 50] [--side 512] [--batch 8] [--nets vgg alex] [--no-torch]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_RATE = 6.3e12
INFINITY_CACHE = 256 << 20


def fmt(v, scale=1.0):
    return f"{statistics.median(v) * scale:.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_head(x, y, lin):
    """x, y fp32 NCHW taps, lin (C,) -> (N,) fp32: the head written out in torch, as the lpips package does."""
    nx = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = y / (y.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((nx - ny).pow(2) * lin.view(1, -1, 1, 1)).sum(1).mean((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, nargs="+", default=[5, 50])
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nets", nargs="+", default=["vgg", "alex"])
    ap.add_argument("--head-launches", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lpips.py measures on the GPU: there is no device here"
    from rcdms_amd import hip
    from rcdms_amd import lpips as L
    from tests import lpips_oracle as O
    print(f"{torch.cuda.get_device_name(0)}, frames {a.side} x {a.side}, chunks of {a.batch} pairs, {a.repeats} windows per path, "
          f"alternating, after one warm-up; ms per call")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in a.nets:
        sd = O.synthetic_state_dict(name, 0)
        net = L.LpipsNet(sd, name, device="cuda", batch=a.batch)
        dsd = {k: v.cuda() for k, v in sd.items()}
        lins = [dsd[f"lin{t}.model.1.weight"].reshape(-1) for t in range(5)]
        shift = torch.tensor(L.SHIFT, device="cuda").view(1, 3, 1, 1)
        scale = torch.tensor(L.SCALE, device="cuda").view(1, 3, 1, 1)

        def torch_lpips(fa, fb):
            out = []
            with torch.no_grad():
                for i in range(0, fa.shape[0], a.batch):
                    x = torch.cat([fa[i:i + a.batch], fb[i:i + a.batch]]).permute(0, 3, 1, 2).float() / 255 * 2 - 1
                    taps = O.tower(dsd, name, (x - shift) / scale)
                    n = taps[0].shape[0] // 2
                    out.append(torch.stack([torch_head(t[:n], t[n:], w) for t, w in zip(taps, lins)], 1))
            return torch.cat(out)

        for P in a.pairs:
            fa = torch.randint(0, 256, (P, a.side, a.side, 3), generator=g, device="cuda", dtype=torch.uint8)
            fb = torch.randint(0, 256, (P, a.side, a.side, 3), generator=g, device="cuda", dtype=torch.uint8)
            calls = max(1, 100 // P)
            window = lambda fn: [fn() for _ in range(calls)][-1]
            _, (_, got) = timed(lambda: net(fa, fb, return_layers=True))             # warm-up: plans, code objects
            if not a.no_torch:
                _, want = timed(lambda: torch_lpips(fa, fb))
            t, tt = [], []
            for _ in range(a.repeats):                                               # the two paths alternate
                t.append(timed(lambda: window(lambda: net(fa, fb)))[0] / calls)
                if not a.no_torch:
                    tt.append(timed(lambda: window(lambda: torch_lpips(fa, fb)))[0] / calls)
            print(f"{name:4s} P = {P:3d}  hip    {fmt(t, 1e3)} ms   {P / statistics.median(t):8.1f} pairs/s")
            if not a.no_torch:
                err = float((got / want.double() - 1).abs().max())
                print(f"               torch  {fmt(tt, 1e3)} ms   {P / statistics.median(tt):8.1f} pairs/s   fp32; largest relative "
                      f"difference of a tap distance, hip against torch {err:.2e}")
            # the head alone, per tap, by device events
            plan = net._plan(min(P, a.batch), a.side, a.side)
            for k, x in enumerate(plan.taps):
                hw, rows = x.h * x.w, 2 * P * x.h * x.w
                feats = torch.randn(rows, x.c, generator=g, device="cuda", dtype=torch.float16).clamp_(min=0)
                d = hip.LpipsHeadDesc(x.c, x.c, P, x.h, x.w, x.c, 0, 0)
                ws = torch.empty(hip.lpips_head_workspace_bytes(d), dtype=torch.uint8, device="cuda")
                out = torch.empty(P, dtype=torch.float64, device="cuda")
                launch = lambda: hip.lpips_head(d, feats.data_ptr(), feats.data_ptr() + 2 * P * hw * x.c, lins[k].data_ptr(),
                                                out.data_ptr(), ws.data_ptr(), ws.numel())
                launch()
                us = []
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.head_launches):
                        launch()
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / a.head_launches)
                nbytes = rows * x.c * 2
                med = statistics.median(us) * 1e-6
                note = "  (rows fit the Infinity Cache: not an HBM rate)" if nbytes <= INFINITY_CACHE else ""
                print(f"               head tap {k} {x.h:3d} x {x.w:3d} x {x.c:3d}: {fmt(us)} us per call (two launches), {nbytes / 1e6:9.1f} MB, "
                      f"{nbytes / med / 1e12:5.2f} TB/s, {nbytes / HBM_RATE / med:5.1%} of the byte floor{note}")
                del feats


if __name__ == "__main__":
    main()
