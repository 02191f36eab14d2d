#!/usr/bin/env python
"""Inception-v3 pool features on one MI355X (rcdms_amd/inception.py) against the same network in torch on the same device.
  hip    N = 5, 50 and 500 uint8 frames of 512 x 512 resident on the device -> (N, 2048) features: the bilinear launch, every
         conv / pool launch of the plan, the global average; chunks of `--batch` frames (default 50).  Printed: images per
         second and two f16 rates over the time of the whole call — `useful`, 2 M K c_out of every conv at its real c_in, and
         `issued`, what the 64 x 64 x 32 tiles of rcdm_conv2d put through the matrix pipe (whole tiles, K rounded up to the
         k-step, the stem's 3 channels padded to 8).
  torch  tests/inception_oracle.py's fp32 network (F.conv2d, unfolded BatchNorm, ReLU) with the weights on the device, behind
         torch's own F.interpolate, in the same process, in the same chunks.
Synthetic weights (tests/inception_oracle.synthetic_state_dict); the frames are random bytes.  Times are a host clock around calls
that end in a device synchronise: a timed window is max(1, min(50, 1000 / N)) calls back to back (at least 1000 frames), the figure
its time per call; median [min, max] of `--repeats` windows after one warm-up of every shape, the hip and torch windows alternating.
No pass / fail threshold.
usage: python tools/bench_inception.py [--repeats 3] [--frames 5 50 500] [--side 512] [--batch 50] [--variant fid] [--no-torch]"""
import argparse
import os
import statistics
import sys
import time

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


# side of the activation every conv of a stage reads (a block's convs all keep the side but its stride-2 ones)
STEM_IN = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 73}
BLOCK_IN_SIDE = {"Mixed_5b": 35, "Mixed_5c": 35, "Mixed_5d": 35, "Mixed_6a": 35, "Mixed_6b": 17, "Mixed_6c": 17, "Mixed_6d": 17,
                 "Mixed_6e": 17, "Mixed_7a": 17, "Mixed_7b": 8, "Mixed_7c": 8}


def conv_work(n):
    """(useful, issued) f16 operations of the convs of one forward of n frames, from the layer table and the sides alone."""
    from rcdms_amd.inception import LAYERS
    useful = issued = 0.0
    for name, (cin, cout, (kh, kw), (sh, sw), (ph, pw)) in LAYERS.items():
        side = STEM_IN.get(name, BLOCK_IN_SIDE.get(name.split(".")[0]))
        ho, wo = (side + 2 * ph - kh) // sh + 1, (side + 2 * pw - kw) // sw + 1
        M = n * ho * wo
        K = kh * kw * ((cin + 7) // 8 * 8)                      # the kernel's c_in: the stem's 3 channels are padded to 8
        useful += 2.0 * M * kh * kw * cin * cout
        issued += 2.0 * ((M + 63) // 64 * 64) * ((cout + 63) // 64 * 64) * ((K + 31) // 32 * 32)
    return useful, issued


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[5, 50, 500])
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--variant", default="fid")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inception.py measures on the GPU: there is no device here"
    from rcdms_amd.inception import InceptionV3Features
    from tests import inception_oracle as O
    sd = O.synthetic_state_dict(0)
    net = InceptionV3Features(sd, variant=a.variant, device="cuda", batch=a.batch)
    ref = O.Net({k: v.cuda() for k, v in sd.items()}, a.variant)

    def torch_features(frames):
        out = []
        with torch.no_grad():
            for i in range(0, frames.shape[0], a.batch):
                x = frames[i:i + a.batch].permute(0, 3, 1, 2).float() / 255
                x = torch.nn.functional.interpolate(x, (299, 299), mode="bilinear", align_corners=False) * 2 - 1
                out.append(ref.features(x))
        return torch.cat(out)

    print(f"{torch.cuda.get_device_name(0)}, variant {a.variant}, frames {a.side} x {a.side}, chunks of {a.batch}, "
          f"{a.repeats} windows per path, alternating, after one warm-up; ms per call")
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in a.frames:
        frames = torch.randint(0, 256, (n, a.side, a.side, 3), generator=g, device="cuda", dtype=torch.uint8)
        useful = issued = 0.0
        work = {}
        for i in range(0, n, a.batch):
            m = min(a.batch, n - i)
            if m not in work:
                work[m] = conv_work(m)
            useful, issued = useful + work[m][0], issued + work[m][1]
        calls = max(1, min(50, 1000 // n))                                          # calls per timed window: >= 1000 frames
        window = lambda fn: [fn() for _ in range(calls)][-1]
        _, feats = timed(lambda: net(frames))                                       # warm-up: plans, code objects
        if not a.no_torch:
            _, want = timed(lambda: torch_features(frames))
        t, tt = [], []
        for _ in range(a.repeats):                                                  # the two paths alternate
            t.append(timed(lambda: window(lambda: net(frames)))[0] / calls)
            if not a.no_torch:
                tt.append(timed(lambda: window(lambda: torch_features(frames)))[0] / calls)
        med = statistics.median(t)
        print(f"N = {n:4d}  hip    {fmt(t, 1e3)} ms   {n / med:9.1f} images/s   useful {useful / med / 1e12:7.2f}  "
              f"issued {issued / med / 1e12:7.2f} Tflop/s f16")
        if not a.no_torch:
            err = float(((feats.double() - want.double()).pow(2).mean() / want.double().pow(2).mean()).sqrt())
            print(f"          torch  {fmt(tt, 1e3)} ms   {n / statistics.median(tt):9.1f} images/s   fp32, "
                  f"{useful / statistics.median(tt) / 1e12:7.2f} Tflop/s useful   rel-RMS hip against torch {err:.2e}")


if __name__ == "__main__":
    main()
