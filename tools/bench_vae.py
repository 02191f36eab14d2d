#!/usr/bin/env python
"""VAE decode and encode of one story (SD-1.5 AutoencoderKL, random-init) on the HIP path, per form of the mid-block
attention (rcdms_amd.vae.mid_attention_form): device-event times around synchronised work, the forms ALTERNATING in one
process so that clock and thermal drift hit both alike.

  tools/bench_vae.py                               5 x 512x512, the default form (what the pipeline runs)
  tools/bench_vae.py --form scores,flash           both forms, alternating: median ms per story [min .. max] of --rounds
  tools/bench_vae.py --height 768 --width 768      larger images (more than 4096 latent pixels: the flash form only)
  tools/bench_vae.py --attn --form scores,flash    the attention alone inside the decoder's plan (between the GroupNorm and
                                                   the output projection), and the flash launch's useful TFLOP/s beside the
                                                   d = 160 kernel's at the same token count
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rcdms_amd import hip, switches, vae  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=512)
ap.add_argument("--width", type=int, default=512)
ap.add_argument("--frames", type=int, default=5)
ap.add_argument("--form", default="auto", help="comma list of auto | scores | flash (RCDM_VAE_FLASH unset | 0 | 1)")
ap.add_argument("--rounds", type=int, default=7, help="timed rounds per form (alternating)")
ap.add_argument("--reps", type=int, default=3, help="stories per round")
ap.add_argument("--attn", action="store_true", help="time the mid-block attention of the decoder alone")
args = ap.parse_args()
dev = torch.device("cuda", 0)
n, H, W = args.frames, args.height, args.width
h, w = H // 8, W // 8
forms = [f.strip() for f in args.form.split(",")]
SWITCH = {"auto": "auto", "scores": "0", "flash": "1"}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def report(name, rows):
    for form, ts in rows.items():
        print(f"{name} [{form}]: {statistics.median(ts):.3f} ms median of {len(ts)} [{min(ts):.3f} .. {max(ts):.3f}]")


models = {}
for form in forms:
    with torch.device("meta"):
        m = vae.AutoencoderKL()
    m = m.to_empty(device=dev).eval()
    bench.init_weights_(m)                       # same seed: the same weights in every copy
    models[form] = m
z = torch.randn(n, 4, h, w, device=dev)
x = torch.rand(n, 3, H, W, device=dev) * 2 - 1
for form, m in models.items():                   # programs are planned at the first call: under that form's switch
    switches.VAE_FLASH = SWITCH[form]
    y = m.decode(z).sample
    d = m.encode(x).latent_dist
    torch.cuda.synchronize()
    prog = m._programs[(n, h, w)][1]
    print(f"[{form}] decode plan {len(prog.plan.ops)} ops, {prog.plan.total_bytes() / 2**20:.0f} MiB of buffers, "
          f"attention as {vae.mid_attention_form(h * w, 512)}; finite {bool(torch.isfinite(y).all() and torch.isfinite(d.mean).all())}")
switches.VAE_FLASH = "auto"

if not args.attn:
    dec = {f: [] for f in forms}
    enc = {f: [] for f in forms}
    for _ in range(args.rounds):
        for form, m in models.items():
            dec[form].append(timed(lambda: m.decode(z), args.reps))
        for form, m in models.items():
            enc[form].append(timed(lambda: m.encode(x), args.reps))
    report(f"vae decode {n} x {H}x{W}, ms per story", dec)
    report(f"vae encode {n} x {H}x{W}, ms per story", enc)
    sys.exit(0)

# ---- the attention alone: the ops of the decoder's plan between the mid block's GroupNorm and its output projection
blocks, flash_op = {}, {}
for form, m in models.items():
    plan = m._programs[(n, h, w)][1].plan
    tags = plan.tags
    fl = [i for i, t in enumerate(tags) if t.startswith("flash_attn ")]
    sm = [i for i, t in enumerate(tags) if t.startswith("softmax_rows")]
    if fl:
        lo, hi = fl[0] - 1, fl[0]               # [q | k | v] GEMM, flash launch
        flash_op[form] = (plan, [plan.ops[fl[0]]])
    else:
        lo, hi = sm[0] - 4, sm[-1] + 1          # q GEMM, k GEMM, then per image V^T, scores, softmax, P V
    blocks[form] = (plan, plan.ops[lo:hi + 1], [tags[i] for i in range(lo, hi + 1)])
    print(f"[{form}] attention block = {hi - lo + 1} ops: {tags[lo]} ... {tags[hi]}")
res = {f: [] for f in forms}
for _ in range(args.rounds):
    for form in forms:
        plan, ops, _ = blocks[form]
        res[form].append(timed(lambda: plan.run(ops), 10))
report(f"mid-block attention {n} x {h * w} tokens x d 512 (projections of q, k, v included), ms", res)
L = h * w
for form, (plan, ops) in flash_op.items():
    ts = [timed(lambda: plan.run(ops), 10) for _ in range(args.rounds)]
    t = statistics.median(ts)
    print(f"flash launch alone [{form}]: {t:.3f} ms [{min(ts):.3f} .. {max(ts):.3f}] = "
          f"{4.0 * n * L * L * 512 / t / 1e9:.0f} useful TFLOP/s")
for form in forms:
    plan, ops, tags = blocks[form]
    per_img = ops[2:] if form not in flash_op else None
    if per_img:
        ts = [timed(lambda: plan.run(per_img), 10) for _ in range(args.rounds)]
        print(f"{len(per_img)} launches of the score-buffer form alone [{form}] (V^T, scores, softmax, P V per image): "
              f"{statistics.median(ts):.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]")
# orientation: the d = 160 kernel at the same token count
C = 160
qkv = torch.randn(n * L, 3 * C, device=dev).half()
out = torch.empty(n * L, C, dtype=torch.float16, device=dev)
desc = hip.AttnDesc(n, 1, L, L, C, 3 * C, 3 * C, 3 * C, C, C ** -0.5)
fn = lambda: hip.flash_attn(desc, qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, out.data_ptr())  # noqa: E731
fn()
ts = [timed(fn, 10) for _ in range(args.rounds)]
t = statistics.median(ts)
print(f"for orientation, rcdm_flash_attn {n} x {L} tokens x d 160: {t:.3f} ms = {4.0 * n * L * L * C / t / 1e9:.0f} useful TFLOP/s")
