#!/usr/bin/env python
"""What the device route of the denoising objective costs against the torch-op route, and what its two launches reach.

loss     DenoisingObjective.loss at the real width (the 1276.9 M-parameter stage-2 UNet at random init), 512 x 512 frames
         (64 x 64 latents), 5 frames, context of 85 rows, B = 1 and B = 4 stories, against the torch-op route through the SAME
         unet.forward — scheduler.add_noise, torch.cat, forward, a float64 mean —, which is what the tree could do before the
         objective existed.  Both routes get the same noise and timesteps.  Host clock around calls that end in a device
         synchronise; the two routes alternate; median [min, max] of `--windows` calls each after `--warmup` calls each (the
         first is the eager launch sequence, the second captures the graph).
launches rcdm_diffuse_assemble (one launch) and rcdm_eps_sqerr (two) alone on the plan's own buffers: `--reps` back-to-back
         calls between two device events.  Floor: the bytes each must move — assemble: 13 fp32 planes in, c_pad f16 columns
         out; sqerr: 4 fp32 planes and the ld f16 columns of the output rows in — at 6.3 TB/s, the rate a float4 copy reaches
         on this part.  Operands that fit the 256 MiB Infinity Cache are marked: their rate is not an HBM rate.

usage: tools/bench_objective.py [--windows 5] [--warmup 2] [--reps 200] [--batches 1 4]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HBM_RATE = 6.3e12
INFINITY_CACHE = 256 << 20


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--ctx-len", type=int, default=85)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective.py needs an MI355X: the hot path has no CPU fallback")
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip, synth
    from rcdms_amd.objective import DenoisingObjective
    from rcdms_amd.unet_program import CIN_PAD
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev)
    obj = DenoisingObjective(model)
    sched = obj.scheduler
    T = sched.config.num_train_timesteps
    print(f"{torch.cuda.get_device_name(0)}, frames {a.latent * 8} x {a.latent * 8}, 5 frames, context {a.ctx_len}, "
          f"{a.windows} calls per route, alternating, after {a.warmup} warm-up calls each; ms per call")
    for B in a.batches:
        s = synth.synthetic_story(stories=B, latent_hw=(a.latent, a.latent), ctx_len=a.ctx_len, cfg=False, seed=42)
        lat, mask, masked, ctx = (s[k].to(dev) for k in ("latents", "mask", "masked_latents", "ctx"))
        g = torch.Generator(device=dev).manual_seed(B)
        noise = torch.randn(lat.shape, generator=g, device=dev)
        t = torch.randint(0, T, (B,), generator=g, device=dev)
        n_el = lat.numel()

        def device_route():
            r = obj.loss(lat, masked, mask, ctx, timesteps=t, noise=noise)
            torch.cuda.synchronize()
            return r.loss

        def torch_route():
            x = torch.cat([sched.add_noise(lat, noise, t), mask, masked], dim=1)
            eps = model(x, t, ctx, return_dict=False)[0]
            loss = ((eps.double() - noise.double()) ** 2).sum() / n_el
            torch.cuda.synchronize()
            return loss

        routes = (("hip  ", device_route), ("torch", torch_route))
        with torch.no_grad():
            for _ in range(a.warmup):
                vals = [fn() for _, fn in routes]
            ms = {name: [] for name, _ in routes}
            for _ in range(a.windows):
                for name, fn in routes:
                    t0 = time.perf_counter()
                    fn()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        rel = abs(float(vals[0]) - float(vals[1])) / float(vals[1])
        for name, _ in routes:
            med, lo, hi = stats(ms[name])
            print(f"B = {B}  {name}  {med:8.3f} [{lo:.3f}, {hi:.3f}] ms" +
                  (f"   loss {float(vals[0]):.9e}, torch route {float(vals[1]):.9e}, relative difference {rel:.2e}"
                   if name == "hip  " else ""))

        # the launches alone, on the plan's buffers
        f, H, W = lat.shape[2:]
        prog = model.program(B, f, H, W, ctx.shape[1], rank1_runs=model._context_runs(ctx))
        table = sched.noise_table(dev)
        rows = B * f * H * W
        nbytes = hip.eps_sqerr_workspace_bytes(B, f, H, W)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        sq = torch.empty(B, f, dtype=torch.float64, device=dev)
        x_in, eps_out = prog.x_in, prog.eps_out
        seqs = {
            "rcdm_diffuse_assemble (one launch)": (
                lambda: hip.diffuse_assemble(lat.data_ptr(), noise.data_ptr(), 0, 0.0, t.data_ptr(), table.data_ptr(), T,
                                             mask.data_ptr(), masked.data_ptr(), B, f, H, W, x_in.ptr, x_in.ld, CIN_PAD),
                rows * (13 * 4 + CIN_PAD * 2)),
            "rcdm_eps_sqerr (two launches)": (
                lambda: hip.eps_sqerr(eps_out.ptr, eps_out.ld, noise.data_ptr(), 0, 0.0, B, f, H, W, sq.data_ptr(), ws.data_ptr(),
                                      nbytes),
                rows * (4 * 4 + eps_out.ld * 2)),
        }
        ev0, ev1 = hip.Event(), hip.Event()
        stream = prog.stream
        sp = stream.cuda_stream
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for name, (fn, moved) in seqs.items():
                fn()
                stream.synchronize()
                us = []
                for _ in range(a.windows):
                    ev0.record(sp)
                    for _ in range(a.reps):
                        fn()
                    ev1.record(sp)
                    stream.synchronize()
                    us.append(ev0.elapsed_ms(ev1) * 1e3 / a.reps)
                med, lo, hi = stats(us)
                note = "  (operands fit the Infinity Cache: not an HBM rate)" if moved <= INFINITY_CACHE else ""
                print(f"         {name}: {med:.3f} [{lo:.3f}, {hi:.3f}] us per call, {moved / 1e6:8.1f} MB, "
                      f"{moved / (med * 1e-6) / 1e12:5.2f} TB/s, {moved / HBM_RATE / (med * 1e-6):5.1%} of the byte floor{note}")


if __name__ == "__main__":
    main()
