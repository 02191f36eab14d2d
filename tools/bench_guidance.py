#!/usr/bin/env python
"""What guidance_rescale and eta cost in the captured step: per-step graph time of the stage-2 denoising loop (one 512x512
story, 50 DDIM steps, the 1276.9 M-parameter UNet at random init) with neither argument — the graph as it was —, with
guidance_rescale = 0.7 (two more launches and the `_scaled` step) and with eta = 1 (the table step with a noise row), timed
the way tools/bench_schedulers.py does: HIP events on the loop's stream around each pass of T graph replays, after warm-up
passes, the three loops interleaved pass by pass in one process.  Then the added launch sequence alone (the two launches
of rcdm_cfg_rescale_factor on the loop's own eps rows) and the DDIM step with and without factors, from device events
around `--reps` back-to-back calls.  One JSON line per case, then a summary line.

usage: tools/bench_guidance.py [--steps-per-story T] [--passes K] [--warmup W] [--guidance-scale G]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def stats(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-per-story", type=int, default=50)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--ctx-len", type=int, default=85)
    ap.add_argument("--guidance-scale", type=float, default=7.5)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py needs an MI355X: the hot path has no CPU fallback")
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip, synth
    from rcdms_amd import scheduler as sc
    from rcdms_amd.sampler import DenoiseLoop
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev)
    story = synth.synthetic_story(stories=1, latent_hw=(a.latent, a.latent), ctx_len=a.ctx_len, seed=42)
    gen = torch.Generator(device=dev)
    mk = lambda: sc.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    cases = [("plain", {}), ("guidance_rescale_0.7", dict(guidance_rescale=0.7)), ("eta_1", dict(eta=1.0))]
    loops = [(name, DenoiseLoop(model, 1, 5, a.latent, a.latent, a.ctx_len, a.guidance_scale, mk(), a.steps_per_story, **kw))
             for name, kw in cases]

    def load(loop):
        gen.manual_seed(0)
        loop.load(story["latents"], story["mask"], story["masked_latents"], story["ctx"], generator=gen)

    for _, loop in loops:
        for _ in range(a.warmup):
            load(loop)
            loop.run()
    torch.cuda.synchronize()
    ev0, ev1 = hip.Event(), hip.Event()
    ms = {name: [] for name, _ in loops}
    for _ in range(a.passes):                      # interleaved: every case sees the same machine state
        for name, loop in loops:
            load(loop)
            sp = loop.prog.stream.cuda_stream
            ev0.record(sp)
            loop.run()
            ev1.record(sp)
            torch.cuda.synchronize()
            ms[name].append(ev0.elapsed_ms(ev1) / loop.T)
    base = stats(ms["plain"])[0]
    summary = {}
    for name, loop in loops:
        med, lo, hi = stats(ms[name])
        print(json.dumps({"case": name, "graph_replays_per_story": loop.T, "ms_per_step_median": med, "ms_per_step_min": lo,
                          "ms_per_step_max": hi, "vs_plain": round(med / base, 5), "delta_us_per_step": round((med - base) * 1e3, 2),
                          "passes": a.passes, "finite": bool(torch.isfinite(loop.lat).all())}), flush=True)
        summary[name] = med

    # the added launches alone, on the eps rows the last step left behind
    loop = loops[1][1]
    eps, S, f, H, W = loop.prog.eps_out, loop.S, loop.f, loop.H, loop.W
    stream = loop.prog.stream
    sp = stream.cuda_stream
    lat = loop.lat.clone()
    step0 = torch.zeros(1, dtype=torch.int32, device=dev)
    seqs = {
        "rescale_factor_2_launches": lambda: hip.cfg_rescale_factor(eps.ptr, eps.ld, S, f, H, W, loop.gs, loop.phi,
                                                                    loop._guide_ws.data_ptr(), loop._guide_ws.numel(),
                                                                    loop.factor.data_ptr()),
        "ddim_step": lambda: hip.cfg_ddim_step(eps.ptr, eps.ld, lat.data_ptr(), S, 2, f, H, W, loop.gs, loop.coef.data_ptr(),
                                               step0.data_ptr()),
        "ddim_step_scaled": lambda: hip.cfg_ddim_step_scaled(eps.ptr, eps.ld, lat.data_ptr(), S, 2, f, H, W, loop.gs,
                                                             loop.coef.data_ptr(), step0.data_ptr(), loop.factor.data_ptr()),
    }
    us = {k: [] for k in seqs}
    with torch.cuda.stream(stream):
        for fn in seqs.values():
            fn()
        stream.synchronize()
        for _ in range(a.passes):
            for k, fn in seqs.items():
                lat.copy_(loop.lat)
                ev0.record(sp)
                for _ in range(a.reps):
                    fn()
                ev1.record(sp)
                stream.synchronize()
                us[k].append(ev0.elapsed_ms(ev1) * 1e3 / a.reps)
    for k in seqs:
        med, lo, hi = stats(us[k])
        print(json.dumps({"sequence": k, "us_per_call_median": med, "us_per_call_min": lo, "us_per_call_max": hi,
                          "calls_per_window": a.reps, "windows": a.passes}), flush=True)
        summary[k + "_us"] = med
    print(json.dumps({"config": f"{a.latent * 8}x{a.latent * 8}, CFG {a.guidance_scale}, 1 story x 5 frames, ctx {a.ctx_len}, "
                                f"{a.steps_per_story} DDIM steps", "summary": summary}), flush=True)


if __name__ == "__main__":
    main()
