#!/usr/bin/env python
"""Per-step graph time of the stage-2 denoising loop with each scheduler the loop runs, at BASELINE config 2 (512x512,
CFG 2.0, 1 story x 5 frames, context 85 x 768, the 1276.9 M-parameter UNet at random init), timed the way bench.py times
the headline: HIP events on the loop's stream around each pass of T graph replays, after warm-up passes; the inputs are
re-staged by load() outside the events.  DDIM (the headline scheduler) is timed in the same process, interleaved with the
others pass by pass, so that the numbers are comparable.  One JSON line per scheduler, then a summary line.

usage: tools/bench_schedulers.py [--steps-per-story T] [--passes K] [--warmup W]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def schedulers():
    from rcdms_amd import scheduler as sc
    kw = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="linear")
    ddim = sc.DDIMScheduler(steps_offset=1, clip_sample=False, **kw)
    return [
        ("ddim", ddim),
        ("pndm", sc.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **kw)),
        ("euler", sc.EulerDiscreteScheduler(**kw)),
        ("euler_ancestral", sc.EulerAncestralDiscreteScheduler(**kw)),
        ("lms", sc.LMSDiscreteScheduler(**kw)),
        ("dpmpp_2m_karras", sc.DPMSolverMultistepScheduler.from_config(ddim.config, use_karras_sigmas=True)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-per-story", type=int, default=50)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--ctx-len", type=int, default=85)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_schedulers.py needs an MI355X: the hot path has no CPU fallback")
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip, synth
    from rcdms_amd.sampler import DenoiseLoop
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev)
    story = synth.synthetic_story(stories=1, latent_hw=(a.latent, a.latent), ctx_len=a.ctx_len, seed=42)
    gen = torch.Generator(device=dev)
    loops = []
    for name, sched in schedulers():
        loop = DenoiseLoop(model, 1, 5, a.latent, a.latent, a.ctx_len, 2.0, sched, a.steps_per_story)
        loops.append((name, loop))

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
    for _ in range(a.passes):                      # interleaved: every scheduler sees the same machine state
        for name, loop in loops:
            load(loop)
            sp = loop.prog.stream.cuda_stream
            ev0.record(sp)
            loop.run()
            ev1.record(sp)
            torch.cuda.synchronize()
            ms[name].append(ev0.elapsed_ms(ev1) / loop.T)
    base = sorted(ms["ddim"])[len(ms["ddim"]) // 2]
    summary = {}
    for name, loop in loops:
        v = sorted(ms[name])
        med = v[len(v) // 2]
        finite = bool(torch.isfinite(loop.lat).all())
        rec = {"scheduler": name, "graph_replays_per_story": loop.T, "ms_per_step_median": round(med, 4),
               "ms_per_step_min": round(v[0], 4), "ms_per_step_max": round(v[-1], 4), "vs_ddim": round(med / base, 4),
               "ms_per_story": round(med * loop.T, 2), "passes": a.passes, "finite": finite}
        print(json.dumps(rec), flush=True)
        summary[name] = round(med, 4)
    print(json.dumps({"config": f"{a.latent * 8}x{a.latent * 8}, CFG 2.0, 1 story x 5 frames, ctx {a.ctx_len}",
                      "steps_per_story": a.steps_per_story, "ms_per_step_median": summary}), flush=True)


if __name__ == "__main__":
    main()
