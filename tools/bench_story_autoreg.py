#!/usr/bin/env python
"""Stage-2 autoregression end to end on one MI355X: StoryRunner(stage2_autoreg=True) — five stage-2 passes at batch S, the
kept frames handed on as device bytes — at S = 1, 2, 4, against
  * the plain runner call (one stage-2 pass) on the same stories, for scale, and
  * the same frames the driver's way, one story at a time: vision + stage 1 as tools/bench_story.py's sequential pipelines,
    then five single-story RCDMsPipeline calls with the driver's hand-off between them — download the kept frame,
    PIL.Image.save, Image.open, ToTensor / Normalize (restated on numpy: torchvision is not a dependency), upload — and the
    vision forward of each newly kept frame, which the runner makes too.
Also: the stage-2 time of each of the five passes (their seen-frame patterns select different launch plans), the hand-off
arithmetic alone (source_from_bytes + the copy into the source rows) and with its vision forward, the live UNetProgram count
and the device memory allocated after the warm-up call.
--plan general runs everything with the rank-1-context plans switched off (RCDM_RANK1_CTX=0, set before rcdms_amd is
imported): every pass then takes the one general plan of its geometry.  Run the tool once per plan form.
Models, weights, frames, captions and the timing method are tools/bench_story.py's: real widths, random-init weights, a host
clock around calls that end in a device synchronise, median [min, max] of `--repeats` windows after `--warmup` calls.  No
pass / fail threshold.  One JSON line at the end.
usage: python tools/bench_story_autoreg.py [--plan rank1|general] [--stories 1,2,4] [--steps 50] [--prior-steps 25]
       [--warmup 1] [--repeats 3] [--no-driver]"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", choices=("rank1", "general"), default="rank1")
    ap.add_argument("--stories", default="1,2,4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--prior-steps", type=int, default=25)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--prior-guidance", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-driver", action="store_true", help="skip the driver's-way baseline")
    a = ap.parse_args()
    if a.plan == "general":
        os.environ["RCDM_RANK1_CTX"] = "0"
    import numpy as np
    import torch
    from PIL import Image
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd.engine import UNetProgram
    from rcdms_amd.story import StoryRunner, source_from_bytes
    from tools.bench_story import WORDS, build_models, timed
    dev = torch.device("cuda", 0)
    prior_pipe, stage2, vision = build_models(dev)
    runner = StoryRunner(prior_pipe, stage2, vision)
    proc, ft = runner.clip_processor, runner.frame_transform
    H, W = ft.height, ft.width
    h, w = H // 8, W // 8
    Ss = [int(s) for s in a.stories.split(",")]
    g = torch.Generator().manual_seed(42)
    frames_host = torch.randint(0, 256, (max(Ss), 5, 128, 128, 3), dtype=torch.uint8, generator=g)
    texts = [[" ".join(WORDS[(7 * s + 3 * f + k) % len(WORDS)] for k in range(4 + (s + 2 * f) % 9)) for f in range(5)]
             for s in range(max(Ss))]
    gen, pgen = torch.Generator(device=dev).manual_seed(1), torch.Generator(device=dev).manual_seed(2)
    kw1 = dict(video_length=5, guidance_scale=a.prior_guidance, num_inference_steps=a.prior_steps)
    kw2 = dict(video_length=5, height=H, width=W, guidance_scale=a.guidance, num_inference_steps=a.steps, output_type="uint8")
    T = (a.warmup, 1, a.repeats)
    tmp = tempfile.mkdtemp(prefix="story_autoreg_")

    def driver_story(s):
        """One story the drivers' way: stage 1 (stage1…:146-261), then the --autoreg loop (stage2…:304-362), batch 1."""
        fr = frames_host[s].to(dev)
        px = proc(images=fr).pixel_values
        vision(px)                                                                         # target_embed
        bw = torch.zeros(2, 128, 128, 3, dtype=torch.uint8, device=dev)
        bw[1] = 255
        pbw = proc(images=bw).pixel_values
        src = vision(torch.cat([px[:1], pbw[:1].expand(4, -1, -1, -1)])).image_embeds.unsqueeze(1)
        lab = vision(torch.cat([pbw[1:], pbw[:1].expand(4, -1, -1, -1)])).image_embeds.unsqueeze(1)
        emb = prior_pipe(texts[s], src, lab, generator=pgen, **kw1).image_embeds.float()
        hidden = [vision(px[:1]).last_hidden_state]                                        # stage 2's own forward (:290)
        source = torch.full((5, 3, H, W), -1.0, device=dev)
        source[0] = ft(fr[:1])[0]
        label = torch.zeros(5, 1, h, w, device=dev)
        label[0] = 1.0
        kept = []
        for i in range(5):
            if i >= 1:
                path = os.path.join(tmp, f"{s}_{i - 1}.png")
                Image.fromarray(kept[-1].cpu().numpy()).save(path)                         # :361-362
                x = np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255    # :307-308, ToTensor
                x = (torch.from_numpy(x).permute(2, 0, 1) - 0.5) / 0.5                     # Normalize([0.5], [0.5])
                source[i - 1] = x.to(dev)
                label[i - 1] = 1.0
                new = vision(proc(images=kept[-1][None]).pixel_values).last_hidden_state
                hidden = [new] if i == 1 else hidden + [new]
            out = stage2(texts[s], source, image_embeds_1=torch.cat(hidden), proj_embeds_0=emb[max(i, 1):].unsqueeze(1),
                         mask_label=label, generator=gen, **kw2).videos
            kept.append(out[0, i])
        return torch.stack(kept)

    def live_plans():
        gc.collect()
        return sum(type(o) is UNetProgram for o in gc.get_objects())

    def fine(fn, calls=100):
        """[median, min, max] ms per call of a sub-millisecond step: windows of `calls` calls, unrounded."""
        import statistics
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0) / calls)
        return [statistics.median(out), min(out), max(out)]

    class PassClock:
        """The stage-2 pipeline with a synchronised clock around every call."""

        def __init__(self, pipe):
            self.pipe, self.ms = pipe, []

        def __getattr__(self, name):
            return getattr(self.pipe, name)

        def __call__(self, *args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = self.pipe(*args, **kw)
            torch.cuda.synchronize()
            self.ms.append(round(1e3 * (time.perf_counter() - t0), 1))
            return out

    base_mem = torch.cuda.memory_allocated(dev)
    rows, driver = [], None
    if not a.no_driver:
        driver = timed(lambda: driver_story(0), *T)
        print(f"driver's way, 1 story per call, five stage-2 calls + PNG hand-off: {driver[0]} ms / story "
              f"[{driver[1]} .. {driver[2]}]", flush=True)
    for S in Ss:
        fr_h, tx = frames_host[:S], texts[:S]
        kw = dict(num_inference_steps=a.steps, prior_steps=a.prior_steps, guidance_scale=a.guidance,
                  prior_guidance_scale=a.prior_guidance, generator=gen, prior_generator=pgen, output_type="uint8")
        auto = timed(lambda: runner(fr_h, tx, stage2_autoreg=True, **kw), *T)
        mem, plans = torch.cuda.memory_allocated(dev), live_plans()
        plain = timed(lambda: runner(fr_h, tx, **kw), *T)
        # one more autoregressive call with a clock around each pass, and the hand-off on its own
        clock = PassClock(stage2)
        runner.stage2_pipe = clock
        try:
            res = runner(fr_h, tx, stage2_autoreg=True, **kw)
        finally:
            runner.stage2_pipe = stage2
        source = torch.full((S, 5, 3, H, W), -1.0, device=dev)
        kept = res.frames_u8[:, 0].contiguous()

        def handoff():
            source[:, 0] = source_from_bytes(kept)

        def handoff_with_vision():
            handoff()
            vision(proc(images=kept).pixel_values)
        t_hand_vis = timed(handoff_with_vision, *T)
        t_hand = [round(t, 3) for t in fine(handoff)]
        variants = len(stage2._loop._variants)
        row = dict(stories=S, autoreg_ms_per_call=auto, autoreg_ms_per_story=round(auto[0] / S, 1), plain_ms_per_call=plain,
                   plain_ms_per_story=round(plain[0] / S, 1), autoreg_over_plain=round(auto[0] / plain[0], 3),
                   pass_ms=clock.ms, handoff_ms=t_hand, handoff_with_vision_ms=t_hand_vis,
                   handoff_share_of_a_pass=round(t_hand[0] / (sum(clock.ms) / 5), 5),
                   live_unet_programs=plans, loop_variants=variants,
                   allocated_gb_after_warmup=round(mem / 2 ** 30, 2), allocated_gb_models_only=round(base_mem / 2 ** 30, 2))
        if driver is not None:
            row["speedup_vs_driver"] = round(driver[0] * S / auto[0], 3)
        rows.append(row)
        print(f"stage2_autoreg S={S} ({a.plan} plans): {auto[0]} ms / call [{auto[1]} .. {auto[2]}] = {row['autoreg_ms_per_story']} "
              f"ms / story; plain {row['plain_ms_per_story']} ms / story (x{row['autoreg_over_plain']}); passes {clock.ms} ms; "
              f"hand-off {t_hand[0]} ms (+ vision: {t_hand_vis[0]} ms); {plans} live plans, {row['allocated_gb_after_warmup']} GB "
              f"allocated ({row['allocated_gb_models_only']} GB before any plan)", flush=True)
    print(json.dumps({"metric": "ms per story, uint8 frames in -> five autoregressive stage-2 passes -> uint8 frames out "
                                "(vision + stage 1 + stage 2)", "unit": "ms", "plan": a.plan, "steps": a.steps,
                      "prior_steps": a.prior_steps, "guidance": a.guidance, "prior_guidance": a.prior_guidance,
                      "warmup": a.warmup, "repeats": a.repeats, "timing_format": "[median, min, max] over the repeats",
                      "driver_ms_per_story": driver, "runner": rows, "data": "synthetic", "dtype": "f16"}), flush=True)


if __name__ == "__main__":
    main()
