#!/usr/bin/env python
"""Whole stories end to end on one MI355X: uploaded uint8 frames + captions -> CLIP vision -> stage 1 (prior, UnCLIP) -> hand-off
-> stage 2 (UNet loop, VAE) -> decoded uint8 frames, S stories per call through rcdms_amd.story.StoryRunner at S = 1, 2, 4,
against the two pipelines called in sequence one story at a time (what had to be done before the pipelines took a story axis:
the drivers' per-story work, three vision forwards for stage 1 and one for stage 2 included, minus the `.npy` files).
Real widths — CLIP-bigG vision and text, the 20-layer prior, SD-1.5 text encoder, the stage-2 UNet at 64 x 64 latents, the
SD-1.5 VAE at 512 x 512 — with the random-init weight family of bench.py (bench.init_weights_); frames are uniform noise of
the dataset's 128 x 128 size, captions procedural.  Also prints the per-stage split of a runner call (vision / stage 1 /
stage 2, each ended by a device synchronise).
Times are a host clock around calls that end in a device synchronise, median [min, max] of `--repeats` windows of `--calls`
calls after `--warmup` calls.  No pass / fail threshold.  One JSON line at the end.
usage: python tools/bench_story.py [--stories 1,2,4] [--steps 50] [--prior-steps 25] [--calls 1] [--warmup 1] [--repeats 3]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ["fred", "wilma", "barney", "betty", "dino", "is", "talking", "in", "the", "room", "walks", "outside", "to", "car", "a"]


class Tokenizer:
    """Stand-in for the CLIP tokenizer (no vocabulary file here): a start id, one id per character, the eos id — the largest
    of the vocabulary, so both pooling rules of rcdms_amd.clip find it."""

    def __init__(self, length, vocab=49408):
        self.model_max_length, self.vocab = length, vocab

    def __call__(self, texts, padding=None, max_length=None, truncation=True, return_tensors="pt"):
        texts = [texts] if isinstance(texts, str) else texts
        L = max_length or self.model_max_length
        ids = torch.zeros(len(texts), L, dtype=torch.long)
        am = torch.zeros(len(texts), L, dtype=torch.long)
        for i, s in enumerate(texts):
            n = min(len(s), L - 2)
            ids[i, 0] = self.vocab - 2
            for j in range(n):
                ids[i, 1 + j] = 1000 + ord(s[j])
            ids[i, 1 + n] = self.vocab - 1
            am[i, :n + 2] = 1
        return types.SimpleNamespace(input_ids=ids, attention_mask=am)


def timed(fn, warmup, calls, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return [round(statistics.median(out), 1), round(min(out), 1), round(max(out), 1)]


def on_device(make, dev):
    import bench
    with torch.device("meta"):
        m = make()
    m = m.to_empty(device=dev).eval()
    bench.init_weights_(m)
    return m


def build_models(dev):
    import bench
    from rcdms_amd import clip, context, vae
    from rcdms_amd.scheduler import DDIMScheduler, UnCLIPScheduler
    from src.models.myprior_transformer import MyPriorTransformer
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    from src.pipelines.prior_pipeline import Seq_Inpaint_Prior_Pipeline
    mk = dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
              temporal_position_encoding=True, temporal_position_encoding_max_len=5, temporal_attention_dim_div=1)
    big_text = dict(clip.TEXT_DEFAULTS, hidden_size=1280, num_attention_heads=20, num_hidden_layers=32, intermediate_size=5120,
                    max_position_embeddings=91, hidden_act="gelu", projection_dim=1280, eos_token_id=49407)
    sd_text = dict(clip.TEXT_DEFAULTS, max_position_embeddings=85)
    vision = on_device(lambda: clip.CLIPVisionEncoder(dict(clip.VISION_DEFAULTS)), dev)
    text1 = on_device(lambda: clip.CLIPTextEncoder(big_text), dev)
    text2 = on_device(lambda: clip.CLIPTextEncoder(sd_text, with_projection=False), dev)
    prior = on_device(lambda: MyPriorTransformer(
        num_attention_heads=32, attention_head_dim=64, num_layers=20, embedding_dim=1280, num_embeddings=91,
        additional_embeddings=6, unet_use_cross_frame_attention=False, unet_use_temporal_attention=False,
        use_motion_module=True, motion_module_type="Vanilla", motion_module_kwargs=mk), dev)
    prior.clip_mean, prior.clip_std = torch.tensor(-0.016, device=dev), torch.tensor(0.415, device=dev)
    unet = bench.build_model(dev)
    local = on_device(lambda: context.fine_stack(text_dim=768, vis_dim=1664), dev)
    glob = on_device(lambda: context.semantic_stack(text_dim=768, vis_dim=1280), dev)
    kl = on_device(lambda: vae.AutoencoderKL(), dev)
    prior_pipe = Seq_Inpaint_Prior_Pipeline(prior=prior, image_encoder=vision, text_encoder=text1, tokenizer=Tokenizer(91),
                                            scheduler=UnCLIPScheduler())
    stage2 = RCDMsPipeline(vae=kl, text_encoder=text2, tokenizer=Tokenizer(85), unet=unet, local_module=local,
                           global_module=glob, scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012,
                                                                        beta_schedule="linear"))
    stage2.set_progress_bar_config(disable=True)
    return prior_pipe, stage2, vision


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stories", default="1,2,4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--prior-steps", type=int, default=25)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--prior-guidance", type=float, default=4.0)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd.story import StoryRunner
    dev = torch.device("cuda", 0)
    prior_pipe, stage2, vision = build_models(dev)
    runner = StoryRunner(prior_pipe, stage2, vision)
    proc, ft = runner.clip_processor, runner.frame_transform
    Ss = [int(s) for s in a.stories.split(",")]
    g = torch.Generator().manual_seed(42)
    frames_host = torch.randint(0, 256, (max(Ss), 5, 128, 128, 3), dtype=torch.uint8, generator=g)
    texts = [[" ".join(WORDS[(7 * s + 3 * f + k) % len(WORDS)] for k in range(4 + (s + 2 * f) % 9)) for f in range(5)]
             for s in range(max(Ss))]
    gen, pgen = torch.Generator(device=dev).manual_seed(1), torch.Generator(device=dev).manual_seed(2)
    kw1 = dict(video_length=5, guidance_scale=a.prior_guidance, num_inference_steps=a.prior_steps)
    kw2 = dict(video_length=5, height=ft.height, width=ft.width, guidance_scale=a.guidance, num_inference_steps=a.steps,
               output_type="uint8")
    h, w = ft.height // 8, ft.width // 8

    def sequential_story(s):
        """One story the drivers' way: stage 1 (stage1…:146-261), then stage 2 (stage2…:267-376), batch 1."""
        fr = frames_host[s].to(dev)
        px = proc(images=fr).pixel_values
        vision(px)                                                                         # target_embed
        bw = torch.zeros(2, 128, 128, 3, dtype=torch.uint8, device=dev)
        bw[1] = 255
        pbw = proc(images=bw).pixel_values
        src = vision(torch.cat([px[:1], pbw[:1].expand(4, -1, -1, -1)])).image_embeds.unsqueeze(1)
        lab = vision(torch.cat([pbw[1:], pbw[:1].expand(4, -1, -1, -1)])).image_embeds.unsqueeze(1)
        emb = prior_pipe(texts[s], src, lab, generator=pgen, **kw1).image_embeds
        hidden = vision(px[:1]).last_hidden_state                                          # stage 2's own forward (:290)
        source = torch.full((5, 3, ft.height, ft.width), -1.0, device=dev)
        source[0] = ft(fr[:1])[0]
        label = torch.zeros(5, 1, h, w, device=dev)
        label[0] = 1.0
        return stage2(texts[s], source, image_embeds_1=hidden, proj_embeds_0=emb[1:].unsqueeze(1).float(), mask_label=label,
                      generator=gen, **kw2).videos

    rows = []
    base = timed(lambda: sequential_story(0), a.warmup, a.calls, a.repeats)
    print(f"sequential pipelines, 1 story per call: {base[0]} ms / story [{base[1]} .. {base[2]}]", flush=True)
    for S in Ss:
        fr_h, tx = frames_host[:S], texts[:S]
        run = lambda: runner(fr_h, tx, num_inference_steps=a.steps, prior_steps=a.prior_steps, guidance_scale=a.guidance,
                             prior_guidance_scale=a.prior_guidance, generator=gen, prior_generator=pgen, output_type="uint8")
        t = timed(run, a.warmup, a.calls, a.repeats)

        # the split: the runner's three parts on the same inputs, each ended by a synchronise
        fr = fr_h.to(dev)
        state = {}

        def part_vision():
            state["vis"] = vision(proc(images=fr.reshape(S * 5, 128, 128, 3)).pixel_values)

        def part_stage1():
            target = state["vis"].image_embeds.reshape(S, 5, -1)
            black, white = runner.black_white_embeds(fr[0])
            state["emb"] = prior_pipe(tx, *runner.stage1_inputs(target, black, white, "continue"), generator=pgen,
                                      **kw1).image_embeds

        def part_stage2():
            hid = state["vis"].last_hidden_state.reshape(S, 5, *state["vis"].last_hidden_state.shape[1:])
            source = torch.full((S, 5, 3, ft.height, ft.width), -1.0, device=dev)
            source[:, 0] = ft(fr[:, 0])
            label = torch.zeros(S, 5, h, w, device=dev)
            label[:, 0] = 1.0
            stage2(tx, source, image_embeds_1=[hid[s, :1] for s in range(S)],
                   proj_embeds_0=[state["emb"][s, 1:].unsqueeze(1).float() for s in range(S)], mask_label=label, generator=gen,
                   **kw2)
        split = [timed(p, a.warmup, a.calls, a.repeats) for p in (part_vision, part_stage1, part_stage2)]
        row = dict(stories=S, ms_per_call=t, ms_per_story=round(t[0] / S, 1), speedup_vs_sequential=round(base[0] * S / t[0], 3),
                   vision_ms=split[0], stage1_ms=split[1], stage2_ms=split[2],
                   rank1_runs=len(stage2._loop.rank1_runs or ()), shared_prefix=bool(stage2._loop.shared))
        rows.append(row)
        print(f"StoryRunner S={S}: {t[0]} ms / call [{t[1]} .. {t[2]}] = {row['ms_per_story']} ms / story, x{row['speedup_vs_sequential']}"
              f" vs sequential; vision {split[0][0]} | stage 1 {split[1][0]} | stage 2 {split[2][0]} ms", flush=True)
    print(json.dumps({"metric": "ms per story, uint8 frames in -> uint8 frames out (stage 1 + stage 2)", "unit": "ms",
                      "steps": a.steps, "prior_steps": a.prior_steps, "guidance": a.guidance, "prior_guidance": a.prior_guidance,
                      "calls": a.calls, "warmup": a.warmup, "repeats": a.repeats,
                      "timing_format": "[median, min, max] over the repeats", "sequential_ms_per_story": base, "runner": rows,
                      "data": "synthetic", "dtype": "f16"}), flush=True)


if __name__ == "__main__":
    main()
