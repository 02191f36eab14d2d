#!/usr/bin/env python
"""CLIP encoders on the HIP path (rcdms_amd/clip.py) at the real shapes, random-init weights on one MI355X: the CLIP-bigG
vision tower (48 layers, 1664 wide, 16 x 104; B = 1 and 5 images of 224^2), the SD-1.5 text encoder (12 layers, 768 wide;
10 x 85 tokens) and the CLIP-bigG text encoder (32 layers, 1280 wide; 10 x 91 tokens).  Prints one JSON line: ms per
forward (host clock around forwards that end in a device synchronise: an eager launch plan, so launch overhead is in),
f16 weight bytes and the weight-read floor at 8 TB/s.  Where `transformers` imports, the same architecture is also timed as
the torch module in fp32 — the path these encoders replace.  No pass / fail threshold.
usage: python tools/bench_clip.py [--steps 10] [--warmup 3] [--no-torch]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def torch_module(kind, cfg, dev):
    """The transformers module of the same architecture on the GPU in fp32, or None when transformers is not installed."""
    try:
        from transformers import (CLIPTextConfig, CLIPTextModelWithProjection, CLIPVisionConfig,
                                  CLIPVisionModelWithProjection)
    except Exception:
        return None
    import bench
    with torch.device("meta"):
        m = (CLIPTextModelWithProjection(CLIPTextConfig(**cfg)) if kind == "text" else
             CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg)))
    m = m.to_empty(device=dev).eval()
    bench.init_weights_(m)
    for n, b in m.named_buffers():     # (buffers, not parameters: to_empty left them uninitialised)
        if n.endswith("position_ids"):
            b.copy_(torch.arange(b.shape[-1], device=dev)[None])
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import bench
    from rcdms_amd import clip
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(42)
    big_text = dict(clip.TEXT_DEFAULTS, hidden_size=1280, num_attention_heads=20, num_hidden_layers=32, intermediate_size=5120,
                    max_position_embeddings=91, hidden_act="gelu", projection_dim=1280, eos_token_id=49407)
    sd_text = dict(clip.TEXT_DEFAULTS, max_position_embeddings=85)
    cases = [("bigG vision", "vision", dict(clip.VISION_DEFAULTS), (1, 5)),
             ("SD text", "text", sd_text, (10,)),
             ("bigG text", "text", big_text, (10,))]
    rows = []
    for name, kind, cfg, batches in cases:
        with torch.device("meta"):
            m = (clip.CLIPTextEncoder if kind == "text" else clip.CLIPVisionEncoder)(cfg)
        m = m.to_empty(device=dev).eval()
        bench.init_weights_(m)
        ref = None if a.no_torch else torch_module(kind, cfg, dev)
        wb = m.weight_bytes_f16()
        for B in batches:
            if kind == "text":
                L = cfg["max_position_embeddings"]
                x = torch.randint(3, cfg["vocab_size"] - 1, (B, L), device=dev, generator=g)
                x[:, L // 2] = cfg["vocab_size"] - 1
                kw = dict(input_ids=x)
            else:
                kw = dict(pixel_values=torch.randn(B, 3, cfg["image_size"], cfg["image_size"], device=dev, generator=g))
            row = {"encoder": name, "batch": B, "tokens": B * (kw["input_ids"].shape[1] if kind == "text" else 257),
                   "layers": cfg["num_hidden_layers"], "ms_per_forward": round(timed(lambda: m(**kw), a.warmup, a.steps), 3),
                   "weight_mb_f16": round(wb / 1e6, 1), "weight_read_floor_ms": round(1e3 * wb / HBM_BYTES_PER_S, 3)}
            if ref is not None:
                with torch.no_grad():
                    row["torch_fp32_ms_per_forward"] = round(timed(lambda: ref(**kw), a.warmup, a.steps), 3)
            else:
                row["torch_fp32_ms_per_forward"] = None
            rows.append(row)
        del m, ref
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "CLIP encoder forward, HIP launch plan vs the torch fp32 module it replaces", "unit": "ms",
                      "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "dtype": "f16", "data": "synthetic",
                      "weights": "random init", "torch_reference": "transformers fp32 module" if any(
                          r["torch_fp32_ms_per_forward"] is not None for r in rows) else "not measured (transformers missing)",
                      "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
