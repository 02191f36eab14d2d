#!/usr/bin/env python
"""The files of one story on one MI355X (rcdms_amd.image.encode_png / checkpoint.story_grid_png) against PIL.Image.save.
  frames  five 512 x 512 uint8 frames resident on the device -> five PNG files as `bytes` on the host, one call
  grid    the 2 x 5 comparison grid, 2560 x 1024, assembled from device cells -> one PNG file as `bytes`
HIP: rcdm_png_encode (filter, block, assemble launches) + one download.  Host: PIL.Image.save of the same arrays (already
on the host; the download the host path needs first is not counted) at Pillow's default (compress_level 6) and at 1.
--match adds the match mode (rcdm_png_encode_match: encode_png(match=True), story_grid_png(match=True)) beside the literal-only
one in the same process: its times, its launch-sequence device time and its file sizes, and the ratios match / literal-only.
Frames are procedural cartoons (discs + gradient + Gaussian noise of --sigma grey levels): not decoder output.
Times are a host clock around calls that end in a device synchronise, median [min, max] of `--repeats` windows of `--steps`
calls after `--warmup` calls (tools/bench_image.py's convention); the device time of the three-launch sequence comes from
device events, the split per kernel from `rocprofv3 --kernel-trace --stats -- python tools/bench_png.py --launch-only
frames|grid` (recorded in profiles/png_encode.txt).  Also prints file sizes against Pillow's.  No pass / fail threshold.
usage: python tools/bench_png.py [--steps 20] [--warmup 5] [--repeats 5] [--sigma 2.0] [--match] [--launch-only frames|grid]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, steps, repeats, sync):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return [round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)]


def device_ms(fn, warmup, steps):
    from rcdms_amd import hip
    for _ in range(warmup):
        fn()
    a, b = hip.Event(), hip.Event()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    return round(a.elapsed_ms(b) / steps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=2.0)
    ap.add_argument("--launch-only", choices=["frames", "grid"], help="only `--steps` launch sequences of one shape: the run to put under rocprofv3")
    ap.add_argument("--match", action="store_true", help="also measure the match mode (with --launch-only: launch it instead)")
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import image as I
    from rcdms_amd.checkpoint import story_grid_png
    from tests import png_oracle as P
    assert torch.cuda.is_available(), "bench_png.py measures on a GPU"
    dev = torch.device("cuda", 0)
    frames = np.stack([P.cartoon(512, 512, a.sigma, 70 + i) for i in range(5)])
    d_frames = torch.from_numpy(frames).to(dev)
    cells = [d_frames[i % 5] for i in range(10)]
    grid = np.concatenate([np.concatenate(list(frames), axis=1)] * 2, axis=0)
    d_grid = torch.from_numpy(grid).to(dev)
    sync = torch.cuda.synchronize
    if a.launch_only:
        enc, src = ((I.png_encoder(512, 512, 5, dev, a.match), d_frames) if a.launch_only == "frames" else
                    (I.png_encoder(1024, 2560, 1, dev, a.match), d_grid))
        for _ in range(a.steps):
            enc.launch(src)
        sync()
        return
    T = (a.warmup, a.steps, a.repeats, sync)
    res = {"metric": "PNG files of one story (5 frames of 512^2 + one 2560x1024 grid)", "unit": "ms", "n_gpus": 1, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "data": f"procedural cartoon, sigma {a.sigma}",
           "timing_format": "[median, min, max] over the repeats"}

    res["frames_hip_ms"] = timed(lambda: I.encode_png(d_frames), *T)
    res["grid_hip_ms"] = timed(lambda: story_grid_png(cells, 2, 5), *T)
    res["story_hip_ms"] = round(res["frames_hip_ms"][0] + res["grid_hip_ms"][0], 3)
    e5, e1 = I.png_encoder(512, 512, 5, dev), I.png_encoder(1024, 2560, 1, dev)
    res["frames_hip_launches_ms"] = device_ms(lambda: e5.launch(d_frames), a.warmup, a.steps)
    res["grid_hip_launches_ms"] = device_ms(lambda: e1.launch(d_grid), a.warmup, a.steps)
    res["download_bytes"] = {"frames": int(e5.out.numel()), "grid": int(e1.out.numel())}

    hip_frames = I.encode_png(d_frames)
    hip_grid = story_grid_png(cells, 2, 5)
    match_frames = match_grid = None
    if a.match:
        res["frames_hip_match_ms"] = timed(lambda: I.encode_png(d_frames, match=True), *T)
        res["grid_hip_match_ms"] = timed(lambda: story_grid_png(cells, 2, 5, match=True), *T)
        res["story_hip_match_ms"] = round(res["frames_hip_match_ms"][0] + res["grid_hip_match_ms"][0], 3)
        m5, m1 = I.png_encoder(512, 512, 5, dev, True), I.png_encoder(1024, 2560, 1, dev, True)
        res["frames_hip_match_launches_ms"] = device_ms(lambda: m5.launch(d_frames), a.warmup, a.steps)
        res["grid_hip_match_launches_ms"] = device_ms(lambda: m1.launch(d_grid), a.warmup, a.steps)
        res["match_over_literal_launches"] = {"frames": round(res["frames_hip_match_launches_ms"] / res["frames_hip_launches_ms"], 3),
                                              "grid": round(res["grid_hip_match_launches_ms"] / res["grid_hip_launches_ms"], 3)}
        match_frames = I.encode_png(d_frames, match=True)
        match_grid = story_grid_png(cells, 2, 5, match=True)
        res["bytes_match"] = {"frames_hip_match": [len(f) for f in match_frames], "grid_hip_match": len(match_grid),
                              "frames_hip": [len(f) for f in hip_frames], "grid_hip": len(hip_grid)}
        res["size_ratio_match_vs_literal"] = {"frames": round(sum(map(len, match_frames)) / sum(map(len, hip_frames)), 3),
                                              "grid": round(len(match_grid) / len(hip_grid), 3)}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        def pil(arr, **kw):
            o = io.BytesIO()
            Image.fromarray(arr).save(o, format="PNG", **kw)
            return o.getvalue()
        host_steps = max(a.steps // 10, 1)
        H = (1, host_steps, a.repeats, lambda: None)
        res["frames_pillow_default_ms"] = timed(lambda: [pil(f) for f in frames], *H)
        res["frames_pillow_level1_ms"] = timed(lambda: [pil(f, compress_level=1) for f in frames], *H)
        res["grid_pillow_default_ms"] = timed(lambda: pil(grid), *H)
        res["grid_pillow_level1_ms"] = timed(lambda: pil(grid, compress_level=1), *H)
        res["story_pillow_default_ms"] = round(res["frames_pillow_default_ms"][0] + res["grid_pillow_default_ms"][0], 3)
        res["story_pillow_level1_ms"] = round(res["frames_pillow_level1_ms"][0] + res["grid_pillow_level1_ms"][0], 3)
        res["bytes"] = {"frames_hip": [len(f) for f in hip_frames], "frames_pillow_default": [len(pil(f)) for f in frames],
                        "frames_pillow_level1": [len(pil(f, compress_level=1)) for f in frames],
                        "grid_hip": len(hip_grid), "grid_pillow_default": len(pil(grid)), "grid_pillow_level1": len(pil(grid, compress_level=1))}
        b = res["bytes"]
        res["size_ratio_vs_pillow_default"] = {"frames": round(sum(b["frames_hip"]) / sum(b["frames_pillow_default"]), 3),
                                               "grid": round(b["grid_hip"] / b["grid_pillow_default"], 3)}
        for f, want in zip(hip_frames, frames):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), want)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(hip_grid))), grid)
        if a.match:
            res["size_ratio_match_vs_pillow_default"] = {"frames": round(sum(map(len, match_frames)) / sum(b["frames_pillow_default"]), 3),
                                                         "grid": round(len(match_grid) / b["grid_pillow_default"], 3)}
            for f, want in zip(match_frames, frames):
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), want)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(match_grid))), grid)
        res["files_decode_to_input"] = True
        import PIL
        res["pillow"] = PIL.__version__
    else:
        res["frames_pillow_default_ms"] = "not measured (Pillow missing)"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
