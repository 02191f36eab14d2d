#!/usr/bin/env python
"""PNG files -> uint8 frames on one MI355X (rcdms_amd.image.decode_png) against Pillow on the host.
  strips   1000 strips of 640 x 128 (five 128 x 128 frames: the h5 split's entries) in one call, written by Pillow at its
           default from procedural cartoons of sigma 2 and of sigma 0
  story    five 512 x 512 files per call: written by Pillow at its default, by encode_png, by encode_png(match=True)
  single   one 512 x 512 file (Pillow's): the latency of a single stream
HIP: decode_png — the host walk, one upload of the file bytes, one of the tables, the two launches of rcdm_png_decode, one
download of the status words; the frames stay on the device.  Host: Image.open(io.BytesIO(b)).convert("RGB") per file, one
thread, plus the upload of the pixels (one torch.from_numpy(np.stack(...)).to(device) per call).  Every decoded batch is
compared with Pillow's pixels before it is timed.  Times are a host clock around calls that end in a device synchronise,
median [min, max] of `--repeats` windows of `--steps` calls after `--warmup` calls (tools/bench_png.py's convention; the
1000-strip case runs steps / 10 calls per window); `*_launches_ms` is the two-launch sequence alone from device events.
No pass / fail threshold.
usage: python tools/bench_png_decode.py [--steps 20] [--warmup 5] [--repeats 5] [--strips 1000] [--launch-only strips|story|single]"""
import argparse
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import device_ms, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--strips", type=int, default=1000)
    ap.add_argument("--launch-only", choices=["strips", "story", "single"], help="only `--steps` launch sequences of one case: the run to put under rocprofv3")
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from PIL import Image
    import PIL
    from rcdms_amd import image as I
    from tests import png_oracle as P
    assert torch.cuda.is_available(), "bench_png_decode.py measures on a GPU"
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize

    def pil_write(arr):
        o = io.BytesIO()
        Image.fromarray(arr).save(o, format="PNG")
        return o.getvalue()

    def pil_read(files):
        return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in files])).to(dev)

    # 20 distinct strips per sigma, repeated: the files of one call differ, the set stays small enough to build quickly
    strips = {s: [pil_write(P.cartoon(640, 128, s, 100 + k)) for k in range(20)] for s in (2.0, 0.0)}
    strips = {s: [v[k % 20] for k in range(a.strips)] for s, v in strips.items()}
    frames = np.stack([P.cartoon(512, 512, 2.0, 70 + i) for i in range(5)])
    d_frames = torch.from_numpy(frames).to(dev)
    story = {"pillow": [pil_write(f) for f in frames], "encode_png": I.encode_png(d_frames), "encode_png_match": I.encode_png(d_frames, match=True)}
    cases = {"strips_sigma2": strips[2.0], "strips_sigma0": strips[0.0], **{f"story_{k}": v for k, v in story.items()},
             "single": story["pillow"][:1]}
    dec = I.png_decoder(dev)

    def resident(files):
        plan = I.png_decode_plan(files)
        src, tables = dec.upload(plan)
        bufs = (torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev), torch.empty(plan.dst_bytes, dtype=torch.uint8, device=dev),
                torch.empty(plan.n, dtype=torch.int32, device=dev))
        return lambda: dec.launch(plan, src, tables, *bufs)

    if a.launch_only:
        fn = resident({"strips": cases["strips_sigma2"], "story": cases["story_pillow"], "single": cases["single"]}[a.launch_only])
        for _ in range(a.steps):
            fn()
        sync()
        return
    res = {"metric": "PNG files -> uint8 frames resident on the device", "unit": "ms per call", "n_gpus": 1, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "timing_format": "[median, min, max] over the repeats", "pillow": PIL.__version__,
           "host": "Image.open(BytesIO(b)).convert('RGB') per file on one thread + one upload of the stacked pixels"}
    for name, files in cases.items():
        got = I.PngDecoder.batch(I.decode_png(files))
        assert torch.equal(got, pil_read(files)), name
        steps = max(a.steps // 10, 1) if len(files) > 100 else a.steps
        warm = 1 if len(files) > 100 else a.warmup
        res[name] = {"files": len(files), "file_bytes": sum(map(len, files)), "pixel_bytes": int(got.numel()),
                     "hip_ms": timed(lambda: I.decode_png(files), warm, steps, a.repeats, sync),
                     "hip_launches_ms": device_ms(resident(files), warm, steps),
                     "pillow_ms": timed(lambda: pil_read(files), 1, max(steps // 2, 1), a.repeats, sync)}
        res[name]["pillow_over_hip"] = round(res[name]["pillow_ms"][0] / res[name]["hip_ms"][0], 2)
    res["decoded_equals_pillow"] = True
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
