#!/usr/bin/env python
"""Image front and back end of one story on one MI355X (rcdms_amd/image.py) against the host paths they replace.
  front   5 frames of 128^2 uint8 on the host -> CLIP pixel values (5, 3, 224, 224) and VAE input (5, 3, 512, 512), both
          fp32 and resident on the device.  HIP: one 245-KB upload, two rcdm_image_resample launches.  Host: Pillow resize
          (+ crop) + numpy rescale / normalise per frame, then the upload of the fp32 tensors (4.7 MB + 15.7 MB).
  back    the decoder's f16 pixel rows of 5 x 512^2 frames -> uint8 frames on the host.  HIP: rcdm_frames_to_u8 + a 3.9-MB
          download.  Host: rcdm_rows_to_ncfhw to fp32 + (x / 2 + 0.5).clamp(0, 1) on the device, the 15.7-MB download, then
          (x * 255).astype(uint8) in numpy — what the pipeline and the driver do today.
Times are a host clock around calls that end in a device synchronise (uploads / downloads included), median of `--repeats`
windows of `--steps` calls after `--warmup` calls; kernel-only times come from device events.  Also prints the bytes each
kernel must move and the time that takes at 8 TB/s (the floor: these launches are far below it, they are latency bound).
Where Pillow is missing only the HIP side is recorded.  No pass / fail threshold.
usage: python tools/bench_image.py [--steps 50] [--warmup 10] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def timed(fn, warmup, steps, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)


def kernel_ms(fn, warmup, steps):
    from rcdms_amd import hip
    for _ in range(warmup):
        fn()
    a, b = hip.Event(), hip.Event()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    return round(a.elapsed_ms(b) / steps, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    from rcdms_amd import image as I
    from rcdms_amd.plan import Plan
    assert torch.cuda.is_available(), "bench_image.py measures on a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, size=(5, 128, 128, 3)).astype(np.uint8)
    proc, ft = I.ClipImageProcessor(device=dev), I.FrameTransform(512, 512, device=dev)
    T = (a.warmup, a.steps, a.repeats)
    res = {"metric": "image front / back end of one story (5 frames)", "unit": "ms", "n_gpus": 1, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "data": "synthetic"}

    # ---- front end
    def hip_front():
        d = torch.from_numpy(frames).to(dev)
        return proc(images=d).pixel_values, ft(d)
    res["front_hip_ms"] = timed(hip_front, *T)
    d = torch.from_numpy(frames).to(dev)
    res["front_hip_kernels_ms"] = {"clip_224_bicubic": kernel_ms(lambda: proc(images=d), a.warmup, a.steps),
                                   "vae_512_bilinear": kernel_ms(lambda: ft(d), a.warmup, a.steps)}
    fb = {"clip_224_bicubic": frames.nbytes + 5 * 3 * 224 * 224 * 4, "vae_512_bilinear": frames.nbytes + 5 * 3 * 512 * 512 * 4}
    res["front_kernel_bytes"] = fb
    res["front_kernel_floor_ms"] = {k: round(1e3 * v / HBM_BYTES_PER_S, 5) for k, v in fb.items()}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        mean, std = np.asarray(I.CLIP_MEAN, dtype=np.float32), np.asarray(I.CLIP_STD, dtype=np.float32)

        def host_front():
            clip, vae = [], []
            for f in frames:
                im = Image.fromarray(f)
                c = np.asarray(im.resize((224, 224), Image.Resampling.BICUBIC), dtype=np.float32) * np.float32(1 / 255)
                clip.append(((c - mean) / std).transpose(2, 0, 1))
                v = np.asarray(im.resize((512, 512), Image.Resampling.BILINEAR), dtype=np.float32) * np.float32(1 / 255)
                vae.append(((v - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))
            return torch.from_numpy(np.stack(clip)).to(dev), torch.from_numpy(np.stack(vae)).to(dev)
        res["front_host_pillow_ms"] = timed(host_front, a.warmup, max(a.steps // 5, 2), a.repeats)
        hc, hv = host_front()
        gc, gv = hip_front()
        res["front_max_abs_diff_vs_host"] = [float((hc - gc).abs().max()), float((hv - gv).abs().max())]
    else:
        res["front_host_pillow_ms"] = "not measured (Pillow missing)"

    # ---- back end: f16 pixel rows as VaeDecodeProgram.out_rows holds them (ld 8)
    plan = Plan(dev)
    rows = plan.rows("bench_rows", 5 * 512 * 512, 8, unique=True)
    plan.materialize()
    rows.buf.t.view(torch.float16).copy_((torch.randn(5 * 512 * 512 * 8, device=dev) * 0.7).half())

    def hip_back():
        return I.frames_to_uint8((rows, 5, 512, 512)).cpu().numpy()

    def host_back():
        out = torch.empty(5, 3, 1, 512, 512, dtype=torch.float32, device=dev)
        hip.rows_to_ncfhw(rows.ptr, rows.ld, 5, 3, 1, 512, 512, out.data_ptr())
        x = (out[:, :, 0] / 2 + 0.5).clamp(0, 1).cpu().float().numpy()
        return (x * 255).astype(np.uint8)
    res["back_hip_ms"] = timed(hip_back, *T)
    res["back_host_ms"] = timed(host_back, a.warmup, max(a.steps // 5, 2), a.repeats)
    res["back_hip_kernel_ms"] = kernel_ms(lambda: I.frames_to_uint8((rows, 5, 512, 512)), a.warmup, a.steps)
    bb = 5 * 512 * 512 * (8 * 2 + 3)          # whole 16-byte rows are fetched for the 6 bytes read
    res["back_kernel_bytes"] = bb
    res["back_kernel_floor_ms"] = round(1e3 * bb / HBM_BYTES_PER_S, 5)
    res["back_bytes_over_pcie"] = {"hip": 5 * 512 * 512 * 3, "host": 5 * 512 * 512 * 3 * 4}
    assert np.array_equal(hip_back(), host_back().transpose(0, 2, 3, 1)), "the two back ends disagree"
    res["back_outputs_identical"] = True
    res["timing_format"] = "[median, min, max] over the repeats"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
