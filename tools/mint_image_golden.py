"""Mint tests/golden/image_*.npz from Pillow itself (run where Pillow imports; the tests only read the files).

Each file holds one resample case: `input` uint8 (n, h, w, 3) — seeded noise with a saturated 0 / 255 quadrant, so bicubic
overshoot reaches the clip —, `output` uint8 (n, out_h, out_w, 3) = PIL.Image.resize (cropped to `window` where the case
has one), the integer tables `kx, bx, ky, by` of tests/image_oracle.py for exactly those output rows / columns (the tool
refuses to write a file unless the oracle run with these tables reproduces Pillow's bytes), and `meta` (JSON: filter,
sizes, window, Pillow version).  Where transformers' PIL-backed CLIPImageProcessor imports, the CLIP cases also carry its
`pixel_values`.

    python tools/mint_image_golden.py [--out tests/golden]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import image_oracle as IO  # noqa: E402

# name -> (n, in_h, in_w, resized_h, resized_w, filter, window (top, left, h, w) | None, seed)
CASES = {
    "image_up_odd":        (1, 13, 7, 29, 31, "bicubic", None, 1),
    "image_down_bilinear": (1, 37, 53, 16, 24, "bilinear", None, 2),
    "image_down_bicubic":  (5, 37, 53, 16, 24, "bicubic", None, 3),        # a batch of five
    "image_skip_rows":     (1, 64, 64, 64, 224, "bicubic", None, 4),       # the vertical pass is skipped
    "image_ratio":         (1, 75, 75, 131, 131, "bicubic", None, 5),
    "image_clip_crop":     (1, 200, 300, 224, 336, "bicubic", (0, 56, 224, 224), 6),
    "image_clip_tall":     (1, 150, 100, 336, 224, "bicubic", (56, 0, 224, 224), 7),
    "image_real_clip":     (1, 128, 128, 224, 224, "bicubic", None, 8),
    "image_real_vae":      (1, 128, 128, 512, 512, "bilinear", None, 9),
}
CLIP_CASES = ("image_clip_crop", "image_real_clip")


def axis_tables(in_size, out_size, filt, first, count):
    if in_size == out_size:                                   # Pillow skips the pass: the identity
        k = np.full((count, 1), 1 << IO.PRECISION_BITS, dtype=np.int32)
        b = np.stack([np.arange(first, first + count), np.ones(count, dtype=np.int64)], axis=1).astype(np.int32)
        return k, b
    k, b, _ = IO.coeffs(in_size, out_size, filt)
    return np.ascontiguousarray(k[first:first + count]), np.ascontiguousarray(b[first:first + count])


def clip_processor():
    try:
        import transformers
        for name in ("CLIPImageProcessorPil", "CLIPImageProcessor"):
            cls = getattr(transformers, name, None)
            if cls is None:
                continue
            try:
                return cls(), f"transformers {transformers.__version__} {name}"
            except Exception:
                continue
    except Exception:
        pass
    return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import PIL
    from PIL import Image
    resampling = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
    proc, proc_name = clip_processor()
    for name, (n, h, w, rh, rw, filt, window, seed) in CASES.items():
        top, left, wh, ww = window or (0, 0, rh, rw)
        inp = np.stack([IO.test_image(h, w, 100 * seed + i) for i in range(n)])
        pil = np.stack([np.asarray(Image.fromarray(im).resize((rw, rh), resampling[filt]))[top:top + wh, left:left + ww] for im in inp])
        kx, bx = axis_tables(w, rw, filt, left, ww)
        ky, by = axis_tables(h, rh, filt, top, wh)
        mine = np.stack([IO._pass(IO._pass(im, kx, bx, 1), ky, by, 0) for im in inp])
        diff = int((mine != pil).sum())
        if diff:
            raise SystemExit(f"{name}: the oracle differs from Pillow {PIL.__version__} in {diff} bytes — not written")
        meta = dict(filter=filt, in_h=h, in_w=w, resized_h=rh, resized_w=rw, window=[top, left, wh, ww], pillow=PIL.__version__)
        extra = {}
        if proc is not None and name in CLIP_CASES:
            try:
                pv = proc(images=[im for im in inp], return_tensors="np")["pixel_values"]
                extra["pixel_values"] = np.asarray(pv, dtype=np.float32)
                meta["pixel_values_from"] = proc_name
            except Exception as e:                                    # a processor that needs a backend this box lacks
                print(f"{name}: {proc_name} did not run ({type(e).__name__}: {e}); no pixel_values", file=sys.stderr)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, input=inp, output=pil, kx=kx, bx=bx, ky=ky, by=by, meta=json.dumps(meta), **extra)
        print(f"{name}: {inp.shape} -> {pil.shape}, 0 bytes differ from Pillow {PIL.__version__}, "
              f"{os.path.getsize(path)} bytes{', pixel_values' if extra else ''}")


if __name__ == "__main__":
    main()
