"""Mint tests/golden/png_*.npz from the restatement of the PNG format (tests/png_oracle.py); the tests only read the files.

Each file holds `input` uint8 (n, h, w, 3), `files` uint8 (the n expected PNG files back to back), `sizes` int64 [n] and
`meta` (JSON: filter, Pillow version, per-case facts).  A file is written only if, for every image in it,
  - PIL.Image.open(...).load() gives mode RGB and exactly the input pixels,
  - zlib.decompress of the concatenated IDAT data equals the filtered stream,
  - every chunk's CRC equals zlib.crc32,
  - (png_limiter) the unlimited Huffman depth of its block really exceeds 15,
  - (png_filters) every one of the five filters wins some row.

    python tools/mint_png_golden.py [--out tests/golden]"""
import argparse
import io
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_oracle as P  # noqa: E402


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def five_filter_image(h=131, w=131, seed=7):
    """Bands of rows built so that each PNG filter is the cheapest somewhere: noise of -1 / 0 / 1 around zero (None), independent horizontal
    random walks from random levels (Sub), a noisy row repeated with small changes (Up), the mean of the left and the upper
    neighbour plus noise (Average), a plane rising along both (Paeth)."""
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w, 3), dtype=np.int64)
    edges = np.linspace(0, h, 6).astype(int)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(5):
        r0, r1 = edges[k], edges[k + 1]
        n = r1 - r0
        if k == 0:
            band = rng.randint(-1, 2, size=(n, w, 3))
        elif k == 1:
            band = rng.randint(0, 256, size=(n, 1, 3)) + np.cumsum(rng.randint(-2, 3, size=(n, w, 3)), axis=1)
        elif k == 2:
            band = rng.randint(0, 256, size=(1, w, 3)) + np.cumsum(rng.randint(-1, 2, size=(n, w, 3)), axis=0)
        elif k == 3:
            band = np.zeros((n, w, 3), dtype=np.int64)       # each byte: the mean of its left and upper neighbours + noise
            kick = rng.randint(-12, 13, size=(n, w, 3))
            for y in range(n):
                above = (img[r0 - 1] if y == 0 else band[y - 1]) & 255
                for x in range(w):
                    left = band[y, x - 1] & 255 if x else np.zeros(3, dtype=np.int64)
                    band[y, x] = ((left + above[x]) >> 1) + kick[y, x]
        else:
            band = (3 * xx[r0:r1] + 5 * yy[r0:r1])[:, :, None] + np.zeros((1, 1, 3), dtype=np.int64)
        img[r0:r1] = band
    return (img & 255).astype(np.uint8)


def limiter_image(seed=11):
    """128 x 85, filter 0: one block of exactly 32768 bytes whose literal counts grow by 1.8x per symbol — 17 literals and
    end-of-block chain into a tree 17 deep."""
    h, w = 128, 85
    counts = [int(round(1.8 ** k)) for k in range(17)]
    counts[0] = max(counts[0], 1)
    pixels = h * w * 3
    counts[-1] += pixels - sum(counts)                      # the filter bytes (128 zeros) add to symbol 0 on top
    assert counts[-1] > counts[-2]
    vals = np.repeat(np.arange(17), counts).astype(np.uint8)
    np.random.RandomState(seed).shuffle(vals)
    return vals.reshape(h, w, 3)


def cases():
    c = {}
    c["png_1x1"] = (noise(1, 1, 1)[None], -1)
    c["png_3x5"] = (noise(3, 5, 2)[None], -1)
    c["png_105x107"] = (P.cartoon(105, 107, 2.0, 3)[None], -1)
    c["png_256x85"] = (P.cartoon(256, 85, 2.0, 4)[None], -1)
    c["png_filters"] = (five_filter_image()[None], -1)
    c["png_limiter"] = (limiter_image()[None], 0)
    c["png_const"] = (np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (1, 64, 64, 3)).copy(), -1)
    c["png_const_black"] = (np.zeros((1, 64, 64, 3), dtype=np.uint8), 0)
    for f in range(5):
        c[f"png_noise_f{f}"] = (noise(40, 200, 5)[None], f)
    c["png_batch"] = (np.stack([P.cartoon(105, 107, [0.0, 0.5, 2.0, 6.0, 40.0][i], 20 + i) for i in range(5)]), -1)
    return c


def verify(name, img, filt, data):
    import PIL
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    if im.mode != "RGB" or not np.array_equal(np.asarray(im), img):
        raise SystemExit(f"{name}: Pillow {PIL.__version__} does not decode the file to the input — not written")
    chunks = P.parse_chunks(data)
    if any(stored != real for _, _, stored, real in chunks):
        raise SystemExit(f"{name}: a chunk CRC differs from zlib.crc32 — not written")
    stream, types = P.filter_stream(img, filt)
    if zlib.decompress(b"".join(body for kind, body, _, _ in chunks if kind == b"IDAT")) != stream.tobytes():
        raise SystemExit(f"{name}: zlib does not inflate the IDAT data to the filtered stream — not written")
    if P.png_size(img, filt) != len(data) or len(data) > P.bound(*img.shape[:2]):
        raise SystemExit(f"{name}: png_size / bound disagree with the packed file — not written")
    facts = {"filter_rows": np.bincount(types, minlength=5).tolist()}
    if name == "png_limiter":
        hist = np.bincount(stream, minlength=256)
        depth = int(P.huffman_depths(np.concatenate([hist, [1]])).max())
        lens, halvings = P.code_lengths(hist)
        if depth <= 15 or halvings < 1 or lens.max() > 15 or P.kraft(lens)[0] != P.kraft(lens)[1]:
            raise SystemExit(f"{name}: unlimited depth {depth}, {halvings} halvings — the limiter case does not limit; not written")
        facts.update(unlimited_depth=depth, halvings=halvings)
    if name == "png_filters" and min(facts["filter_rows"]) == 0:
        raise SystemExit(f"{name}: filters win {facts['filter_rows']} rows — one never wins; not written")
    return facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import PIL
    for name, (inp, filt) in cases().items():
        files = [P.encode(im, filt) for im in inp]
        facts = [verify(name, im, filt, f) for im, f in zip(inp, files)]
        meta = dict(filter=filt, pillow=PIL.__version__, facts=facts)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, input=inp, files=np.frombuffer(b"".join(files), dtype=np.uint8),
                            sizes=np.asarray([len(f) for f in files], dtype=np.int64), meta=json.dumps(meta))
        print(f"{name}: {inp.shape} filter {filt} -> {[len(f) for f in files]} bytes, {facts[0]}, npz {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
