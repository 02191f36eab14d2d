"""Mint tests/golden/pngm_*.npz from the restatement of the match mode (tests/png_match_oracle.py); the tests only read them.

The layout is that of tools/mint_png_golden.py: `input` uint8 (n, h, w, 3), `files` uint8 (the n expected PNG files back to
back), `sizes` int64 [n], `meta` (JSON: filter, Pillow version, per-image facts).  A file is written only if, for every image,
  - PIL.Image.open(...).load() gives mode RGB and exactly the input pixels,
  - zlib.decompress of the concatenated IDAT data equals the filtered stream, and every chunk's CRC equals zlib.crc32,
  - png_size agrees with the packed file, which is no longer than the literal-only file and within rcdm_png_bound,
and the case has the property it is there for:
  pngm_1x1, pngm_3x5   no usable match: the bytes are the literal-only file's
  pngm_black           64x64 black: 258-capped matches at distance 1 across rows, ONE used distance symbol
  pngm_w1 / w2 / w3    40 rows of width 1, 2, 3: duplicate candidate distances
  pngm_105x107         two blocks; a match cut short by the block boundary and a match whose source lies in front of it
  pngm_256x85          flat top half, uniform noise below: a match-form and a literal-form block in one file
  pngm_300x85          the same over three blocks (the third is short)
  pngm_2x8192          rows of 24577 bytes: the candidate 2 S is dropped, S + 3 is kept; the second row matches the first at S
  pngm_batch           five 105x107 frames, noise of 0 / 0.25 / 0.5 / 2 / 40 grey levels: five different sizes
  pngm_f0 .. f4        one flat 33x31 image under each fixed filter
  pngm_limiter         128x85, filter 0: 17 literals with counts growing 1.8x, laid out so that no candidate distance repeats
                       four bytes, then a run of zeros: the block takes the match form AND its literal / length tree is
                       deeper than 15 before the limiter

    python tools/mint_png_match_golden.py [--out tests/golden]"""
import argparse
import io
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_match_oracle as M  # noqa: E402
from tests import png_oracle as P  # noqa: E402


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def half_noise(h, w, seed):
    img = P.cartoon(h, w, 0.0, seed)
    img[h // 2:] = noise(h - h // 2, w, seed + 100)
    return img


def limiter_image(ratio=1.8, nsym=17):
    """128 x 85 for filter 0 (rows of 256 stream bytes): symbols 1..nsym with counts ratio^k, the most frequent remaining one
    first unless it would make a third equal byte in a row at one of the candidate distances; zeros behind them."""
    h, w = 128, 85
    cand = M.candidates(1 + 3 * w)
    left = [max(1, int(round(ratio ** k))) for k in range(nsym)]
    st = np.zeros(h * (1 + 3 * w), dtype=np.uint8)
    run = {d: 0 for d in cand}
    i = 0
    while sum(left):
        pick = 0                                            # the filter byte of a row
        if i % (1 + 3 * w):
            bad = {int(st[i - d]) for d in cand if d <= i and run[d] >= 2}
            order = sorted((k for k in range(nsym) if left[k]), key=lambda k: -left[k])
            k = ([k for k in order if k + 1 not in bad] or order)[0]
            left[k] -= 1
            pick = k + 1
        st[i] = pick
        for d in cand:
            run[d] = run[d] + 1 if d <= i and st[i - d] == pick else 0
        i += 1
    return st.reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3).copy()


def cases():
    c = {}
    c["pngm_1x1"] = (noise(1, 1, 1)[None], -1)
    c["pngm_3x5"] = (noise(3, 5, 2)[None], -1)
    c["pngm_black"] = (np.zeros((1, 64, 64, 3), dtype=np.uint8), -1)
    for w in (1, 2, 3):
        c[f"pngm_w{w}"] = (P.cartoon(40, w, 0.0, 5)[None], -1)
    c["pngm_105x107"] = (P.cartoon(105, 107, 0.0, 3)[None], -1)
    c["pngm_256x85"] = (half_noise(256, 85, 4)[None], -1)
    c["pngm_300x85"] = (half_noise(300, 85, 8)[None], -1)
    c["pngm_2x8192"] = (P.cartoon(2, 8192, 0.0, 6)[None], -1)
    c["pngm_batch"] = (np.stack([P.cartoon(105, 107, s, 20 + i) for i, s in enumerate([0.0, 0.25, 0.5, 2.0, 40.0])]), -1)
    for f in range(5):
        c[f"pngm_f{f}"] = (P.cartoon(33, 31, 0.0, 7)[None], f)
    c["pngm_limiter"] = (limiter_image()[None], 0)
    return c


def fail(name, what):
    raise SystemExit(f"{name}: {what} — not written")


def verify(name, img, filt, data):
    import PIL
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    if im.mode != "RGB" or not np.array_equal(np.asarray(im), img):
        fail(name, f"Pillow {PIL.__version__} does not decode the file to the input")
    chunks = P.parse_chunks(data)
    if any(stored != real for _, _, stored, real in chunks):
        fail(name, "a chunk CRC differs from zlib.crc32")
    stream, _ = P.filter_stream(img, filt)
    if zlib.decompress(b"".join(body for kind, body, _, _ in chunks if kind == b"IDAT")) != stream.tobytes():
        fail(name, "zlib does not inflate the IDAT data to the filtered stream")
    literal = P.encode(img, filt)
    if M.png_size(img, filt) != len(data) or len(data) > len(literal) or len(data) > P.bound(*img.shape[:2]):
        fail(name, "png_size / the literal-only size / the bound disagree with the packed file")
    h, w, _ = img.shape
    row = 1 + 3 * w
    forms = M.block_choice(img, filt)
    facts = {"match_form": [bool(f) for f in forms], "literal_bytes": len(literal)}
    parses = [M.parse_block(stream, b0, min(b0 + P.BLOCK, len(stream)), row) for b0 in range(0, len(stream), P.BLOCK)]
    dists = sorted({d for p in parses for _, _, d in p if d})
    facts["distances"] = dists
    if name in ("pngm_1x1", "pngm_3x5") and (any(forms) or data != literal):
        fail(name, "a block took the match form")
    if name == "pngm_black":
        lens = [n for _, n, d in parses[0] if d]
        if dists != [1] or lens.count(258) < 40 or not forms[0]:
            fail(name, f"distances {dists}, {lens.count(258)} capped matches")
    if name == "pngm_105x107":
        cut = parses[0][-1]
        longer = M.match_at(stream, cut[0], len(stream), row)[0]
        back = [t for t in parses[1] if t[2] and t[0] - t[2] < P.BLOCK]
        if len(forms) != 2 or not all(forms) or not cut[2] or longer <= cut[1] or not back:
            fail(name, f"last token of block 0 {cut} (uncut length {longer}), {len(back)} matches reading back")
        facts.update(cut=list(cut), uncut_length=longer, reading_back=len(back))
    if name in ("pngm_256x85", "pngm_300x85") and (len(forms) != (2 if name == "pngm_256x85" else 3) or all(forms) or not any(forms)):
        fail(name, f"block forms {forms}: both forms must occur")
    if name == "pngm_2x8192" and (2 * row <= M.WINDOW or row + 3 > M.WINDOW or row not in dists or not all(forms)):
        fail(name, f"distances {dists}")
    if name == "pngm_limiter":
        ll, dd, _ = M.match_counts(stream, parses[0])
        depth = int(P.huffman_depths(ll).max())
        lens, halvings = M.limited_lengths(ll)
        if not forms[0] or depth <= 15 or halvings < 1 or lens.max() > 15 or P.kraft(lens)[0] != P.kraft(lens)[1]:
            fail(name, f"match form {forms[0]}, unlimited depth {depth}, {halvings} halvings")
        facts.update(unlimited_depth=depth, halvings=halvings)
    return facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import PIL
    for name, (inp, filt) in cases().items():
        files = [M.encode(im, filt) for im in inp]
        facts = [verify(name, im, filt, f) for im, f in zip(inp, files)]
        if name == "pngm_batch" and len({len(f) for f in files}) != len(files):
            fail(name, "two files of the batch have one size")
        meta = dict(filter=filt, pillow=PIL.__version__, facts=facts)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, input=inp, files=np.frombuffer(b"".join(files), dtype=np.uint8),
                            sizes=np.asarray([len(f) for f in files], dtype=np.int64), meta=json.dumps(meta))
        print(f"{name}: {inp.shape} filter {filt} -> {[len(f) for f in files]} bytes, {facts[0]}, npz {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
