"""Mint tests/golden/pngd_*.npz: PNG files as bytes, the RGB pixels they decode to and the status the reader gives each
(include/rcdm.h, "PNG, reading").  The tests only read the goldens; the bytes are pinned because what zlib emits depends on
its version.

Each golden holds `files` uint8 (the files back to back), `sizes` int64 [n], `status` int32 [n], `shapes` int32 [n][2] (h, w),
`pixels` uint8 (the h * w * 3 bytes of every file with status 0, back to back), `names` and `meta` (JSON: Pillow / zlib
versions, the deflate blocks of each file as [kind, matches, longest, farthest, overlapping]).  A golden is written only if
  - Pillow decodes every good file and `convert("RGB")` gives exactly `pixels`,
  - the restatement tests/png_decode_oracle.py gives every file its status and the good ones the same pixels,
  - every crafted stream equals what zlib.decompress makes of it,
  - the facts asserted per fixture below hold (block kinds, distances, overlaps, filter types).

    python tools/mint_png_decode_golden.py [--out tests/golden]"""
import argparse
import io
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_decode_oracle as D  # noqa: E402
from tests import png_oracle as P  # noqa: E402


def noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def pil_png(arr, mode=None, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "PNG", **kw)
    return buf.getvalue()


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def blocks_of(data):
    m = D.walk(data)
    blocks = []
    D.inflate(D.zlib_stream(data), m["h"] * (1 + D.BPP[m["color_type"]] * m["w"]), blocks)
    return blocks


def filter_types(data):
    m = D.walk(data)
    raw = zlib.decompress(D.zlib_stream(data))
    return np.frombuffer(raw, dtype=np.uint8).reshape(m["h"], -1)[:, 0]


def raw_rows(img):
    """uint8 (h, w, 3) -> the filtered stream under filter 0"""
    h, w, _ = img.shape
    return np.concatenate([np.zeros((h, 1), dtype=np.uint8), img.reshape(h, 3 * w)], axis=1).tobytes()


# ------------------------------------------------------------------------------------------------ fixtures
def small():
    out = [("1x1", pil_png(noise((1, 1, 3), 1))),
           ("8x8_const", pil_png(np.full((8, 8, 3), (200, 100, 50), dtype=np.uint8))),
           ("16x16_const_l1", pil_png(np.full((16, 16, 3), (9, 99, 199), dtype=np.uint8), compress_level=1)),
           ("3x5_noise", pil_png(noise((3, 5, 3), 2), compress_level=0))]
    b = [blocks_of(f) for _, f in out]
    assert [k[0] for k in b[0]] == [1] and b[0][0][1] == 0, b[0]
    assert [k[0] for k in b[1]] == [1] and b[1][0][4] > 0, b[1]              # fixed, overlapping matches
    assert [k[0] for k in b[2]] == [1] and b[2][0][2] == 258, b[2]
    assert [k[0] for k in b[3]] == [0], b[3]
    return out


def types():
    h, w = 37, 41
    g = noise((h, w), 3)
    la = noise((h, w, 2), 4)
    rgba = noise((h, w, 4), 5)
    from PIL import Image
    pal = Image.fromarray(noise((h, w), 6) % 17, "P")
    pal.putpalette(noise((17, 3), 7).reshape(-1).tolist())
    buf = io.BytesIO()
    pal.save(buf, "PNG")
    filt = np.load(os.path.join(ROOT, "tests", "golden", "png_filters.npz"))["input"][0]
    # Pillow's own writer never chooses Average (not on this image, not on any other input of the goldens): its file
    # covers four filter types, and the same image under the project's adaptive filter choice (all five, tests/png_oracle.py),
    # deflated by zlib at level 9, covers the fifth
    stream, _ = P.filter_stream(filt)
    out = [("grey", pil_png(g)), ("grey_alpha", pil_png(la)), ("rgba", pil_png(rgba)), ("palette17", buf.getvalue()),
           ("filters131", pil_png(filt)), ("filters131_five", D.make_png(131, 131, 2, zlib.compress(stream.tobytes(), 9)))]
    assert [D.walk(f)["color_type"] for _, f in out] == [0, 4, 6, 3, 2, 2]
    assert D.walk(out[3][1])["plte"][1] == 17 * 3
    assert (np.bincount(filter_types(out[4][1]), minlength=5) > 0).sum() >= 4
    assert np.bincount(filter_types(out[5][1]), minlength=5).min() > 0, "every filter type on some row"
    return out


def cartoon0():
    img = P.cartoon(640, 128, 0.0, 71)
    out = [(f"cartoon0_l{l}", pil_png(img, compress_level=l)) for l in (0, 1, 6, 9)]
    b = [blocks_of(f) for _, f in out]
    assert all(k[0] == 0 for k in b[0]) and len(b[0]) > 1 and len(D.walk(out[0][1])["idats"]) > 1
    for k in b[1:]:
        assert any(x[0] == 2 and x[2] == 258 and x[3] > 24576 and x[4] > 100 for x in k), k
    return out


def cartoon2():
    out = [("cartoon2", pil_png(P.cartoon(640, 128, 2.0, 72)))]
    b = blocks_of(out[0][1])
    assert len(b) > 1 and all(k[0] == 2 for k in b) and max(k[3] for k in b) > 24576 and len(D.walk(out[0][1])["idats"]) > 1
    return out


def far():
    rows = noise((9, 1092, 3), 8)
    img = np.concatenate([rows] * 5)[:39]
    out = [("far_39x1092", pil_png(img, compress_level=9))]
    b = blocks_of(out[0][1])
    assert sum(k[1] for k in b) > 300 and max(k[3] for k in b) == 9 * (1 + 3 * 1092) and sum(k[4] for k in b) == 0, b
    return out


def flat():
    out = [("flat_300x300", pil_png(np.full((300, 300, 3), (31, 41, 59), dtype=np.uint8), compress_level=9))]
    b = blocks_of(out[0][1])
    assert sum(k[1] for k in b) > 1000 and sum(k[4] for k in b) > 0.5 * sum(k[1] for k in b), b
    return out


def crafted(rechunk_of):
    out = []

    def add(name, img, deflate):
        raw = raw_rows(img)
        z = D.zlib_wrap(deflate.tobytes(), raw)
        assert zlib.decompress(z) == raw, name
        out.append((name, D.make_png(img.shape[1], img.shape[0], 2, z)))

    # the window's far edge: a stored block of 32768 bytes, then row 0 again from D = 32768
    rows = noise((8, 1365, 3), 9)
    img = np.concatenate([rows, rows[:1]])
    raw = raw_rows(img)
    assert len(raw) == 9 * 4096
    add("edge_D32768", img, D.Deflate().stored(raw[:32768]).fixed([(258, 32768)] * 15 + [(226, 32768)], final=True))
    assert max(k[3] for k in blocks_of(out[-1][1])) == 32768
    # D = 1 with L = 258, D = 2 with L = 3
    img = np.zeros((3, 29, 3), dtype=np.uint8)
    img.reshape(-1)[-5:] = [7, 9, 7, 9, 7]
    add("D1_L258", img, D.Deflate().fixed([0, (258, 1), 7, 9, (3, 2)], final=True))
    # an empty stored block between two dynamic blocks
    img = noise((4, 4, 3), 10)
    raw = raw_rows(img)
    add("empty_stored", img, D.Deflate().dynamic(list(raw[:26])).stored(b"").dynamic(list(raw[26:]), final=True))
    # a dynamic block with ONE distance code (length 1: the incomplete set deflate allows)
    img = np.tile(noise((5, 1, 3), 11), (1, 5, 1))
    tokens = []
    for r in range(5):
        tokens += [0, *img[r, 0].tolist(), (12, 3)]
    add("one_distance_code", img, D.Deflate().dynamic(tokens, final=True))
    # a dynamic block with no distance code at all
    img = noise((3, 5, 3), 12)
    add("no_distance_code", img, D.Deflate().dynamic(list(raw_rows(img)), final=True))
    # IDATs of 1, 7, 0, 4096 and the remaining bytes
    out.append(("rechunked", D.rechunk(rechunk_of, [1, 7, 0, 4096])))
    assert [n for _, n in D.walk(out[-1][1])["idats"]][:4] == [1, 7, 0, 4096] and len(D.walk(out[-1][1])["idats"]) == 5
    return out


def corrupt(stored_3x5, fixed_8x8, filters131):
    """(name, file, status): each derived from a small golden or written with its geometry; CRCs right in all of them."""
    z8 = D.zlib_stream(fixed_8x8)
    raw8 = zlib.decompress(z8)
    z131 = D.zlib_stream(filters131)
    z35 = bytearray(D.zlib_stream(stored_3x5))
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    raw = raw_rows(img)

    def png8(deflate, wrap_raw=raw):
        return D.make_png(8, 8, 2, D.zlib_wrap(deflate.tobytes(), wrap_raw))

    out = [("cut_10_bytes", D.set_stream(filters131, z131[:-10]), D.ETRUNC)]
    out.append(("distance_before_start", png8(D.Deflate().fixed([0, 1, 2, (5, 4)] + list(raw[8:]), final=True)), D.EDISTANCE))
    out.append(("block_type_3", png8(D.Deflate().fixed(list(raw[:100])).reserved()), D.EBLOCK))
    z = bytearray(z35)
    assert z[2] == 1 and (z[3] | z[4] << 8) == len(z) - 11                 # one final stored block
    z[5] ^= 0x10
    out.append(("stored_nlen", D.set_stream(stored_3x5, bytes(z)), D.ESTORED))
    lens = [0] * 257
    lens[0] = lens[1] = lens[256] = 1                                       # three codes of one bit
    out.append(("oversubscribed", png8(D.Deflate().dynamic([0, 1, 0], final=True, lit_lens=lens, dist_lens=[0])), D.ECODES))
    out.append(("length_symbol_286", png8(D.Deflate().fixed([0, 0, 0, ("lit", 286)], final=True)), D.ESYMBOL))
    out.append(("distance_symbol_30", png8(D.Deflate().fixed([0, 0, 0, ("lit", 257), ("dist", 30)], final=True)), D.ESYMBOL))
    out.append(("height_one_less", D.set_height(fixed_8x8, 7), D.EOVERRUN))
    out.append(("height_one_more", D.set_height(fixed_8x8, 9), D.EUNDERRUN))
    bad = bytearray(raw8)
    bad[3 * 25] = 5
    out.append(("filter_byte_5", D.set_stream(fixed_8x8, zlib.compress(bytes(bad))), D.EFILTER))
    z = bytearray(z8)
    z[-1] ^= 1
    out.append(("adler", D.set_stream(fixed_8x8, bytes(z)), D.EADLER))
    z = bytearray(z8)
    z[0], z[1] = 0x88, 0x1C                                                 # a 64 K window; the header checksum holds
    assert (z[0] << 8 | z[1]) % 31 == 0
    out.append(("zlib_window_64k", D.set_stream(fixed_8x8, bytes(z)), D.EZLIB))
    assert {s for _, _, s in out} == set(range(1, 12)), "every status code"
    return out


def refused_elsewhere(data):
    """zlib refuses the stream, or inflates it to another size than the IHDR's, or Pillow refuses the file."""
    m = D.walk(data)
    try:
        raw = zlib.decompress(D.zlib_stream(data))
    except zlib.error:
        return True
    if len(raw) != m["h"] * (1 + D.BPP[m["color_type"]] * m["w"]):
        return True
    try:
        pil_rgb(data)
    except Exception:
        return True
    return False


def write(out_dir, name, items):
    import PIL
    files, status, shapes, pixels, meta = [], [], [], [], {"pillow": PIL.__version__, "zlib": zlib.ZLIB_RUNTIME_VERSION, "blocks": {}}
    for it in items:
        nm, data, want = it if len(it) == 3 else (*it, D.OK)
        m = D.walk(data)
        st, px = D.decode(data)
        assert st == want, f"{nm}: the oracle says {D.STATUS_NAMES[st]}, expected {D.STATUS_NAMES[want]}"
        for kind, body, stored, real in P.parse_chunks(data):
            assert stored == real, nm
        if want == D.OK:
            ref = pil_rgb(data)
            assert np.array_equal(px, ref), f"{nm}: the oracle and Pillow disagree"
            pixels.append(ref.reshape(-1))
            meta["blocks"][nm] = blocks_of(data)
        else:
            assert refused_elsewhere(data), f"{nm}: neither zlib nor Pillow refuses it"
        files.append(np.frombuffer(data, dtype=np.uint8))
        status.append(want)
        shapes.append((m["h"], m["w"]))
    path = os.path.join(out_dir, f"pngd_{name}.npz")
    np.savez_compressed(path, files=np.concatenate(files), sizes=np.asarray([len(f) for f in files], dtype=np.int64),
                        status=np.asarray(status, dtype=np.int32), shapes=np.asarray(shapes, dtype=np.int32),
                        pixels=np.concatenate(pixels) if pixels else np.zeros(0, dtype=np.uint8),
                        names=np.asarray([it[0] for it in items]), meta=json.dumps(meta))
    print(f"{path}: {len(items)} files, {os.path.getsize(path)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    out_dir = ap.parse_args().out
    s, t = small(), types()
    write(out_dir, "small", s)
    write(out_dir, "types", t)
    write(out_dir, "cartoon0", cartoon0())
    write(out_dir, "cartoon2", cartoon2())
    write(out_dir, "far", far())
    write(out_dir, "flat", flat())
    write(out_dir, "crafted", crafted(t[4][1]))
    write(out_dir, "corrupt", corrupt(s[3][1], s[1][1], t[4][1]))


if __name__ == "__main__":
    main()
