"""CPU: the PNG reader without a device — the restatement tests/png_decode_oracle.py against Pillow and zlib on every
fixture of tools/mint_png_decode_golden.py, the host walk of rcdms_amd/image.py, the argument checks of rcdm_png_decode
(nothing is launched: the pointers are never dereferenced), and the shared core csrc/png_inflate.h itself, compiled into
tools/png_decode_host.cpp and run over every fixture, the corrupt ones included, and over every file the encoder's goldens
hold.  The format is integer arithmetic: every comparison is equality."""
import ctypes
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_decode_oracle as D
from tests import png_oracle as P
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", [g for g in D.GOLDENS if g != "corrupt"])
def test_oracle_equals_pillow(name):
    items, _ = D.golden(name)
    for nm, data, st, want in items:
        assert st == 0
        ref = pil_rgb(data)
        assert np.array_equal(ref, want), f"{nm}: Pillow and the golden"
        got_st, got = D.decode(data)
        assert got_st == 0 and np.array_equal(got, want), nm
        got_st, got = D.decode(data, "bgr")
        assert got_st == 0 and np.array_equal(got, want[:, :, ::-1]), nm


def test_fixture_facts():
    """What the fixtures are there for, from the goldens' own block lists [kind, matches, longest, farthest, overlapping]."""
    blocks = {}
    for g in D.GOLDENS[:-1]:
        blocks.update(D.golden(g)[1]["blocks"])
    kinds = lambda nm: [b[0] for b in blocks[nm]]
    assert kinds("1x1") == [1] and blocks["1x1"][0][1] == 0
    assert kinds("8x8_const") == [1] and blocks["8x8_const"][0][4] > 0
    assert blocks["16x16_const_l1"][0][2] == 258
    assert kinds("3x5_noise") == [0]
    assert set(kinds("cartoon0_l0")) == {0} and len(kinds("cartoon0_l0")) > 1
    for l in (1, 6, 9):
        b = blocks[f"cartoon0_l{l}"]
        assert max(x[2] for x in b) == 258 and max(x[3] for x in b) > 24576 and sum(x[4] for x in b) > 100
    assert len(kinds("cartoon2")) > 1 and set(kinds("cartoon2")) == {2}
    assert max(x[3] for x in blocks["far_39x1092"]) == 9 * (1 + 3 * 1092) and sum(x[4] for x in blocks["far_39x1092"]) == 0
    assert sum(x[1] for x in blocks["flat_300x300"]) > 1000
    assert kinds("edge_D32768") == [0, 1] and blocks["edge_D32768"][1][3] == 32768
    assert kinds("empty_stored") == [2, 0, 2]
    items = {nm: data for nm, data, _, _ in D.golden("crafted")[0] + D.golden("types")[0] + D.golden("cartoon2")[0]}
    assert [n for _, n in D.walk(items["rechunked"])["idats"]][:4] == [1, 7, 0, 4096]
    assert len(D.walk(items["cartoon2"])["idats"]) > 1
    types = np.frombuffer(zlib.decompress(D.zlib_stream(items["filters131_five"])), dtype=np.uint8).reshape(131, -1)[:, 0]
    assert np.bincount(types, minlength=5).min() > 0, "every filter type on some rows"
    assert [D.walk(items[k])["color_type"] for k in ("grey", "grey_alpha", "rgba", "palette17")] == [0, 4, 6, 3]


def test_crafted_streams_equal_zlib():
    for nm, data, st, want in D.golden("crafted")[0]:
        m = D.walk(data)
        raw = zlib.decompress(D.zlib_stream(data))
        got_st, got = D.inflate(D.zlib_stream(data), m["h"] * (1 + 3 * m["w"]))
        assert got_st == 0 and bytes(got) == raw, nm


def refused_elsewhere(data):
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


def test_corrupt_files_get_their_status():
    items, _ = D.golden("corrupt")
    assert {st for _, _, st, _ in items} == set(range(1, 12)), "every RCDM_PNG_E* code"
    for nm, data, st, _ in items:
        got, _ = D.decode(data)
        assert got == st, f"{nm}: {D.STATUS_NAMES[got]}, expected {D.STATUS_NAMES[st]}"
        assert refused_elsewhere(data), f"{nm}: zlib and Pillow both take it"
        for kind, body, stored, real in P.parse_chunks(data):
            assert stored == real, f"{nm}: CRC of {kind!r}"


def test_status_codes_are_the_headers():
    hip, _ = _lib()
    text = open(os.path.join(ROOT, "include", "rcdm.h")).read()
    for code, name in enumerate(D.STATUS_NAMES):
        if code:
            assert f"#define {name} {code} " in text and hip.PNG_STATUS[code] == name
    assert len(hip.PNG_STATUS) == len(D.STATUS_NAMES) - 1


def test_rechunk_keeps_the_stream():
    data = D.golden("types")[0][4][1]
    cut = D.rechunk(data, [1, 7, 0, 4096])
    assert D.zlib_stream(cut) == D.zlib_stream(data) and cut != data


# ------------------------------------------------------------------------------------------------ the host walk
def test_host_walk_and_plan():
    from rcdms_amd import hip
    from rcdms_amd import image as I
    files = [data for g in ("small", "types", "crafted") for _, data, _, _ in D.golden(g)[0]]
    plan = I.png_decode_plan(files)
    assert plan.n == len(files) and plan.n_idat == sum(len(D.walk(f)["idats"]) for f in files)
    ws_end = 0
    for i, f in enumerate(files):
        m, r = D.walk(f), plan.records[i]
        assert (r.w, r.h, r.color_type) == (m["w"], m["h"], m["color_type"]) and r.dst_pitch == 3 * r.w
        assert plan.src[r.src_offset:r.src_offset + r.src_bytes].tobytes() == f and r.src_offset % 16 == 0
        got = b"".join(f[plan.idats[k].offset:plan.idats[k].offset + plan.idats[k].bytes]
                       for k in range(r.idat_first, r.idat_first + r.idat_count))
        assert got == D.zlib_stream(f) and r.zlib_bytes == len(got)
        if m["color_type"] == 3:
            assert (r.plte_offset, 3 * r.plte_entries) == m["plte"]
        assert r.ws_offset == ws_end and r.ws_offset % 16 == 0
        ws_end += hip.png_file_workspace(r.zlib_bytes, r.h * (1 + D.BPP[r.color_type] * r.w))
    assert plan.workspace_bytes == ws_end and plan.dst_bytes == sum(3 * h * w for h, w in plan.shapes)


def _ihdr(data, **kw):
    w, h, depth, ct, comp, filt, il = struct.unpack(">IIBBBBB", data[16:29])
    f = dict(w=w, h=h, depth=depth, ct=ct, il=il)
    f.update(kw)
    body = struct.pack(">IIBBBBB", f["w"], f["h"], f["depth"], f["ct"], comp, filt, f["il"])
    return data[:8] + P.chunk(b"IHDR", body) + data[33:]


def test_host_walk_refuses_what_is_out_of_scope():
    from rcdms_amd import image as I
    good = D.golden("small")[0][1][1]
    pal = D.golden("types")[0][3][1]
    assert I.png_walk(good).idats
    with pytest.raises(NotImplementedError, match="file 3: Adam7"):
        I.png_walk(_ihdr(good, il=1), 3)
    with pytest.raises(NotImplementedError, match="file 1: bit depth 16"):
        I.png_decode_plan([good, _ihdr(good, depth=16)])
    with pytest.raises(NotImplementedError, match="file 0: bit depth 4"):
        I.png_walk(_ihdr(pal, depth=4))
    with pytest.raises(NotImplementedError, match="file 2: no IHDR"):
        I.png_walk(good[:8] + good[33:], 2)
    chunks = P.parse_chunks(good)
    no_idat = P.SIGNATURE + b"".join(P.chunk(k, b) for k, b, _, _ in chunks if k != b"IDAT")
    with pytest.raises(NotImplementedError, match="file 0: no IDAT"):
        I.png_walk(no_idat)
    no_plte = P.SIGNATURE + b"".join(P.chunk(k, b) for k, b, _, _ in P.parse_chunks(pal) if k != b"PLTE")
    with pytest.raises(NotImplementedError, match="file 5: colour type 3 without a PLTE"):
        I.png_walk(no_plte, 5)
    with pytest.raises(NotImplementedError, match="sides are 1..8192"):
        I.png_walk(_ihdr(good, w=8193))
    with pytest.raises(ValueError, match="not a PNG signature"):
        I.png_walk(b"GIF89a" + good[6:])
    with pytest.raises(ValueError, match="runs past the end"):
        I.png_walk(good[:-20])
    # ancillary chunks are skipped, tRNS included; CRCs only under check_crc
    extra = D.make_png(8, 8, 2, D.zlib_stream(good), extra=[(b"tRNS", b"\0\1\0\2\0\3"), (b"gAMA", struct.pack(">I", 45455))])
    assert I.png_walk(extra, check_crc=True).idats == [(o, n) for o, n in D.walk(extra)["idats"]]
    bad = bytearray(good)
    bad[-13] ^= 1                                          # the last byte of the IDAT chunk's CRC
    assert I.png_walk(bytes(bad)).idats
    with pytest.raises(ValueError, match="CRC of the b'IDAT' chunk"):
        I.png_walk(bytes(bad), check_crc=True)


def test_decode_png_has_no_cpu_path():
    import torch
    from rcdms_amd import hip
    from rcdms_amd import image as I
    if torch.cuda.is_available():
        return                                             # tests/test_hip_png_decode.py runs the calls
    with pytest.raises(hip.RcdmError):
        I.decode_png(D.golden("small")[0][0][1])


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in ("rcdm_png_decode", "rcdm_png_decode_workspace_bytes"):
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.PngFile) == 72 and ctypes.sizeof(hip.PngIdat) == 16


def test_decode_workspace_bytes():
    from rcdms_amd import image as I
    hip, lib = _lib()
    files = [data for _, data, _, _ in D.golden("small")[0] + D.golden("types")[0]]
    plan = I.png_decode_plan(files)
    assert hip.png_decode_workspace_bytes(plan.records, plan.n) == plan.workspace_bytes > 0
    assert lib.rcdm_png_decode_workspace_bytes(None, 1) == 0
    assert hip.png_decode_workspace_bytes(plan.records, 0) == 0
    for field, value in (("w", 8193), ("h", 0), ("color_type", 5), ("dst_pitch", 2), ("ws_offset", 8)):
        plan = I.png_decode_plan(files)
        setattr(plan.records[1], field, value)
        assert hip.png_decode_workspace_bytes(plan.records, plan.n) == 0, field


def test_decode_argument_checks():
    hip, lib = _lib()
    files, idats, src, ws, dst, status = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000    # never dereferenced
    call = lambda f=files, i=idats, n=1, ni=1, order=0, s=src, w=ws, d=dst, st=status: lib.rcdm_png_decode(f, i, n, ni, order, s, w, d, st, None)
    for k in ("f", "i", "s", "w", "d", "st"):
        assert call(**{k: None}) == EINVAL, k
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL and call(ni=0) == EINVAL
    assert call(n=65536, ni=65536) == ESHAPE
    assert call(order=2) == EINVAL and call(order=-1) == EINVAL
    assert call(w=ws + 8) == EINVAL                        # a misaligned workspace
    assert call(st=status + 2) == EINVAL                   # misaligned status
    assert call(f=files + 4) == EINVAL and call(i=idats + 4) == EINVAL


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/png_decode_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("pngd") / "png_decode_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "png_decode_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_tool(exe, tmp_path, files, bgr=False):
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"{i}.png"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + (["--bgr"] if bgr else []) + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(files)
    return [(int(a), int(b, 16), int(c), int(d)) for a, b, c, d in (ln.split() for ln in lines)]


def test_host_tool_on_every_fixture(host_tool, tmp_path):
    items = [it for g in D.GOLDENS for it in D.golden(g)[0]]
    got = run_tool(host_tool, tmp_path, [data for _, data, _, _ in items])
    got_bgr = run_tool(host_tool, tmp_path, [data for _, data, _, _ in items], bgr=True)
    for (nm, data, st, px), (gst, crc, w, h), (bst, bcrc, _, _) in zip(items, got, got_bgr):
        assert gst == st == bst, f"{nm}: {gst}, expected {D.STATUS_NAMES[st]}"
        if st == 0:
            assert (h, w) == px.shape[:2] and crc == zlib.crc32(px.tobytes()), nm
            assert bcrc == zlib.crc32(np.ascontiguousarray(px[:, :, ::-1]).tobytes()), nm


def test_host_tool_reads_what_the_encoder_writes(host_tool, tmp_path):
    items = D.written_goldens()
    assert any(px.shape[:2] == (2, 8192) for _, _, px in items) and len(items) > 30
    got = run_tool(host_tool, tmp_path, [data for _, data, _ in items])
    for (nm, data, px), (st, crc, w, h) in zip(items, got):
        assert st == 0 and (h, w) == px.shape[:2] and crc == zlib.crc32(px.tobytes()), nm
