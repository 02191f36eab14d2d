"""GPU: rcdm_png_decode (csrc/png_decode.hip) and what rcdms_amd/image.py builds on it, against the goldens of
tools/mint_png_decode_golden.py (Pillow's pixels; the restatement tests/png_decode_oracle.py) with plain equality.

Every buffer of a call is guarded: the uploaded files sit between two canary bands and are checked unchanged; `dst` has a
padded row pitch and a gap in front of every image, and every byte outside the h x 3 w pixels of the good files must still
hold the canary afterwards — a file with a non-zero status writes nothing; the words around status[] are checked; the
workspace is filled with 0xEE first, so nothing may rely on what it held.  The corrupt files assert a REFUSAL: each gets the
same status from the same decoder core on the CPU (tests/test_png_decode_host.py; tools/png_decode_host_check.py runs that
program under AddressSanitizer + UBSan, tools/png_decode_standin.py the kernels themselves with a thread per lane)."""
import numpy as np
import pytest
import torch

from rcdms_amd import hip
from rcdms_amd import image as I
from tests import png_decode_oracle as D
from tests.test_hip_image import CANARY, DEV
from tests.test_hip_png import GUARD

pytestmark = pytest.mark.gpu


class Call:
    """One rcdm_png_decode call inside canary; .status [n] and .images (list of uint8 arrays, None where status != 0)."""

    def __init__(self, files, order="rgb", pad=13, gap=333):
        dec = I.png_decoder(DEV)
        plan = I.png_decode_plan(files, pitch=lambda w: 3 * w + pad, gap=gap)
        n = plan.n
        src_host = np.full(2 * GUARD + len(plan.src), CANARY, dtype=np.uint8)
        src_host[GUARD:GUARD + len(plan.src)] = plan.src
        src = torch.from_numpy(src_host).to(DEV)
        _, tables = dec.upload(plan)
        tables_before = tables.clone()
        ws = torch.full((plan.workspace_bytes,), 0xEE, dtype=torch.uint8, device=DEV)
        dst = torch.full((plan.dst_bytes,), CANARY, dtype=torch.uint8, device=DEV)
        status = torch.full((n + 2,), -1, dtype=torch.int32, device=DEV)
        dec.launch(plan, src[GUARD:GUARD + len(plan.src)], tables, ws, dst, status[1:1 + n], order)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert st[0] == -1 and st[-1] == -1, "the words around status[] were written"
        assert np.array_equal(src.cpu().numpy(), src_host), "the uploaded files changed"
        assert torch.equal(tables, tables_before), "the records changed"
        raw = dst.cpu().numpy()
        keep = np.ones(raw.shape, dtype=bool)
        self.status, self.images = st[1:1 + n], []
        for i, (h, w) in enumerate(plan.shapes):
            r = plan.records[i]
            if self.status[i]:
                self.images.append(None)
                continue
            rows = np.lib.stride_tricks.as_strided(raw[r.dst_offset:], (h, 3 * w), (r.dst_pitch, 1))
            np.lib.stride_tricks.as_strided(keep[r.dst_offset:], (h, 3 * w), (r.dst_pitch, 1))[:] = False
            self.images.append(rows.reshape(h, w, 3).copy())
        bad = (raw != CANARY) & keep
        assert not bad.any(), f"{int(bad.sum())} bytes written outside the images, first at {int(np.flatnonzero(bad)[0])}"


@pytest.mark.parametrize("name", [g for g in D.GOLDENS if g != "corrupt"])
def test_decode_equals_golden(hiplib, name):
    items, _ = D.golden(name)
    files = [data for _, data, _, _ in items]
    rgb, bgr = Call(files), Call(files, order="bgr", pad=0, gap=1)
    for k, (nm, _, _, want) in enumerate(items):
        assert rgb.status[k] == 0 and bgr.status[k] == 0, f"{nm}: {hip.PNG_STATUS.get(int(rgb.status[k]))}"
        assert np.array_equal(rgb.images[k], want), f"{nm}: {int((rgb.images[k] != want).sum())} bytes differ"
        assert np.array_equal(bgr.images[k], want[:, :, ::-1]), nm


def test_corrupt_files_are_refused(hiplib):
    items, _ = D.golden("corrupt")
    assert {st for _, _, st, _ in items} == set(range(1, 12)), "every RCDM_PNG_E* code"
    got = Call([data for _, data, _, _ in items])          # asserts that not one byte of dst was written
    for k, (nm, _, st, _) in enumerate(items):
        assert got.status[k] == st, f"{nm}: {hip.PNG_STATUS.get(int(got.status[k]), got.status[k])}, expected {D.STATUS_NAMES[st]}"


def test_reads_what_the_encoder_writes(hiplib):
    """Every file of the png_*.npz and pngm_*.npz goldens (literal-only and match mode, 2 x 8192 included) in one call."""
    items = D.written_goldens()
    assert any(px.shape[:2] == (2, 8192) for _, _, px in items) and len(items) > 30
    got = Call([data for _, data, _ in items], pad=3, gap=64)
    for k, (nm, _, want) in enumerate(items):
        assert got.status[k] == 0 and np.array_equal(got.images[k], want), nm


def test_64_mixed_files_two_corrupt_in_the_middle(hiplib):
    good = [it for g in ("small", "types", "crafted", "flat", "far") for it in D.golden(g)[0]] + D.golden("cartoon0")[0][1:2]
    corrupt = {nm: it for it in D.golden("corrupt")[0] for nm in [it[0]]}
    items = [good[k % len(good)] for k in range(62)]
    items[31:31] = [corrupt["distance_before_start"], corrupt["cut_10_bytes"]]
    assert len(items) == 64 and len({it[3].shape for it in items if it[3] is not None}) > 8
    got = Call([it[1] for it in items], pad=7, gap=100)
    for k, (nm, _, st, want) in enumerate(items):
        assert got.status[k] == st, f"file {k} ({nm})"
        if st == 0:
            assert np.array_equal(got.images[k], want), f"file {k} ({nm})"
    assert [k for k in range(64) if got.status[k]] == [31, 32]


def test_decode_png_and_load_png(hiplib, tmp_path):
    items = D.golden("types")[0] + D.golden("small")[0]
    files = [it[1] for it in items]
    frames = I.decode_png(files, check_crc=True)
    assert len(frames) == len(files) and all(f.is_cuda and f.dtype == torch.uint8 and f.is_contiguous() for f in frames)
    base = frames[0].data_ptr()
    for f, it in zip(frames, items):
        assert np.array_equal(f.cpu().numpy(), it[3]), it[0]
        assert f.data_ptr() == base, "views of one buffer with dense rows, in order"
        base += f.numel()
    one = I.decode_png(files[0], order="bgr")
    assert len(one) == 1 and np.array_equal(one[0].cpu().numpy(), items[0][3][:, :, ::-1])
    paths = []
    for k, data in enumerate(files[:3]):
        paths.append(tmp_path / f"{k}.png")
        paths[-1].write_bytes(data)
    for f, it in zip(I.load_png(paths, order="bgr"), items):
        assert np.array_equal(f.cpu().numpy(), it[3][:, :, ::-1])
    assert np.array_equal(I.load_png(str(paths[1]))[0].cpu().numpy(), items[1][3])
    same = I.decode_png([files[4]] * 3)                   # equal sizes: one (n, h, w, 3) view
    batch = I.PngDecoder.batch(same)
    assert batch.shape == (3, 131, 131, 3) and batch.data_ptr() == same[0].data_ptr()
    assert np.array_equal(batch.cpu().numpy(), np.stack([items[4][3]] * 3))


def test_decode_png_names_the_bad_file(hiplib):
    good = D.golden("small")[0][1][1]
    for nm, data, st, _ in D.golden("corrupt")[0]:
        with pytest.raises(hip.RcdmError, match=f"file 2: {D.STATUS_NAMES[st]}$"):
            I.decode_png([good, good, data, good])
    bad = bytearray(good)
    bad[-13] ^= 1
    with pytest.raises(ValueError, match="file 1: CRC"):
        I.decode_png([good, bytes(bad)], check_crc=True)
    assert len(I.decode_png([good, bytes(bad)])) == 2      # CRCs are the host's, and only on request


def test_round_trip_through_the_encoder(hiplib):
    x = np.load(D.GOLD + "/png_batch.npz")["input"]
    assert x.shape == (5, 105, 107, 3)
    dev = torch.from_numpy(x).to(DEV)
    for match in (False, True):
        frames = I.decode_png(I.encode_png(dev, match=match))
        assert torch.equal(I.PngDecoder.batch(frames), dev), f"match={match}"


def test_graph_replay_equals_eager(hiplib):
    items = D.golden("types")[0]
    dec = I.png_decoder(DEV)
    plan = I.png_decode_plan([it[1] for it in items])
    src, tables = dec.upload(plan)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(plan.dst_bytes, dtype=torch.uint8, device=DEV)
    status = torch.full((plan.n,), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = hip.Graph()
        g.begin()
        try:
            dec.launch(plan, src, tables, ws, dst, status)
        finally:
            g.end()
        s.synchronize()
        assert not bool(dst.any()) and bool((status == -1).all()), "capture must not execute"
        g.launch()
        s.synchronize()
    assert not bool(status.any())
    assert np.array_equal(dst.cpu().numpy(), np.concatenate([it[3].reshape(-1) for it in items]))


def test_a_decoded_strip_feeds_the_front_end(hiplib):
    """The h5 split's strip shape: frame 1 of a decoded 640 x 128 strip, sliced on the device, through ClipImageProcessor
    and FrameTransform — the same numbers as the same functions give for the numpy slice."""
    nm, data, _, want = D.golden("cartoon2")[0][0]
    assert want.shape == (640, 128, 3)
    strip = I.decode_png(data, order="bgr")[0]
    frame, ref = strip[128:256], np.ascontiguousarray(want[128:256, :, ::-1])
    proc, ft = I.ClipImageProcessor(device=DEV), I.FrameTransform(64, 64, device=DEV)
    assert torch.equal(proc(images=frame).pixel_values, proc(images=ref).pixel_values)
    assert torch.equal(ft(frame), ft(ref))
    assert torch.equal(proc.cropped_uint8(strip.view(5, 128, 128, 3)), proc.cropped_uint8(ref_all(want)))


def ref_all(want):
    return [np.ascontiguousarray(want[k * 128:(k + 1) * 128, :, ::-1]) for k in range(5)]
