"""CPU: the host side of the image front / back end (rcdms_amd/image.py, csrc/image.hip's argument checks).
  - tests/image_oracle.py (the numpy restatement of Pillow's 8-bit resample) equals every golden minted from Pillow
    (tools/mint_image_golden.py) byte for byte, and live Pillow where it imports;
  - rcdms_amd.image.resample_tables (vectorised) equals the goldens' integer tables exactly;
  - the shortest-edge / centre-crop geometry;
  - both entry points refuse bad descriptors before they touch a device;
  - checkpoint.image_grid takes uint8 tiles."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

from rcdms_amd import hip
from rcdms_amd import image as I
from tests import image_oracle as IO

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "image_*.npz")))


def golden(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g, json.loads(str(g["meta"]))


def test_goldens_present():
    assert len(NAMES) == 9, NAMES


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_pillow_golden(name):
    g, m = golden(name)
    top, left, wh, ww = m["window"]
    for inp, want in zip(g["input"], g["output"]):
        got = IO.resize(inp, (m["resized_w"], m["resized_h"]), m["filter"])[top:top + wh, left:left + ww]
        assert got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())
    assert int((g["input"] == 0).sum()) and int((g["input"] == 255).sum())      # the saturated quadrant
    if m["filter"] == "bicubic" and m["resized_w"] > m["in_w"]:                 # enlarged: its overshoot reaches both clips
        assert int((g["output"] == 0).sum()) and int((g["output"] == 255).sum())


@pytest.mark.parametrize("h,w,oh,ow,filt", [(37, 53, 16, 24, "bilinear"), (37, 53, 16, 24, "bicubic"), (64, 64, 64, 224, "bicubic"),
                                            (333, 500, 149, 224, "bicubic"), (13, 7, 29, 31, "bilinear")])
def test_oracle_equals_live_pillow(h, w, oh, ow, filt):
    try:
        from PIL import Image
    except ImportError:
        return      # the goldens above are the pin where Pillow is absent
    img = IO.test_image(h, w, 17)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), getattr(Image.Resampling, filt.upper())))
    assert np.array_equal(IO.resize(img, (ow, oh), filt), want)
    box = (1.5, 2.0, w - 3.25, h - 1.0)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), getattr(Image.Resampling, filt.upper()), box=box))
    assert np.array_equal(IO.resize(img, (ow, oh), filt, box=box), want)


@pytest.mark.parametrize("name", NAMES)
def test_resample_tables_equal_golden_tables(name):
    g, m = golden(name)
    top, left, wh, ww = m["window"]
    tx = I.resample_tables(m["in_w"], m["resized_w"], m["filter"], window=(left, ww))
    ty = I.resample_tables(m["in_h"], m["resized_h"], m["filter"], window=(top, wh))
    for got, want in ((tx.k, g["kx"]), (tx.bounds, g["bx"]), (ty.k, g["ky"]), (ty.bounds, g["by"])):
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    assert tx.taps == g["kx"].shape[1] and ty.taps == g["ky"].shape[1]


def test_resample_tables_box_and_limits():
    k, b, taps = IO.coeffs(53, 24, "bicubic", box=(1.5, 49.75))
    t = I.resample_tables(53, 24, "bicubic", box=(1.5, 49.75))
    assert t.taps == taps and np.array_equal(t.k, k) and np.array_equal(t.bounds, b)
    t = I.resample_tables(64, 64, "bicubic", window=(3, 5))                   # a skipped pass: the identity
    assert t.taps == 1 and t.k.tolist() == [[1 << 22]] * 5 and t.bounds.tolist() == [[3 + i, 1] for i in range(5)]
    assert I.resample_tables(1024, 128, "bicubic").taps == 33                 # 8x bicubic reduction: inside the 40-tap limit
    assert I.resample_tables(1024, 128, 3).taps == 33                         # PIL.Image.Resampling.BICUBIC
    assert I.tile_rows(I.resample_tables(128, 512, "bilinear").bounds) == 10
    with pytest.raises(ValueError):
        I.resample_tables(64, 32, "lanczos")
    with pytest.raises(ValueError):
        I.resample_tables(64, 32, "bicubic", window=(30, 3))


def test_clip_geometry():
    assert I.clip_geometry(200, 300, 224, 224) == IO.clip_geometry(200, 300, 224, 224) == (224, 336, 0, 56)
    assert I.clip_geometry(300, 200, 224, 224) == IO.clip_geometry(300, 200, 224, 224) == (336, 224, 56, 0)
    assert I.clip_geometry(128, 128, 224, 224) == IO.clip_geometry(128, 128, 224, 224) == (224, 224, 0, 0)
    assert I.clip_geometry(75, 100, 56, 56) == (56, 74, 0, 9)                  # int(56 * 100 / 75) = 74: truncated, not rounded
    with pytest.raises(ValueError):
        I.clip_geometry(64, 64, 32, 56)


@pytest.mark.parametrize("name", ["image_clip_crop", "image_real_clip"])
def test_pixel_values_match_transformers_where_minted(name):
    g, m = golden(name)
    u8, pv = IO.clip_pixel_values(g["input"][0])
    assert np.array_equal(u8, g["output"][0])
    assert np.abs(IO.normalize_f32(u8, IO.CLIP_MEAN, IO.CLIP_STD) - pv).max() <= 1e-6
    if "pixel_values" in g.files:           # minted where transformers' PIL-backed processor imports
        assert np.abs(g["pixel_values"][0].astype(np.float64) - pv).max() <= 1e-6


def test_frames_u8_oracle_is_the_torch_sequence():
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = bits[torch.isfinite(bits) & (bits.abs() <= 1.25)]
    want = ((x.float() / 2 + 0.5).clamp(0, 1).numpy() * 255).astype(np.uint8)
    assert np.array_equal(IO.frames_u8(x.float().numpy()), want) and set(np.unique(want)) == set(range(256))
    assert IO.frames_u8(np.array([np.nan, np.inf, -np.inf], dtype=np.float32)).tolist() == [0, 255, 0]


def _resample_desc(**kw):
    d = hip.ResampleDesc()
    d.n, d.channels, d.in_h, d.in_w, d.out_h, d.out_w = 1, 3, 16, 16, 32, 32
    d.taps_x = d.taps_y = 5
    d.tile_rows, d.mode = 16, hip.IMAGE_U8
    d.src_pitch, d.dst_pitch = 48, 96
    d.std[:] = [1.0, 1.0, 1.0]
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_reject_without_a_device():
    lib = hip.load()
    P = 4096                                                    # never dereferenced: every case returns before a launch
    call = lambda d: lib.rcdm_image_resample(ctypes.byref(d), P, P, P, P, P, P, 0)
    assert lib.rcdm_image_resample(None, P, P, P, P, P, P, 0) == -1
    for i in range(6):                                          # each null pointer
        args = [P] * 6
        args[i] = 0
        assert lib.rcdm_image_resample(ctypes.byref(_resample_desc()), *args, 0) == -1
    assert call(_resample_desc(taps_x=41)) == -2 and call(_resample_desc(taps_y=41)) == -2
    assert call(_resample_desc(channels=4)) == -2 and call(_resample_desc(channels=1)) == -2
    assert call(_resample_desc(in_w=8193, src_pitch=3 * 8193)) == -2
    assert call(_resample_desc(src_pitch=47)) == -1 and call(_resample_desc(dst_pitch=95)) == -1
    assert call(_resample_desc(mode=3)) == -1 and call(_resample_desc(tile_rows=0)) == -1
    assert call(_resample_desc(mode=hip.IMAGE_F16_ROWS, ld=8, c_pad=4)) == -1          # pad channels in whole 16-byte stores
    assert call(_resample_desc(mode=hip.IMAGE_F32_NCHW, std=(ctypes.c_float * 3)(1.0, 0.0, 1.0))) == -1
    assert call(_resample_desc(tile_rows=700)) == -2                                    # more LDS than a block has
    d = _resample_desc()
    assert hip.image_resample_lds_bytes(d) == (32 * 5 * 2 + 4 * 32) * 4 + 16 * 96
    assert hip.image_resample_lds_bytes(_resample_desc(taps_x=41)) == 0

    f = lambda **kw: hip.FramesU8Desc(**{**dict(dst_pitch=96, dst_stride=0, n=1, H=8, W=32, channels=3, src_kind=0, ld=8), **kw})
    assert lib.rcdm_frames_to_u8(None, P, P, 0) == -1
    assert lib.rcdm_frames_to_u8(ctypes.byref(f()), 0, P, 0) == -1 and lib.rcdm_frames_to_u8(ctypes.byref(f()), P, 0, 0) == -1
    assert lib.rcdm_frames_to_u8(ctypes.byref(f(channels=4)), P, P, 0) == -2
    assert lib.rcdm_frames_to_u8(ctypes.byref(f(dst_pitch=95)), P, P, 0) == -1
    assert lib.rcdm_frames_to_u8(ctypes.byref(f(ld=2)), P, P, 0) == -1
    assert lib.rcdm_frames_to_u8(ctypes.byref(f(src_kind=2)), P, P, 0) == -1


def test_image_calls_fail_loudly_without_a_gpu():
    if torch.cuda.is_available():
        return
    with pytest.raises(hip.RcdmError):
        I.ClipImageProcessor()(images=IO.test_image(16, 16, 1), return_tensors="pt")
    with pytest.raises(hip.RcdmError):
        I.frames_to_uint8(torch.zeros(1, 3, 8, 8))


def test_image_grid_takes_uint8_tiles():
    from rcdms_amd.checkpoint import image_grid
    rng = np.random.RandomState(5)
    tiles = [rng.rand(8, 6, 3).astype(np.float32) for _ in range(6)]
    want = np.asarray(image_grid(tiles, 2, 3))
    u8 = [(t * 255).astype(np.uint8) for t in tiles]
    assert np.array_equal(np.asarray(image_grid(u8, 2, 3)), want)
    assert np.array_equal(np.asarray(image_grid([torch.from_numpy(t) for t in u8], 2, 3)), want)
    assert want.shape == (16, 18, 3) and np.array_equal(want[8:, 6:12], u8[4])
