"""GPU: rcdm_png_encode_match (csrc/png.hip, png_match_block_kernel) and the match=True / png_match=True switches built on it.
The files are compared with the goldens of tools/mint_png_match_golden.py (the restatement tests/png_match_oracle.py) byte
for byte — the format is integer arithmetic, there is no tolerance — and the GPU's own bytes are decoded by Pillow.

Buffers as in tests/test_hip_png.py: every source in the `U8` canary bands (pad bytes in every row, guard rows, gap rows),
every destination in `Streams` (canary in front of, behind and between the files, and behind sizes[i] in every slot), and the
workspace in `Workspace` below: filled with a byte the kernels may not rely on, canary on both sides.  What each golden is
there for is listed in tools/mint_png_match_golden.py; the facts it needs are in its meta and asserted here again."""
import numpy as np
import pytest
import torch

from rcdms_amd import hip
from rcdms_amd import image as I
from tests import png_match_oracle as M
from tests import png_oracle as P
from tests.test_hip_image import CANARY, DEV, U8
from tests.test_hip_png import GUARD, Streams, check_file, decoded, golden

pytestmark = pytest.mark.gpu


class Workspace:
    """`nbytes` of workspace, 16-byte aligned, filled with 0xEE, inside canary."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((2 * GUARD + nbytes,), CANARY, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + nbytes] = 0xEE
        assert (self.buf.data_ptr() + GUARD) % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def check(self):
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + self.nbytes:] == CANARY).all(), "wrote outside the workspace"


def encode(src_view, filt, stride=None):
    """rcdm_png_encode_match on guarded buffers -> (files, bound)."""
    n, h, w, _ = src_view.shape
    d = hip.PngDesc(src_view.stride(1) if h > 1 else 3 * w, src_view.stride(0) if n > 1 else 0, 0, n, h, w, 3, I._png_filter(filt))
    bound = hip.png_bound(d)
    stride = bound if stride is None else stride
    d.dst_stride = stride if n > 1 else 0
    nbytes = hip.png_match_workspace_bytes(d)
    assert nbytes == hip.png_workspace_bytes(d) > 0
    ws = Workspace(nbytes)
    dst = Streams(n, stride)
    hip.png_encode_match(d, src_view.data_ptr(), ws.ptr, dst.ptr, dst.sizes_ptr)
    files = dst.files()
    ws.check()
    return files, bound


SINGLE = ["pngm_1x1", "pngm_3x5", "pngm_black", "pngm_w1", "pngm_w2", "pngm_w3", "pngm_105x107", "pngm_256x85", "pngm_300x85",
          "pngm_2x8192", "pngm_f0", "pngm_f1", "pngm_f2", "pngm_f3", "pngm_f4", "pngm_limiter"]


@pytest.mark.parametrize("name", SINGLE)
def test_png_match_equals_golden(hiplib, name):
    inp, want, m = golden(name)
    _, h, w, _ = inp.shape
    src = U8(1, h, w, pad=13, data=inp)
    got, bound = encode(src.view, m["filter"])
    src.check()
    assert bound == P.bound(h, w)
    check_file(got[0], inp[0], bound)
    assert len(got[0]) == len(want[0]), f"{len(got[0])} bytes, golden {len(want[0])}"
    assert got[0] == want[0], f"first differing byte at {next(i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)}"
    facts = m["facts"][0]
    assert len(got[0]) <= facts["literal_bytes"]
    if name in ("pngm_1x1", "pngm_3x5"):
        assert not any(facts["match_form"]) and got[0] == P.encode(inp[0], m["filter"])
    if name == "pngm_black":
        assert facts["distances"] == [1] and facts["match_form"] == [True]
    if name == "pngm_105x107":
        assert facts["match_form"] == [True, True] and facts["uncut_length"] > facts["cut"][1] and facts["reading_back"] > 0
    if name == "pngm_256x85":
        assert facts["match_form"] == [True, False]
    if name == "pngm_300x85":
        assert len(facts["match_form"]) == 3 and True in facts["match_form"] and False in facts["match_form"]
    if name == "pngm_2x8192":
        assert 2 * (1 + 3 * w) > M.WINDOW and (1 + 3 * w) in facts["distances"]
    if name == "pngm_limiter":
        assert facts["match_form"] == [True] and facts["unlimited_depth"] > 15 and facts["halvings"] >= 1


def test_png_match_batch_of_five(hiplib):
    inp, want, m = golden("pngm_batch")
    n, h, w, _ = inp.shape
    src = U8(n, h, w, pad=5, gap_rows=3, data=inp)
    bound = P.bound(h, w)
    got, b = encode(src.view, m["filter"], stride=bound + 37)
    src.check()
    assert b == bound and len(set(len(f) for f in want)) == n
    for i in range(n):
        check_file(got[i], inp[i], bound)
        assert got[i] == want[i], f"image {i}"
    assert got[4] == P.encode(inp[4])                     # noise of 40 grey levels: every block falls back
    # the public entry on the same strided view
    assert I.encode_png(src.view, match=True) == want
    src.check()
    assert I.encode_png(src.view[2], match=True) == want[2:3]
    assert I.encode_png(src.view) == [P.encode(im) for im in inp]   # match=False is still the literal-only file


@pytest.fixture(scope="module")
def frames():
    """Three procedural 128 x 128 frames (noise of 0, 0.5 and 6 grey levels) on the host and the device."""
    f = np.stack([P.cartoon(128, 128, s, 70 + i) for i, s in enumerate([0.0, 0.5, 6.0])])
    return f, torch.from_numpy(f).to(DEV)


def test_encode_png_match_decodes_to_the_frames(hiplib, frames, tmp_path):
    host, dev = frames
    plain = I.encode_png(dev)
    match = I.encode_png(dev, match=True)
    for k in range(3):
        assert np.array_equal(decoded(match[k]), host[k]) and np.array_equal(decoded(plain[k]), host[k])
        assert len(match[k]) <= len(plain[k]) and match[k] == M.encode(host[k])
    assert len(match[0]) < len(plain[0]) // 2             # the flat frame
    paths = [tmp_path / f"{k}.png" for k in range(3)]
    I.save_png(paths, dev, match=True)
    assert [p.read_bytes() for p in paths] == match


def test_story_grid_png_match(hiplib, frames):
    from rcdms_amd.checkpoint import story_grid_png
    host, dev = frames
    cells = [dev[i % 3] for i in range(6)]
    want = np.concatenate([np.concatenate([host[i % 3] for i in range(r * 3, r * 3 + 3)], axis=1) for r in range(2)], axis=0)
    plain, match = story_grid_png(cells, 2, 3), story_grid_png(cells, 2, 3, match=True)
    assert np.array_equal(decoded(match), want) and np.array_equal(decoded(plain), want)
    check_file(match, want, P.bound(*want.shape[:2]))
    assert len(match) == M.png_size(want) <= len(plain) == P.png_size(want)


def test_decode_png_match(hiplib):
    from rcdms_amd import synth
    from tests.test_hip_image import _tiny_vae
    m = _tiny_vae(False)
    z = synth.normal_tensor("image.z", (2, 4, 8, 8), 43).to(DEV) * 3.0
    want = m.decode_uint8(z).cpu().numpy()
    plain, match = m.decode_png(z), m.decode_png(z, match=True)
    for k in range(2):
        assert np.array_equal(decoded(match[k]), want[k]) and np.array_equal(decoded(plain[k]), want[k])
        assert match[k] == M.encode(want[k]) and plain[k] == P.encode(want[k])


def test_pipeline_png_match_output(hiplib):
    """output_type="png", png_match=True: files whose pixels are those of the png_match=False call."""
    from rcdms_amd import context, synth
    from rcdms_amd.scheduler import DDIMScheduler
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    from tests.test_hip_image import _tiny_vae
    from tests.test_hip_unet import build
    from tests.test_pipeline_e2e import D, _Text, _Tok
    unet = build("unet_tiny")
    local = context.fine_stack(text_dim=D, vis_dim=32, hidden_dim=D, num_heads=8)
    glob = context.semantic_stack(text_dim=D, vis_dim=24, hidden_dim=D, num_heads=8)
    local.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in local.state_dict().items()}, 11))
    glob.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in glob.state_dict().items()}, 12))
    pipe = RCDMsPipeline(vae=_tiny_vae(True), text_encoder=_Text(), tokenizer=_Tok(), unet=unet, local_module=local, global_module=glob,
                         scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear")).to(DEV)
    H = W = 128
    caps = ["pororo waves", "loopy sings", "eddy builds", "crong jumps", "poby fishes"]
    src = synth.normal_tensor("e2e.src", (5, 3, H, W), 2) * 0.5
    mask_label = torch.zeros(1, 5, H // 8, W // 8)
    mask_label[:, 0] = 1.0
    kw = dict(image_embeds_1=synth.normal_tensor("e2e.img1", (1, 9, 32), 3).to(DEV),
              proj_embeds_0=synth.normal_tensor("e2e.proj0", (4, 1, 24), 4).to(DEV), mask_label=mask_label.to(DEV), video_length=5,
              height=H, width=W, num_inference_steps=2, guidance_scale=2.0,
              latents=synth.normal_tensor("e2e.lat", (1, 4, 5, H // 8, W // 8), 5).to(DEV))
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)
    plain = pipe(caps, src.to(DEV), generator=gen(), output_type="png", **kw).videos
    match = pipe(caps, src.to(DEV), generator=gen(), output_type="png", png_match=True, **kw).videos
    assert len(match) == 1 and len(match[0]) == 5 and all(isinstance(f, bytes) for f in match[0])
    for k in range(5):
        want = decoded(plain[0][k])
        assert np.array_equal(decoded(match[0][k]), want), k
        assert match[0][k] == M.encode(want) and len(match[0][k]) <= len(plain[0][k])
