"""GPU: rcdm_png_encode (csrc/png.hip) and what rcdms_amd/image.py, checkpoint.py, the VAE and the pipeline build on it.
The files are compared with the goldens of tools/mint_png_golden.py (the restatement tests/png_oracle.py) byte for byte —
the format is integer arithmetic, there is no tolerance — and the GPU's own bytes are decoded by Pillow.

Every source sits in the `U8` canary bands of tests/test_hip_image.py (pad bytes in every row, guard rows, gap rows between
images); every destination in `Streams` below: canary in front of the first stream, behind the last, and in every stream's
slot behind sizes[i], so a byte written past the reported size — or anywhere else — is seen.  Both are checked after each
call, the sources also for being unchanged.  Block geometry (RCDM_PNG_BLOCK = 32768 filtered bytes):
  1x1, 3x5       one block far shorter than a workgroup; the zero row above the first row
  105x107        rows of 322 B, two blocks with the cut inside a row, last block 1042 B
  256x85         rows of 256 B, exactly two full blocks: BFINAL behind a full block
  filters        131x131, every filter wins some rows (asserted from the filter bytes)
  limiter        128x85, filter 0, counts growing 1.8x per symbol: the unlimited tree is 16 deep
  const          64x64 of one colour; const_black with filter 0: ONE distinct literal, 1 bit per byte
  noise_f0..4    40x200 uniform noise under each fixed filter: codes of 8-9 bits, the slot near its bound
  batch          5 different 105x107 images in one call, padded pitch, gap rows, dst_stride = bound + 37"""
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch

from rcdms_amd import hip
from rcdms_amd import image as I
from tests import png_oracle as P
from tests.test_hip_image import CANARY, DEV, U8

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 4096


def golden(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    ends = np.cumsum(g["sizes"])
    files = [g["files"][e - s:e].tobytes() for s, e in zip(g["sizes"], ends)]
    return g["input"], files, json.loads(str(g["meta"]))


class Streams:
    """n output streams of `stride` bytes and the n sizes, all inside canary."""

    def __init__(self, n, stride):
        self.n, self.stride = n, stride
        self.buf = torch.full((2 * GUARD + n * stride,), CANARY, dtype=torch.uint8, device=DEV)
        self.sizes = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    @property
    def sizes_ptr(self):
        return self.sizes.data_ptr() + 8

    def files(self):
        """-> the n files; asserts that every byte outside [i * stride, i * stride + sizes[i]) still holds the canary."""
        torch.cuda.synchronize()
        sizes = self.sizes.cpu().numpy()
        assert sizes[0] == -1 and sizes[-1] == -1, "the words around sizes[] were written"
        raw = self.buf.cpu().numpy()
        keep = np.ones(raw.shape, dtype=bool)
        out = []
        for i in range(self.n):
            s = int(sizes[1 + i])
            assert 0 < s <= self.stride, f"sizes[{i}] = {s}"
            lo = GUARD + i * self.stride
            keep[lo:lo + s] = False
            out.append(raw[lo:lo + s].tobytes())
        bad = (raw != CANARY) & keep
        assert not bad.any(), f"{int(bad.sum())} bytes written outside the files, first at {int(np.flatnonzero(bad)[0]) - GUARD}"
        return out


def encode(src_view, filt, stride=None):
    """rcdm_png_encode through PngEncoder.launch into canary-guarded streams -> (files, bound)."""
    n, h, w, _ = src_view.shape
    enc = I.png_encoder(h, w, n, DEV)
    enc.workspace.fill_(0xEE)                             # the kernels may not rely on what the workspace held
    stride = enc.bound if stride is None else stride
    dst = Streams(n, stride)
    enc.launch(src_view, filt, dst=dst.ptr, dst_stride=stride, sizes=dst.sizes_ptr)
    return dst.files(), enc.bound


def check_file(data, img, bound):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img), "Pillow does not decode the GPU's file to the input"
    assert len(data) <= bound
    for kind, body, stored, real in P.parse_chunks(data):
        assert stored == real, f"CRC of a {kind!r} chunk"


SINGLE = ["png_1x1", "png_3x5", "png_105x107", "png_256x85", "png_filters", "png_limiter", "png_const", "png_const_black",
          "png_noise_f0", "png_noise_f1", "png_noise_f2", "png_noise_f3", "png_noise_f4"]


@pytest.mark.parametrize("name", SINGLE)
def test_png_equals_golden(hiplib, name):
    inp, want, m = golden(name)
    _, h, w, _ = inp.shape
    src = U8(1, h, w, pad=13, data=inp)
    got, bound = encode(src.view, m["filter"])
    src.check()
    assert bound == P.bound(h, w) == hip.png_bound(hip.PngDesc(3 * w, 0, 0, 1, h, w, 3, -1))
    check_file(got[0], inp[0], bound)
    assert len(got[0]) == len(want[0]), f"{len(got[0])} bytes, golden {len(want[0])}"
    assert got[0] == want[0], f"first differing byte at {next(i for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b)}"
    stream, types = P.filter_stream(inp[0], m["filter"])
    if name == "png_filters":
        assert np.bincount(types, minlength=5).min() > 0, "every filter must win some rows"
    if name == "png_limiter":
        hist = np.bincount(stream, minlength=256)
        assert len(stream) == hip.PNG_BLOCK and P.huffman_depths(np.concatenate([hist, [1]])).max() > 15
    if name == "png_const_black":
        assert len(np.unique(stream)) == 1
    if name == "png_256x85":
        assert len(stream) == 2 * hip.PNG_BLOCK
    if name == "png_105x107":
        assert len(stream) - hip.PNG_BLOCK == 1042 and hip.PNG_BLOCK % (1 + 3 * w)


def test_png_batch_of_five(hiplib):
    inp, want, m = golden("png_batch")
    n, h, w, _ = inp.shape
    src = U8(n, h, w, pad=5, gap_rows=3, data=inp)
    bound = P.bound(h, w)
    got, b = encode(src.view, m["filter"], stride=bound + 37)
    src.check()
    assert b == bound and len(set(len(f) for f in want)) == n
    for i in range(n):
        check_file(got[i], inp[i], bound)
        assert got[i] == want[i], f"image {i}"
    # the public entry on the same strided view: one download, a slice per file
    assert I.encode_png(src.view) == want
    src.check()
    assert I.encode_png(src.view[2]) == want[2:3]


def test_png_rejects_a_short_dst_stride(hiplib):
    h, w = 3, 5
    src = torch.zeros(2, h, w, 3, dtype=torch.uint8, device=DEV)
    enc = I.png_encoder(h, w, 2, DEV)
    with pytest.raises(hip.RcdmError, match="RCDM_EINVAL"):
        enc.launch(src, dst_stride=enc.bound - 1)


@pytest.fixture(scope="module")
def story():
    """Five procedural 512 x 512 frames (noise of 0, 0.5, 2, 2, 6 grey levels) on the host and the device."""
    frames = np.stack([P.cartoon(512, 512, s, 60 + i) for i, s in enumerate([0.0, 0.5, 2.0, 2.0, 6.0])])
    return frames, torch.from_numpy(frames).to(DEV)


def test_png_five_story_frames(hiplib, story):
    frames, dev = story
    src = U8(5, 512, 512, pad=4, data=dev)
    bound = P.bound(512, 512)
    got, b = encode(src.view, "adaptive", stride=bound + 5)
    src.check()
    assert b == bound
    for i in range(5):
        check_file(got[i], frames[i], bound)
        assert len(got[i]) == P.png_size(frames[i]), i


def test_story_grid_png(hiplib, story):
    from rcdms_amd.checkpoint import story_grid_png
    frames, dev = story
    cells = [dev[i % 5] if i < 5 else dev[(i + 2) % 5].flip(1) for i in range(10)]
    want = np.concatenate([np.concatenate([c.cpu().numpy() for c in cells[r * 5:(r + 1) * 5]], axis=1) for r in range(2)], axis=0)
    assert want.shape == (1024, 2560, 3)
    data = story_grid_png(cells, 2, 5)
    bound = P.bound(1024, 2560)
    check_file(data, want, bound)
    assert len(data) == P.png_size(want)
    for c, f in zip(cells, frames):
        assert np.array_equal(c.cpu().numpy(), f)         # the cells are only read


def test_png_graph_replay_equals_eager(hiplib):
    inp, want, m = golden("png_batch")
    n, h, w, _ = inp.shape
    src = torch.from_numpy(inp).to(DEV)
    enc = I.PngEncoder(h, w, n, DEV)
    eager = enc.encode(src)
    assert eager == want
    enc.out.zero_()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = hip.Graph()
        g.begin()
        try:
            enc.launch(src)
        finally:
            g.end()
        s.synchronize()
        assert not bool(enc.out.any()), "capture must not execute"
        g.launch()
        s.synchronize()
    raw = enc.out.cpu().numpy()
    sizes = raw[n * enc.stride:].view(np.uint64)
    assert [raw[i * enc.stride:i * enc.stride + int(sizes[i])].tobytes() for i in range(n)] == eager


def decoded(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def test_decode_png_equals_decode_uint8(hiplib):
    from rcdms_amd import synth
    from tests.test_hip_image import _tiny_vae
    m = _tiny_vae(False)
    z = synth.normal_tensor("image.z", (2, 4, 8, 8), 43).to(DEV) * 3.0
    frames = m.decode_uint8(z).cpu().numpy()
    files = m.decode_png(z)
    assert len(files) == 2 and all(isinstance(f, bytes) for f in files)
    for f, want in zip(files, frames):
        assert np.array_equal(decoded(f), want)
        assert f == P.encode(want)
    assert len(np.unique(frames)) > 50


def test_pipeline_png_output(hiplib):
    """output_type="png": [[bytes] * f] * b whose decoded pixels are the "uint8" frames of the same call, byte for byte."""
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
    want = pipe(caps, src.to(DEV), generator=gen(), output_type="uint8", **kw).videos.cpu().numpy()
    got = pipe(caps, src.to(DEV), generator=gen(), output_type="png", **kw).videos
    assert len(got) == 1 and len(got[0]) == 5 and all(isinstance(f, bytes) for f in got[0])
    for k in range(5):
        assert np.array_equal(decoded(got[0][k]), want[0, k]), k
    assert len(np.unique(want)) > 20
