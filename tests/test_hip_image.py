"""GPU: rcdm_image_resample / rcdm_frames_to_u8 (csrc/image.hip) and what rcdms_amd/image.py, the VAE and the pipeline build
on them.  The resample kernel's bytes are compared with Pillow's own (the goldens of tools/mint_image_golden.py) with NO
tolerance: the arithmetic is integer.  The kernel's output tile is 32 x 32 (RCDM_IMAGE_TILE): the 131 x 131 case spans
4 full tiles and a ragged one of 3 in both axes, the 224 x 224 cases 7 full tiles, 29 x 31 and 16 x 24 less than one.

Every buffer a kernel is handed sits inside guard bands: float outputs through tests/guard.py (NaN fill), uint8 buffers
through `U8` below — a 0xA5 canary in the pad bytes of every row (pitch > 3 w), in 256 guard rows above and below, and in
the gap rows between the images of a batch — checked after every call, inputs included."""
import json
import os

import numpy as np
import pytest
import torch

from rcdms_amd import hip
from rcdms_amd import image as I
from tests import guard as G
from tests import image_oracle as IO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CANARY = 0xA5
DEV = "cuda"


def golden(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g, json.loads(str(g["meta"]))


class U8:
    """n images of h x w x 3 bytes inside canary: row pitch 3 w + pad, gap_rows canary rows between images, G.GUARD_ROWS
    above and below.  .view is the (n, h, w, 3) strided tensor a kernel gets; check() asserts every other byte still holds
    the canary (and, for an input, that the images are unchanged)."""

    def __init__(self, n, h, w, pad=13, gap_rows=0, data=None):
        self.pitch = 3 * w + pad
        self.rows_per_image = h + gap_rows
        total = 2 * G.GUARD_ROWS + n * self.rows_per_image
        self.buf = torch.full((total * self.pitch,), CANARY, dtype=torch.uint8, device=DEV)
        off = G.GUARD_ROWS * self.pitch
        self.view = self.buf.as_strided((n, h, w, 3), (self.rows_per_image * self.pitch, self.pitch, 3, 1), off)
        self.mask = torch.zeros_like(self.buf, dtype=torch.bool)
        self.mask.as_strided(self.view.shape, self.view.stride(), off).fill_(True)
        self.data = None
        if data is not None:
            self.data = torch.as_tensor(data).to(DEV)
            self.view.copy_(self.data)

    def check(self):
        torch.cuda.synchronize()
        bad = (self.buf != CANARY) & ~self.mask
        assert not bool(bad.any()), f"{int(bad.sum())} canary bytes overwritten, first at byte {int(bad.nonzero()[0])} (pitch {self.pitch})"
        if self.data is not None:
            assert torch.equal(self.view, self.data), "a read-only source image changed"


def resampler_for(m):
    return I.resampler(m["in_h"], m["in_w"], m["resized_h"], m["resized_w"], m["filter"],
                       None if m["window"][:2] == [0, 0] and m["window"][2:] == [m["resized_h"], m["resized_w"]] else tuple(m["window"]), DEV)


CASES = ["image_up_odd", "image_down_bilinear", "image_down_bicubic", "image_skip_rows", "image_ratio", "image_clip_crop",
         "image_clip_tall", "image_real_clip", "image_real_vae"]


@pytest.mark.parametrize("name", CASES)
def test_resample_uint8_equals_pillow(hiplib, name):
    """Mode RCDM_IMAGE_U8 against Pillow's bytes; image_down_bicubic is the batch of five, here with an image stride larger
    than the image on both sides (gap rows)."""
    g, m = golden(name)
    n = g["input"].shape[0]
    src = U8(n, m["in_h"], m["in_w"], pad=5, gap_rows=3 if n > 1 else 0, data=g["input"])
    want = torch.from_numpy(g["output"])
    dst = U8(n, want.shape[1], want.shape[2], pad=13, gap_rows=7 if n > 1 else 0)
    r = resampler_for(m)
    r.to_uint8(src.view, out=dst.view)
    src.check()
    dst.check()
    got = dst.view.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} bytes differ from Pillow"
    if name in ("image_ratio", "image_clip_crop"):
        assert want.shape[1] > 2 * hip.IMAGE_TILE and want.shape[2] > 2 * hip.IMAGE_TILE
    if name == "image_ratio":
        assert want.shape[1] % hip.IMAGE_TILE and want.shape[2] % hip.IMAGE_TILE
    if name == "image_clip_crop":
        assert m["window"][1] == 56                           # tables that start at a non-zero output column
    # flip_channels: the same bytes with channels 0 and 2 exchanged
    dst2 = U8(n, want.shape[1], want.shape[2], pad=1, gap_rows=2 if n > 1 else 0)
    r.to_uint8(src.view, flip=True, out=dst2.view)
    dst2.check()
    assert torch.equal(dst2.view.cpu(), want.flip(-1))


def test_resample_reads_a_frame_out_of_a_strip(hiplib):
    """The h5 split holds five frames stacked in one 640 x 128 strip: frames 1 and 3 of it, by pointer and image stride."""
    g, m = golden("image_real_clip")
    frames = np.stack([np.roll(g["input"][0], 11 * i, axis=1) for i in range(5)])
    strip = U8(1, 5 * 128, 128, pad=0, data=frames.reshape(1, 640, 128, 3))
    sel = strip.view[0].view(5, 128, 128, 3)[1::2]
    assert sel.stride(0) == 2 * 128 * strip.pitch and not sel.is_contiguous()
    got = I.resampler(128, 128, 56, 56, "bicubic", None, DEV).to_uint8(sel)
    strip.check()
    for j, i in enumerate((1, 3)):
        assert np.array_equal(got[j].cpu().numpy(), IO.resize(frames[i], (56, 56), "bicubic"))


@pytest.mark.parametrize("name,mean,std,flip", [("image_real_clip", I.CLIP_MEAN, I.CLIP_STD, False),
                                                ("image_clip_crop", I.CLIP_MEAN, I.CLIP_STD, True),
                                                ("image_down_bicubic", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), False),
                                                ("image_ratio", (0.4, 0.5, 0.6), (0.3, 0.5, 1.5), False)])
def test_resample_float_modes(hiplib, name, mean, std, flip):
    """RCDM_IMAGE_F32_NCHW within 1e-6 of (u8 / 255 - mean) / std in float64 on Pillow's bytes: the value takes four fp32
    roundings (the product by fl(1/255), the difference, fl(1/std), the last product) of <= 2^-24 relative each on
    magnitudes <= 1, amplified by 1 / std <= 3.83 (CLIP's smallest std, 0.2613): <= 4 * 6e-8 * 3.83 = 9.2e-7; results
    stay <= 2.3.  RCDM_IMAGE_F16_ROWS equals that tensor rounded to f16 bit for bit, pad channels zero."""
    g, m = golden(name)
    assert min(std) >= 0.26
    n = g["input"].shape[0]
    src = U8(n, m["in_h"], m["in_w"], pad=2, gap_rows=1 if n > 1 else 0, data=g["input"])
    u8 = g["output"][..., ::-1] if flip else g["output"]
    want = np.stack([IO.normalize(x, mean, std) for x in u8])
    _, _, oh, ow = want.shape
    r = resampler_for(m)
    out_b, _ = G.guarded_out(n * 3 * oh, ow, ow, torch.float32, device=DEV)
    r.launch(r.desc(src.view, hip.IMAGE_F32_NCHW, flip, mean, std), src.view, out_b.data_ptr())
    torch.cuda.synchronize()
    src.check()
    G.check_out(out_b)
    G.check_written(out_b)
    got_b = out_b.cpu().reshape(n, 3, oh, ow)
    err = float(np.abs(got_b.double().numpy() - want).max())
    print(f"{name}: mode F32_NCHW max |err| {err:.3e}, max |value| {float(got_b.abs().max()):.3f}")
    assert err <= 1e-6, err
    # ... and it is the fp32 sequence the header states, bit for bit
    assert np.array_equal(got_b.numpy(), np.stack([IO.normalize_f32(x, mean, std) for x in u8]))
    c_pad, ld = 16, 24
    out_c, _ = G.guarded_out(n * oh * ow, c_pad, ld, torch.float16, device=DEV)
    r.to_rows(src.view, mean, std, out_c.data_ptr(), ld, c_pad, flip)
    torch.cuda.synchronize()
    src.check()
    G.check_out(out_c)
    G.check_written(out_c)
    rows = out_c[:, :c_pad].cpu().reshape(n, oh, ow, c_pad)
    assert torch.equal(rows[..., :3].view(torch.int16), got_b.half().permute(0, 2, 3, 1).contiguous().view(torch.int16))
    assert not bool(rows[..., 3:].view(torch.int16).any()), "pad channels must be zero"


def _f16_values():
    """Every finite f16 value in [-1.25, 1.25] (31 745 of them: all truncation boundaries of x / 2 + 0.5 -> byte), then +-inf,
    padded with zeros to a whole image of 64-pixel rows."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    v = bits[torch.isfinite(bits) & (bits.abs() <= 1.25)]
    v = torch.cat([v, torch.tensor([float("inf"), float("-inf")], dtype=torch.float16)])
    W = 64
    H = -(-v.numel() // (3 * W))
    x = torch.zeros(H * W * 3, dtype=torch.float16)
    x[:v.numel()] = v
    return x.reshape(H * W, 3), H, W


def _torch_cpu_u8(x):
    return torch.from_numpy(((x.float() / 2 + 0.5).clamp(0, 1).numpy() * 255).astype(np.uint8))


def test_frames_to_u8_every_f16_value(hiplib):
    px, H, W = _f16_values()
    assert px.numel() >= 31000
    want = _torch_cpu_u8(px).reshape(1, H, W, 3)
    assert set(want.unique().tolist()) == set(range(256))
    rows, _ = G.guarded_in(px, 8, device=DEV)                                   # ld 8: five poisoned pad channels per pixel
    dst = U8(1, H, W, pad=7)
    d = hip.FramesU8Desc(dst.pitch, 0, 1, H, W, 3, hip.FRAMES_F16_ROWS, 8)
    hip.frames_to_u8(d, rows.data_ptr(), dst.view.data_ptr())
    dst.check()
    G.check_in(rows)
    assert torch.equal(dst.view.cpu(), want)
    # the same values as an fp32 NCHW tensor, guard rows around it
    nchw = px.float().reshape(H, W, 3).permute(2, 0, 1).contiguous()
    src32, _ = G.guarded_in(nchw.reshape(3 * H, W), W, device=DEV)
    dst2 = U8(1, H, W, pad=3)
    d = hip.FramesU8Desc(dst2.pitch, 0, 1, H, W, 3, hip.FRAMES_F32_NCHW, 0)
    hip.frames_to_u8(d, src32.data_ptr(), dst2.view.data_ptr())
    dst2.check()
    G.check_in(src32)
    assert torch.equal(dst2.view.cpu(), want)
    # NaN has no byte in the reference (numpy leaves the cast undefined): the kernel's is 0
    nan = torch.full((1, 3, 4, 4), float("nan"), device=DEV)
    assert not bool(I.frames_to_uint8(nan).any())


def test_frames_to_u8_into_grid_cells(hiplib):
    """Three frames written by pitch and offset into cells (1, 1..3) of a 2 x 5 grid image: the seven other cells, the pad
    bytes and the guard rows keep what they held."""
    h, w = 24, 20
    x = (torch.randn(3, 3, h, w, generator=torch.Generator().manual_seed(3)) * 0.8)
    grid = U8(1, 2 * h, 5 * w, pad=9)
    before = torch.randint(0, 256, (2 * h, 5 * w, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    grid.view[0].copy_(before.to(DEV))
    cells = grid.view[0].as_strided((3, h, w, 3), (3 * w, grid.pitch, 3, 1), grid.view[0].storage_offset() + h * grid.pitch + 3 * w)
    I.frames_to_uint8(x.to(DEV), out=cells)
    grid.check()
    got = grid.view[0].cpu()
    want = before.clone()
    for i in range(3):
        want[h:, (1 + i) * w:(2 + i) * w] = _torch_cpu_u8(x[i]).permute(1, 2, 0)
    assert torch.equal(got, want)


def test_processor_front_end_of_the_vision_encoder(hiplib):
    """ClipImageProcessor -> CLIPVisionEncoder at the 56-px config: the processor's pixel values are the oracle's fp32
    sequence bit for bit, so the encoder's outputs are identical; accepted inputs: numpy, a list, PIL, a device tensor."""
    from tests.test_clip import gpu_encoder
    enc = gpu_encoder("clip_vision_56")
    frames = np.stack([IO.test_image(75, 100, 40 + i) for i in range(3)])      # 75 x 100 -> 56 x 74 -> crop columns 9 .. 65
    proc = I.ClipImageProcessor(size=56, crop_size=56)
    pv = proc(images=frames, return_tensors="pt").pixel_values
    assert pv.is_cuda and pv.dtype == torch.float32 and tuple(pv.shape) == (3, 3, 56, 56)
    want = []
    for f in frames:
        u8, pv64 = IO.clip_pixel_values(f, 56, 56)
        want.append(IO.normalize_f32(u8, IO.CLIP_MEAN, IO.CLIP_STD))
        assert np.abs(want[-1] - pv64).max() <= 1e-6
    want = torch.from_numpy(np.stack(want))
    assert torch.equal(pv.cpu(), want)
    assert torch.equal(proc.cropped_uint8(frames).cpu(), torch.from_numpy(np.stack([IO.clip_pixel_values(f, 56, 56)[0] for f in frames])))
    a, b = enc(pv), enc(want.to(DEV))
    assert torch.equal(a.last_hidden_state, b.last_hidden_state) and torch.equal(a.image_embeds, b.image_embeds)
    assert torch.isfinite(a.image_embeds).all()
    assert torch.equal(proc(images=list(frames)).pixel_values, pv)
    assert torch.equal(proc(images=torch.from_numpy(frames).to(DEV))["pixel_values"], pv)
    try:
        from PIL import Image
        assert torch.equal(proc(images=[Image.fromarray(f) for f in frames]).pixel_values, pv)
    except ImportError:
        pass
    flipped = I.ClipImageProcessor(size=56, crop_size=56, flip_channels=True)(images=frames).pixel_values
    assert torch.equal(flipped, I.ClipImageProcessor(size=56, crop_size=56)(images=np.ascontiguousarray(frames[..., ::-1])).pixel_values)


def _tiny_vae(both):
    from oracle import vae_oracle as V
    from rcdms_amd import synth, vae
    cfg = V.tiny_vae_config()
    shapes = dict(V.decoder_shapes(cfg))
    if both:
        shapes.update(V.encoder_shapes(cfg))
    kw = dict(cfg)
    kw["norm_num_groups"] = kw.pop("groups")
    m = (vae.AutoencoderKL if both else vae.AutoencoderKLDecoder)(**kw).eval()
    m.load_state_dict(synth.procedural_state_dict(shapes, 41))
    return m.to(DEV)


def test_frame_transform_rows_into_the_vae_encoder(hiplib):
    """FrameTransform(rows=True) writes f16 pixel rows into the encode plan's input: the posterior equals the one of the
    fp32 NCHW route (encode(transform(frames))) bit for bit, at 64 x 64."""
    m = _tiny_vae(True)
    frames = np.stack([IO.test_image(32, 40, 50 + i) for i in range(2)])
    ft = I.FrameTransform(64, 64)
    x = ft(frames)
    assert tuple(x.shape) == (2, 3, 64, 64) and x.dtype == torch.float32 and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
    want = np.stack([IO.normalize_f32(IO.resize(f, (64, 64), "bilinear"), (0.5,) * 3, (0.5,) * 3) for f in frames])
    assert np.array_equal(x.cpu().numpy(), want)
    a = m.encode(x).latent_dist
    b = m.encode_frames(frames, ft).latent_dist
    assert torch.isfinite(a.mean).all() and torch.equal(a.mean, b.mean) and torch.equal(a.logvar, b.logvar)


def test_decode_uint8_equals_truncated_decode(hiplib):
    from rcdms_amd import synth
    m = _tiny_vae(False)
    z = synth.normal_tensor("image.z", (2, 4, 8, 8), 43).to(DEV) * 3.0          # wide enough to reach both clamps
    got = m.decode_uint8(z)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (2, 64, 64, 3)
    sample = m.decode(z).sample
    want = I.frames_to_uint8(sample)
    assert torch.equal(got, want)
    assert torch.equal(want.cpu(), _torch_cpu_u8(sample.cpu()).permute(0, 2, 3, 1))
    assert len(got.unique()) > 50


@pytest.mark.parametrize("hip_vae", [False, True], ids=["stub_vae", "hip_vae"])
def test_pipeline_uint8_output(hiplib, hip_vae):
    """output_type="uint8": device uint8 (b, f, H, W, 3), the truncation of the "tensor" output of the same call."""
    from rcdms_amd import context, synth
    from rcdms_amd.scheduler import DDIMScheduler
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    from tests.test_hip_unet import build
    from tests.test_pipeline_e2e import D, _Text, _Tok, _Vae
    unet = build("unet_tiny")
    local = context.fine_stack(text_dim=D, vis_dim=32, hidden_dim=D, num_heads=8)
    glob = context.semantic_stack(text_dim=D, vis_dim=24, hidden_dim=D, num_heads=8)
    local.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in local.state_dict().items()}, 11))
    glob.load_state_dict(synth.procedural_state_dict({k: v.shape for k, v in glob.state_dict().items()}, 12))
    vae = _tiny_vae(True) if hip_vae else _Vae()
    pipe = RCDMsPipeline(vae=vae, text_encoder=_Text(), tokenizer=_Tok(), unet=unet, local_module=local, global_module=glob,
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
    ref = pipe(caps, src.to(DEV), generator=gen(), **kw).videos
    assert ref.dtype == torch.float32 and not ref.is_cuda and tuple(ref.shape) == (1, 3, 5, H, W)      # "tensor": as before
    got = pipe(caps, src.to(DEV), generator=gen(), output_type="uint8", **kw).videos
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1, 5, H, W, 3)
    want = torch.from_numpy((ref.numpy() * 255).astype(np.uint8)).permute(0, 2, 3, 4, 1)
    assert torch.equal(got.cpu(), want)
    assert len(want.unique()) > 20
