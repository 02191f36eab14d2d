"""GPU: StoryRunner(..., metrics=...) on the tiny chain of tests/test_story_gpu.py (its builders, imported): the SSIM / PSNR of
the generated uint8 frames against the given frames resized to the stage-2 size, and the CLIP-I cosine.  The figures are
checked three ways: against rcdms_amd.metrics.frame_metrics on the same device tensors (the same bits), against the float64
restatement tests/ssim_oracle.py on the downloaded bytes (its budget), and — CLIP-I — against a vision forward of the test's
own.  metrics=() must change nothing: the new fields are None and the frames are byte-identical."""
import numpy as np
import pytest
import torch

from tests import ssim_oracle as O
from tests.test_story_gpu import CAPS, DEV, H, S, W, chain, cuda_gen  # noqa: F401  (chain: the module-scoped fixture)

pytestmark = pytest.mark.gpu
ALL = ("ssim", "psnr", "clip_i")


def call(b, metrics, **kw):
    args = dict(num_inference_steps=3, prior_steps=3, guidance_scale=2.0, prior_guidance_scale=4.0, output_type="uint8",
                generator=[cuda_gen(s) for s in (51, 52, 53)], prior_generator=[cuda_gen(s) for s in (41, 42, 43)], metrics=metrics)
    args.update(kw)
    return b.runner(b.frames, CAPS, **args)


@pytest.fixture(scope="module")
def results(chain):
    return call(chain, ALL), call(chain, ())


def targets(b):
    from rcdms_amd.image import resampler
    flat = b.frames.reshape(S * 5, *b.frames.shape[2:]).to(DEV)
    return resampler(flat.shape[1], flat.shape[2], H, W, "bilinear").to_uint8(flat).view(S, 5, H, W, 3)


def test_story_metrics_equal_frame_metrics_and_the_oracle(chain, results):
    from rcdms_amd.metrics import frame_metrics
    res, _ = results
    assert tuple(res.videos.shape) == (S, 5, H, W, 3) and res.videos.dtype == torch.uint8
    for t in (res.ssim, res.psnr, res.clip_i):
        assert tuple(t.shape) == (S, 5) and t.is_cuda
    target = targets(chain)
    assert torch.equal(chain.runner.target_frames(chain.frames.to(DEV)), target)
    try:
        from PIL import Image
        pil = np.asarray(Image.fromarray(chain.frames[1, 2].numpy()).resize((W, H), Image.Resampling.BILINEAR))
        assert np.array_equal(target[1, 2].cpu().numpy(), pil), "the target frames are not Pillow's bilinear resize"
    except ImportError:
        pass
    fm = frame_metrics(res.videos, target)
    assert torch.equal(res.ssim.view(torch.int64), fm.ssim.view(S, 5).view(torch.int64))
    assert torch.equal(res.psnr.view(torch.int64), fm.psnr.view(S, 5).view(torch.int64))
    got, tgt = res.videos.cpu().numpy(), target.cpu().numpy()
    ssim, psnr = res.ssim.cpu().numpy(), res.psnr.cpu().numpy()
    for s in range(S):
        for f in range(5):
            want = O.ssim(got[s, f], tgt[s, f])
            assert abs(ssim[s, f] - want) <= O.BUDGET, (s, f, ssim[s, f], want)
            assert psnr[s, f] == pytest.approx(O.psnr(got[s, f], tgt[s, f]), rel=1e-12), (s, f)
    print(f"story metrics: ssim {ssim.min():.6f}..{ssim.max():.6f}, psnr {psnr.min():.3f}..{psnr.max():.3f} dB")
    assert (np.abs(ssim) <= 1.0).all() and np.isfinite(psnr).all() and (psnr > 0).all()


def test_story_clip_i_is_the_cosine_of_a_separate_vision_forward(chain, results):
    res, _ = results
    b = chain
    px = b.runner.clip_processor(images=res.videos.reshape(S * 5, H, W, 3)).pixel_values
    e = b.vision(px).image_embeds.reshape(S, 5, -1).float()
    want = torch.nn.functional.cosine_similarity(e, res.target_embeds.float(), dim=-1)
    diff = float((res.clip_i - want).abs().max())
    print(f"clip_i {float(res.clip_i.min()):.4f}..{float(res.clip_i.max()):.4f}, |runner - separate forward| {diff:.2e}")
    # the same kernels on the same pixels: equal, but for a last-bit difference of an f16 row between two runs (2^-10 relative
    # on single elements of a 128-element dot product)
    assert diff <= 2.0 ** -10, diff
    assert float(res.clip_i.abs().max()) <= 1.0 + 1e-6


def test_no_metrics_changes_nothing(chain, results):
    on, off = results
    assert off.ssim is None and off.psnr is None and off.clip_i is None
    assert torch.equal(on.videos, off.videos), "the frames differ with metrics on"
    assert torch.equal(on.image_embeds, off.image_embeds) and torch.equal(on.cosine, off.cosine)
    only = call(chain, ("psnr",))
    assert only.ssim is None and only.clip_i is None and torch.equal(only.psnr.view(torch.int64), on.psnr.view(torch.int64))


def test_metrics_need_uint8_frames_of_a_stage2_run(chain):
    b = chain
    with pytest.raises(ValueError, match="uint8"):
        call(b, ("ssim",), output_type="tensor")
    with pytest.raises(ValueError, match="uint8"):
        call(b, ("psnr",), output_type="png")
    with pytest.raises(ValueError, match="stage 2"):
        call(b, ("clip_i",), stage2=False)
    with pytest.raises(ValueError, match="fid"):
        call(b, ("ssim", "fid"))
