"""GPU: the stage-2 autoregression of StoryRunner (stage2_autoreg=True) on the tiny chain of tests/test_story_gpu.py (its
builders and its oracle flow, imported): S = 2 stories, 128 x 128 frames, 16 x 16 latents, 2 denoising steps — the smallest run
with two stories, five passes each and all four seen-frame patterns.  Every pass against the single-story oracle fed the
runner's own hand-off, so that the passes' errors are not compounded; the launch-plan bookkeeping over repeated calls; the
driver's PNG files; the metrics."""
import gc
import io

import numpy as np
import pytest
import torch

from rcdms_amd.story import source_from_bytes
from tests import test_story_gpu as SG
from tests.test_hip_unet import rel_rms
from tests.test_story_gpu import CAPS, DEV, H, LH, LW, STAGE2_BOUND, W, chain, cuda_gen, stage2_story_ref  # noqa: F401  (chain: the module-scoped fixture)

pytestmark = pytest.mark.gpu
S = 2
STEPS, GS = 2, 2.0
SEEDS1, SEEDS2 = [41, 42], [51, 52]


def call(b, **kw):
    args = dict(stage2_autoreg=True, num_inference_steps=STEPS, prior_steps=3, guidance_scale=GS, prior_guidance_scale=4.0,
                generator=[cuda_gen(s) for s in SEEDS2], prior_generator=[cuda_gen(s) for s in SEEDS1])
    args.update(kw)
    return b.runner(b.frames[:S], CAPS[:S], **args)


@pytest.fixture(scope="module")
def run(chain, tmp_path_factory):
    """One autoregressive call shared by the tests below: float frames, both directories, SSIM and PSNR."""
    d = tmp_path_factory.mktemp("autoreg")
    res = call(chain, output_type="tensor", frames_dir=str(d / "metric"), grid_dir=str(d / "grid"), indices=[7, 9],
               metrics=("ssim", "psnr"))
    return res, d


def test_every_pass_matches_the_oracle_on_the_runners_own_hand_off(chain, run, monkeypatch):
    b, (res, _) = chain, run
    assert tuple(res.videos.shape) == (S, 3, 5, H, W) and torch.isfinite(res.videos).all()
    assert tuple(res.frames_u8.shape) == (S, 5, H, W, 3) and res.frames_u8.dtype == torch.uint8 and res.frames_u8.is_cuda
    caps = [[c.lower() for c in story] for story in CAPS[:S]]
    frames = b.frames[:S].to(DEV)
    # the hidden states the HIP vision tower gives (CLIP has its own tests and bounds): the given frame 0, then — in the
    # runner's own batches of S — the generated frames 0..3
    px = lambda u8: b.runner.clip_processor(images=u8).pixel_values
    given = b.vision(px(frames[:, 0])).last_hidden_state.float().cpu()                                   # (S, tokens, width)
    gen = [b.vision(px(res.frames_u8[:, j].contiguous())).last_hidden_state.float().cpu() for j in range(4)]
    src0 = b.runner.frame_transform(frames[:, 0]).cpu()
    handed = source_from_bytes(res.frames_u8).cpu()                                                      # (S, 5, 3, H, W)
    assert torch.equal(handed, (res.frames_u8.cpu().permute(0, 1, 4, 2, 3).float() / 255 - 0.5) / 0.5)
    embeds = res.image_embeds.float().cpu()
    # stage2_story_ref draws the posterior noise from cuda_gen(seed): hand it the story's running generator instead
    monkeypatch.setattr(SG, "cuda_gen", lambda g: g)
    for s in range(S):
        te = b.pipe._encode_prompt(caps[s], torch.device(DEV), 1, True, None).float().cpu()
        g = cuda_gen(SEEDS2[s])                            # story s's five passes draw from it one after the other
        for i in range(5):
            n = max(i, 1)
            src = torch.full((5, 3, H, W), -1.0)
            mask = torch.zeros(5, LH, LW)
            mask[:n] = 1.0
            if i == 0:
                src[0], img1 = src0[s], given[s:s + 1]
            else:
                src[:i], img1 = handed[s, :i], torch.stack([gen[j][s] for j in range(i)])
            # the pass's draws in the pipeline's order: posterior noise (replayed inside the oracle flow from a copy of the
            # generator at this point), then the initial latents
            replay = cuda_gen(0)
            replay.set_state(g.get_state())
            torch.randn(5, 4, LH, LW, generator=g, device=DEV)
            lat0 = torch.randn((1, 4, 5, LH, LW), generator=g, device=DEV, dtype=torch.float32).cpu()
            want = stage2_story_ref(b, te, mask, img1, embeds[s, n:].unsqueeze(1), src, lat0, replay, STEPS, GS)
            r = rel_rms(res.videos[s, :, i].float(), want[:, i])
            print(f"stage-2 autoreg: story {s}, pass {i}: kept frame rel-RMS {r:.3e}")
            # measured on MI355X, passes 0..4: story 0 1.18e-3 / 1.23e-3 / 1.25e-3 / 1.17e-3 / 1.22e-3, story 1 1.42e-3 /
            # 1.27e-3 / 1.19e-3 / 1.38e-3 / 1.31e-3
            assert r <= STAGE2_BOUND, (s, i, r)
            want8 = (res.videos[s, :, i].permute(1, 2, 0) * 255).to(torch.uint8)
            assert int((res.frames_u8[s, i].cpu().int() - want8.int()).abs().max()) <= 1


def test_repeated_calls_build_no_plan_and_hold_no_more(chain, monkeypatch):
    from rcdms_amd.engine import UNetProgram
    b = chain
    built, captured = [], []
    init, capture = UNetProgram.__init__, UNetProgram.capture

    def counting_init(self, *a, **kw):
        built.append(kw.get("rank1_runs"))
        return init(self, *a, **kw)

    def counting_capture(self, *a, **kw):
        captured.append(self.rank1_runs)
        return capture(self, *a, **kw)
    monkeypatch.setattr(UNetProgram, "__init__", counting_init)
    monkeypatch.setattr(UNetProgram, "capture", counting_capture)

    def live():
        gc.collect()
        return sum(type(o) is UNetProgram for o in gc.get_objects())
    call(b, output_type="uint8")
    patterns = {v["prog"].rank1_runs for v in b.pipe._loop._variants.values()}
    assert len(patterns) == 4 and len(b.pipe.unet._programs) <= b.pipe.unet.MAX_LIVE_PLANS
    # every plan the loop keeps is one the model keeps
    assert all(any(v["prog"] is p for p in b.pipe.unet._programs.values()) for v in b.pipe._loop._variants.values())
    built.clear(), captured.clear()
    call(b, output_type="uint8")
    assert built == [] and captured == []                  # the second call replays what the first one built
    live2 = live()
    call(b, output_type="uint8")
    assert built == [] and captured == [] and live() == live2
    assert len(b.pipe.unet._programs) <= b.pipe.unet.MAX_LIVE_PLANS and len(b.pipe._loop._variants) == 4
    # a plain call afterwards: the plan of tests/test_story_gpu.py's chain test — the two seen rows of every story lead its
    # ten context rows — which is pass 0's, so nothing is built for it either
    res = call(b, stage2_autoreg=False, output_type="uint8")
    assert b.pipe._loop.rank1_runs == tuple((s * 5, s * 5 + 2) for s in range(S)) and b.pipe._loop.shared
    assert built == [] and captured == [] and res.frames_u8 is None


def decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def test_files_hold_the_handed_off_bytes(chain, run):
    b, (res, d) = chain, run
    u8 = res.frames_u8.cpu().numpy()
    targets = b.runner.target_frames(b.frames[:S].to(DEV)).cpu().numpy()
    assert sorted(p.name for p in (d / "metric").iterdir()) == sorted(f"{k}_{i}.png" for k in (7, 9) for i in range(5))
    assert sorted(p.name for p in (d / "grid").iterdir()) == ["7.png", "9.png"]
    for s, k in enumerate((7, 9)):
        for i in range(5):
            assert np.array_equal(decode((d / "metric" / f"{k}_{i}.png").read_bytes()), u8[s, i])
        grid = decode((d / "grid" / f"{k}.png").read_bytes())
        assert grid.shape == (2 * H, 5 * W, 3)
        assert np.array_equal(grid[:H], np.concatenate(list(u8[s]), axis=1))           # the generated row …
        assert np.array_equal(grid[H:], np.concatenate(list(targets[s]), axis=1))      # … over the target row


def test_png_output_is_the_files(chain, tmp_path):
    res = call(chain, output_type="png", frames_dir=str(tmp_path), indices=["a", "b"])
    assert len(res.videos) == S and all(len(v) == 5 for v in res.videos)
    u8 = res.frames_u8.cpu().numpy()
    for s, k in enumerate(("a", "b")):
        for i in range(5):
            assert isinstance(res.videos[s][i], bytes) and (tmp_path / f"{k}_{i}.png").read_bytes() == res.videos[s][i]
            assert np.array_equal(decode(res.videos[s][i]), u8[s, i])


def test_metrics_come_from_the_handed_off_bytes(chain, run):
    from rcdms_amd.metrics import frame_metrics
    b, (res, _) = chain, run
    fm = frame_metrics(res.frames_u8, b.runner.target_frames(b.frames[:S].to(DEV)))
    assert tuple(res.ssim.shape) == (S, 5) and tuple(res.psnr.shape) == (S, 5) and res.clip_i is None
    assert torch.equal(res.ssim, fm.ssim.view(S, 5)) and torch.equal(res.psnr, fm.psnr.view(S, 5))
