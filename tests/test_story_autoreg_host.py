"""CPU: the stage-2 autoregression of rcdms_amd.story.StoryRunner (stage2_autoreg=True) with stand-in modules — the five
passes' arguments against the pass table of StoryRunner.__call__, the device hand-off arithmetic bit for bit, one vision
forward per newly kept frame, the argument checks, the unchanged plain call, and the frames_dir / grid_dir files with a
stand-in encoder."""
import os
import types

import pytest
import torch

from rcdms_amd import story as ST
from tests.test_story_host import CAPS, E, _CountingEncoder, _EchoPrior, _Processor, _frames

S = 2
H = W = 16
SCALE = 8
PLAIN_KEYS = {"prompt", "source_img", "image_embeds_1", "proj_embeds_0", "mask_label", "video_length", "height", "width",
              "guidance_scale", "generator", "num_inference_steps", "output_type", "fix_context_order", "guidance_rescale", "eta"}


def fake_bytes(call, stories):
    """uint8 (S, 5, H, W, 3) that names (call, story, frame) in every pixel, with a little structure inside a frame."""
    base = torch.tensor([[40 * call + 7 * s + f + 1 for f in range(5)] for s in range(stories)], dtype=torch.int64)
    ripple = (torch.arange(H * W * 3) % 3).view(H, W, 3)
    return (base[:, :, None, None, None] + ripple).to(torch.uint8)


class _FakeStage2:
    """Stage-2 stand-in: records every call (tensors cloned) and returns frames that encode (call, story, frame)."""
    vae_scale_factor = SCALE
    unet = types.SimpleNamespace(config=types.SimpleNamespace(sample_size=H // SCALE))

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        rec = dict(kw)
        rec["source_img"], rec["mask_label"] = kw["source_img"].clone(), kw["mask_label"].clone()
        rec["image_embeds_1"] = [t.clone() for t in kw["image_embeds_1"]]
        rec["proj_embeds_0"] = [t.clone() for t in kw["proj_embeds_0"]]
        u8 = fake_bytes(len(self.calls), len(kw["prompt"]))
        self.calls.append(rec)
        if kw["output_type"] == "uint8":
            return types.SimpleNamespace(videos=u8)
        assert kw["output_type"] == "tensor"
        videos = u8.permute(0, 4, 1, 2, 3).float() / 255                       # (S, 3, 5, H, W)
        return types.SimpleNamespace(videos=videos, frames_u8=u8 if kw.get("return_uint8") else None)


class _Transform:
    height, width = H, W

    def __call__(self, frames):
        x = frames.permute(0, 3, 1, 2).float() / 127.5 - 1.0
        return torch.nn.functional.interpolate(x, size=(H, W))


def make_runner():
    enc, prior, stage2 = _CountingEncoder(), _EchoPrior(), _FakeStage2()
    runner = ST.StoryRunner(prior, stage2, enc, clip_processor=_Processor(), frame_transform=_Transform())
    return runner, enc, prior, stage2


def gens():
    return [torch.Generator().manual_seed(3), torch.Generator().manual_seed(4)]


def test_five_passes_follow_the_pass_table():
    runner, enc, prior, stage2 = make_runner()
    frames, g = _frames(S), gens()
    res = runner(frames, CAPS[:S], stage2_autoreg=True, generator=g, num_inference_steps=7, guidance_scale=3.0,
                 fix_context_order=True, guidance_rescale=0.3, eta=0.2)
    assert len(stage2.calls) == 5 and len(prior.calls) == 1                 # stage 1 ran once: `autoreg` is its own switch
    embeds = res.image_embeds
    assert tuple(embeds.shape) == (S, 5, E)
    # the targets, black + white, then one forward of S frames per newly kept frame (frames 0..3; frame 4 is never seen)
    assert enc.batches == [5 * S, 2, S, S, S, S]
    kept = torch.stack([fake_bytes(i, S)[:, i] for i in range(5)], dim=1)    # (S, 5, H, W, 3): frame i of call i
    assert res.frames_u8.dtype == torch.uint8 and torch.equal(res.frames_u8, kept)
    given0 = _Transform()(frames[:, 0])
    hidden0 = enc(_Processor()(images=frames[:, 0]).pixel_values).last_hidden_state
    for i, c in enumerate(stage2.calls):
        n = max(i, 1)
        seen = c["mask_label"].reshape(S, 5, -1)
        assert tuple(c["mask_label"].shape) == (S, 5, H // SCALE, W // SCALE)
        assert torch.equal(seen[:, :n], torch.ones_like(seen[:, :n])) and torch.equal(seen[:, n:], torch.zeros_like(seen[:, n:]))
        assert [int(seen[s].amax(dim=1).sum()) for s in range(S)] == [(1, 1, 2, 3, 4)[i]] * S
        assert tuple(c["source_img"].shape) == (S, 5, 3, H, W) and c["source_img"].dtype == torch.float32
        assert torch.equal(c["source_img"][:, n:], torch.full((S, 5 - n, 3, H, W), -1.0))
        if i == 0:
            assert torch.equal(c["source_img"][:, 0], given0)
        else:
            # the driver's PNG round trip of the kept bytes: ToTensor, Normalize([0.5], [0.5]), in fp32
            b = kept[:, :i].permute(0, 1, 4, 2, 3).to(torch.float32)
            assert torch.equal(c["source_img"][:, :i], (b / 255 - 0.5) / 0.5)
        for s in range(S):
            img1, proj0 = c["image_embeds_1"][s], c["proj_embeds_0"][s]
            assert (img1.shape[0], proj0.shape[0]) == ((1, 4), (1, 4), (2, 3), (3, 2), (4, 1))[i]
            assert tuple(proj0.shape) == (5 - n, 1, E) and torch.equal(proj0[:, 0], embeds[s, n:])
            if i == 0:
                assert torch.equal(img1, hidden0[s:s + 1])
            else:
                want = enc(_Processor()(images=kept[s, :i]).pixel_values).last_hidden_state
                assert torch.equal(img1, want)
        assert c["generator"] is g and all(a is b for a, b in zip(c["generator"], g))
        assert (c["num_inference_steps"], c["guidance_scale"], c["fix_context_order"], c["guidance_rescale"], c["eta"]) == \
            (7, 3.0, True, 0.3, 0.2)
        assert c["prompt"] == CAPS[:S] and c["output_type"] == "tensor" and c["return_uint8"] is True
    # "tensor": frame i of the result is frame i of call i
    assert tuple(res.videos.shape) == (S, 3, 5, H, W)
    for i in range(5):
        assert torch.equal(res.videos[:, :, i], fake_bytes(i, S)[:, i].permute(0, 3, 1, 2).float() / 255)


def test_uint8_layout_and_one_shared_generator():
    runner, enc, prior, stage2 = make_runner()
    g = torch.Generator().manual_seed(9)
    res = runner(_frames(S), CAPS[:S], stage2_autoreg=True, output_type="uint8", generator=g)
    assert len(stage2.calls) == 5 and all(c["generator"] is g and c["output_type"] == "uint8" for c in stage2.calls)
    assert all("return_uint8" not in c for c in stage2.calls)
    assert tuple(res.videos.shape) == (S, 5, H, W, 3) and torch.equal(res.videos, res.frames_u8)
    for i in range(5):
        assert torch.equal(res.videos[:, i], fake_bytes(i, S)[:, i])


def test_argument_checks():
    runner, enc, prior, stage2 = make_runner()
    with pytest.raises(ValueError, match="stage2_batchtest_rcdms_model.py:367"):
        runner(_frames(S), CAPS[:S], mode="visualization", stage2=True, stage2_autoreg=True)
    with pytest.raises(ValueError, match="no stage 2"):
        runner(_frames(S), CAPS[:S], stage2=False, stage2_autoreg=True)
    with pytest.raises(ValueError, match="no stage 2"):
        runner(_frames(S), CAPS[:S], mode="visualization", stage2_autoreg=True)     # stage 2 is off by default there
    with pytest.raises(ValueError, match="no stage 2"):
        ST.StoryRunner(_EchoPrior(), None, _CountingEncoder(), clip_processor=_Processor())(
            _frames(S), CAPS[:S], stage2_autoreg=True)
    for bad in ("numpy", "pil", None):
        with pytest.raises(ValueError, match="output_type"):
            runner(_frames(S), CAPS[:S], stage2_autoreg=True, output_type=bad)
    with pytest.raises(ValueError, match="no stage 2"):
        runner(_frames(S), CAPS[:S], stage2=False, frames_dir="unused")
    with pytest.raises(ValueError, match="output_type"):
        runner(_frames(S), CAPS[:S], grid_dir="unused", output_type="numpy")
    assert stage2.calls == [] and not os.path.exists("unused")


def test_plain_call_is_todays_call():
    runner, enc, prior, stage2 = make_runner()
    frames, g = _frames(S), gens()
    res = runner(frames, CAPS[:S], stage2_autoreg=False, generator=g, num_inference_steps=7, output_type="uint8")
    assert len(stage2.calls) == 1 and enc.batches == [5 * S, 2]
    c = stage2.calls[0]
    assert set(c) == PLAIN_KEYS                                              # nothing new reaches the pipeline
    assert c["generator"] is g and c["output_type"] == "uint8" and c["num_inference_steps"] == 7 and c["video_length"] == 5
    assert (c["height"], c["width"], c["guidance_scale"], c["fix_context_order"], c["guidance_rescale"], c["eta"]) == \
        (H, W, 7.5, False, 0.0, 0.0)
    assert torch.equal(c["source_img"][:, 0], _Transform()(frames[:, 0]))
    assert torch.equal(c["source_img"][:, 1:], torch.full((S, 4, 3, H, W), -1.0))
    assert torch.equal(c["mask_label"][:, 0], torch.ones(S, 2, 2)) and torch.equal(c["mask_label"][:, 1:], torch.zeros(S, 4, 2, 2))
    hidden0 = enc(_Processor()(images=frames[:, 0]).pixel_values).last_hidden_state
    for s in range(S):
        assert torch.equal(c["image_embeds_1"][s], hidden0[s:s + 1])
        assert torch.equal(c["proj_embeds_0"][s][:, 0], res.image_embeds[s, 1:])
    assert res.frames_u8 is None and torch.equal(res.videos, fake_bytes(0, S))


def test_plan_key_is_the_runs_the_plan_uses():
    from rcdms_amd.engine import XATTN_MAX_KEYS, plan_rank1_runs
    assert plan_rank1_runs(None, 10, 13) is None
    assert plan_rank1_runs([[0, 2], (5, 7)], 20, 13) == ((0, 2), (5, 7))     # any sequence in, one hashable form out
    assert plan_rank1_runs(((0, 10),), 10, 13) is None and plan_rank1_runs(((0, 4), (4, 10)), 10, 13) is None   # all full rank
    assert plan_rank1_runs(((0, 2),), 10, XATTN_MAX_KEYS + 1) is None        # too long for the rank-1 form: the general plan
    assert plan_rank1_runs(((0, 2),), 10, XATTN_MAX_KEYS) == ((0, 2),)


class _FakeProgram:
    def __init__(self, runs):
        self.rank1_runs = runs

    def time_table(self, timesteps):
        return torch.zeros(len(timesteps), 4)


class _FakeModel:
    """The model side of the plan bookkeeping with UNet3DConditionModel's rules: an LRU of `bound` plans keyed by the runs, a
    notice to every watcher for each plan let go."""
    device = torch.device("cpu")

    def __init__(self, bound):
        self.bound, self.plans, self.built, self.users = bound, {}, [], []

    def watch_plans(self, user):
        self.users.append(user)

    def program(self, b, frames, H, W, L, shared_prefix=False, rank1_runs=None):
        key = (b, shared_prefix, rank1_runs)
        prog = self.plans.pop(key, None)
        if prog is None:
            while len(self.plans) >= self.bound:
                gone = self.plans.pop(next(iter(self.plans)))
                for u in self.users:
                    u.plan_dropped(gone)
            prog = _FakeProgram(rank1_runs)
            self.built.append(rank1_runs)
        self.plans[key] = prog
        return prog


def test_loop_keeps_no_plan_the_model_let_go():
    from rcdms_amd.sampler import DenoiseLoop
    from rcdms_amd.scheduler import DDIMScheduler
    model = _FakeModel(bound=4)
    loop = DenoiseLoop(model, 2, 5, 8, 8, 13, 2.0, DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                                                                steps_offset=1, clip_sample=False), 4)
    assert model.users == [loop]
    patterns = [((0, 2), (5, 7)), ((0, 4), (5, 9)), ((0, 11), (15, 16)), ((0, 12), (15, 17))]   # 1, 2, 3, 4 seen frames, S = 2
    for _ in range(3):                                       # three autoregressive calls: passes 0 and 1 share a pattern
        for runs in [patterns[0]] + patterns:
            loop._select(True, runs)
            assert loop.rank1_runs == runs and loop.prog is model.plans[(4, True, runs)]
    assert model.built == patterns and len(loop._variants) == 4
    # requests that end in the same plan share one entry: a list for a tuple, every image full rank for no runs at all
    loop._select(True, [list(r) for r in patterns[0]])
    loop._select(True, ((0, 20),))
    assert model.built == patterns + [None] and loop.rank1_runs is None
    # ... and that fifth plan pushed the least recently used one out of the model, and with it out of the loop
    assert len(loop._variants) == 4 and (True, patterns[1]) not in loop._variants
    assert {id(v["prog"]) for v in loop._variants.values()} == {id(p) for p in model.plans.values()}
    loop._select(True, None)
    assert model.built == patterns + [None]


def test_model_tells_its_watchers_which_plans_it_drops():
    from src.models.unet import UNet3DConditionModel
    with torch.device("meta"):
        m = UNet3DConditionModel(in_channels=9, cross_attention_dim=64, block_out_channels=(64, 128, 256, 256),
                                 use_motion_module=False, unet_use_cross_frame_attention=False,
                                 unet_use_temporal_attention=False)

    class Watcher:
        def __init__(self):
            self.dropped = []

        def plan_dropped(self, prog):
            self.dropped.append(prog)
    a, b = Watcher(), Watcher()
    m.watch_plans(a)
    m.watch_plans(b)
    m._programs = {"k1": "plan 1", "k2": "plan 2"}
    gen = m._weights_gen
    del b                                                    # watchers are held weakly
    m._invalidate()                                          # new weights: every plan goes
    assert a.dropped == ["plan 1", "plan 2"] and m._programs == {} and m._weights_gen == gen + 1
    assert len(m._plan_users) == 1


@pytest.mark.parametrize("autoreg", [True, False])
def test_files_are_written_only_when_asked(tmp_path, monkeypatch, autoreg):
    """The encoders are stand-ins (the real ones run on the device: tests/test_story_autoreg_gpu.py): a frame's "file" is its
    first pixel, a grid's "file" the first pixels of its ten cells."""
    from rcdms_amd import checkpoint, image
    encoded = []

    def fake_encode(frames, filter="adaptive", match=False):
        encoded.append(tuple(frames.shape))
        return [b"F" + bytes(f[0, 0].tolist()) for f in frames]

    def fake_grid(cells, rows, cols, match=False):
        assert (rows, cols) == (2, 5) and len(cells) == 10
        return b"G" + b"".join(bytes(c[0, 0].tolist()) for c in cells)
    monkeypatch.setattr(image, "encode_png", fake_encode)
    monkeypatch.setattr(checkpoint, "story_grid_png", fake_grid)
    monkeypatch.chdir(tmp_path)
    runner, enc, prior, stage2 = make_runner()
    targets = torch.full((S, 5, H, W, 3), 200, dtype=torch.uint8) + torch.arange(5, dtype=torch.uint8).view(1, 5, 1, 1, 1)
    monkeypatch.setattr(runner, "target_frames", lambda frames: targets)
    res = runner(_frames(S), CAPS[:S], stage2_autoreg=autoreg, output_type="uint8")
    assert encoded == [] and os.listdir(tmp_path) == []                      # no directory given: nothing encoded or written
    fdir, gdir = tmp_path / "metric", tmp_path / "grid"
    stage2.calls.clear()                                                     # the stand-in numbers its frames by call
    res = runner(_frames(S), CAPS[:S], stage2_autoreg=autoreg, output_type="uint8", frames_dir=str(fdir), indices=[7, 9])
    assert encoded == [(S * 5, H, W, 3)] and not gdir.exists()
    u8 = res.videos
    assert sorted(os.listdir(fdir)) == sorted(f"{k}_{i}.png" for k in (7, 9) for i in range(5))
    for s, k in enumerate((7, 9)):
        for i in range(5):
            assert (fdir / f"{k}_{i}.png").read_bytes() == b"F" + bytes(u8[s, i, 0, 0].tolist())
    stage2.calls.clear()
    res = runner(_frames(S), CAPS[:S], stage2_autoreg=autoreg, output_type="png", grid_dir=str(gdir), indices=[7, 9])
    assert sorted(os.listdir(gdir)) == ["7.png", "9.png"] and len(os.listdir(fdir)) == 10
    for s, k in enumerate((7, 9)):
        # "png": the frame files come back as the result; the grid is the generated row over the target row
        assert res.videos[s] == [b"F" + bytes(u8[s, i, 0, 0].tolist()) for i in range(5)]
        assert (gdir / f"{k}.png").read_bytes() == b"G" + b"".join(
            [bytes(u8[s, i, 0, 0].tolist()) for i in range(5)] + [bytes(targets[s, i, 0, 0].tolist()) for i in range(5)])
    assert (res.frames_u8 is not None) == autoreg
