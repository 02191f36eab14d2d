"""CPU: the host side of story batches (rcdms_amd.story and the story axis of the two pipelines) — the context-row
placement against an explicit triple loop, argument validation, the stage-1 `.npy` hand-off files, and the per-runner cache
of the black / white image embeddings with stand-in modules."""
import types

import numpy as np
import pytest
import torch

from rcdms_amd import story as ST
from rcdms_amd.scheduler import DDIMScheduler, UnCLIPScheduler
from src.pipelines.RCDMs_pipeline import RCDMsPipeline
from src.pipelines.prior_pipeline import Seq_Inpaint_Prior_Pipeline

E = 8
CAPS = [["a", "b b", "c", "d d d", "e"], ["f", "g", "h h", "i", "j"], ["k", "l", "m", "n n", "o"]]


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("reps", [1, 2])
def test_place_story_rows_matches_triple_loop(S, reps):
    L, D = 3, 2
    rows = [torch.arange(reps * 5 * L * D, dtype=torch.float32).view(reps * 5, L, D) + 1000.0 * s for s in range(S)]
    got = ST.place_story_rows(rows, reps)
    want = torch.full((reps * S * 5, L, D), float("nan"))
    for r in range(reps):
        for s in range(S):
            for f in range(5):
                want[(r * S + s) * 5 + f] = rows[s][r * 5 + f]
    assert got.shape == want.shape and torch.equal(got, want)
    if S == 1:
        assert torch.equal(got, rows[0])                              # one story: the identity
    masks = [r[:, 0] for r in rows]                                   # any trailing shape: the mask rows go the same way
    assert torch.equal(ST.place_story_rows(masks, reps), want[:, 0])


def test_place_story_rows_rejects_ragged_stories():
    with pytest.raises(ValueError):
        ST.place_story_rows([torch.zeros(10, 2), torch.zeros(5, 2)], 2)
    with pytest.raises(ValueError):
        ST.place_story_rows([torch.zeros(10, 2), torch.zeros(10, 3)], 2)


def test_story_count():
    assert ST.story_count("one caption") is None
    assert ST.story_count(CAPS[0]) is None                            # today's form: a flat list of five captions
    assert ST.story_count(CAPS) == 3 and ST.story_count([CAPS[1]]) == 1
    with pytest.raises(ValueError, match="mixes"):
        ST.story_count([CAPS[0], "stray caption"])
    with pytest.raises(ValueError, match="5 caption strings"):
        ST.story_count([CAPS[0], CAPS[1][:4]])
    with pytest.raises(ValueError):
        ST.story_count([CAPS[0], [1, 2, 3, 4, 5]])


def test_story_generators():
    g = [torch.Generator().manual_seed(i) for i in range(3)]
    assert ST.story_generators(g, 3) == g
    assert ST.story_generators(g[0], 3) == [g[0]] * 3 and ST.story_generators(None, 2) == [None, None]
    with pytest.raises(ValueError, match="generators"):
        ST.story_generators(g[:2], 3)


class _FakePrior:
    config = types.SimpleNamespace(embedding_dim=E)
    device = torch.device("cpu")


def _prior_pipe():
    return Seq_Inpaint_Prior_Pipeline(prior=_FakePrior(), image_encoder=None, text_encoder=None, tokenizer=None,
                                      scheduler=UnCLIPScheduler())


def test_prior_pipeline_story_axis_validation():
    """Every check fires before any module is touched (the stand-ins have none)."""
    pipe = _prior_pipe()
    ok = dict(imgs_proj_embeds1=torch.zeros(3, 5, 1, E), mask_label=torch.zeros(3, 5, 1, E), video_length=5)
    with pytest.raises(ValueError, match="mixes"):
        pipe([CAPS[0], "x"], **ok)
    for name, bad in (("imgs_proj_embeds1", torch.zeros(2, 5, 1, E)), ("imgs_proj_embeds1", torch.zeros(5, 1, E)),
                      ("mask_label", torch.zeros(4, 5, 1, E)), ("latents", torch.zeros(2, 5, E)),
                      ("latents", torch.zeros(15, E))):
        kw = dict(ok)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            pipe(CAPS, **kw)
    with pytest.raises(ValueError, match="generators"):
        pipe(CAPS, generator=[torch.Generator(), torch.Generator()], **ok)


class _FakeUNet:
    class config:
        sample_size = 2
    device = torch.device("cpu")


def _stage2_pipe():
    return RCDMsPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_FakeUNet(), local_module=None, global_module=None,
                         scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear"))


def test_stage2_pipeline_story_axis_validation():
    pipe = _stage2_pipe()
    H = W = 16
    ok = dict(source_img=torch.zeros(3, 5, 3, H, W), mask_label=torch.zeros(3, 5, 2, 2), video_length=5, height=H, width=W,
              image_embeds_1=[torch.zeros(1, 4, 6)] * 3, proj_embeds_0=[torch.zeros(4, 1, 6)] * 3)
    with pytest.raises(ValueError, match="mixes"):
        pipe(["x", CAPS[0]], **ok)
    for name, bad in (("source_img", torch.zeros(2, 5, 3, H, W)), ("source_img", torch.zeros(5, 3, H, W)),
                      ("mask_label", torch.zeros(2, 5, 2, 2)), ("latents", torch.zeros(1, 4, 5, 2, 2)),
                      ("image_embeds_1", [torch.zeros(1, 4, 6)] * 2), ("image_embeds_1", torch.zeros(3, 1, 4, 6)),
                      ("proj_embeds_0", [torch.zeros(4, 1, 6)] * 4)):
        kw = dict(ok)
        kw[name] = bad
        with pytest.raises(ValueError, match=name):
            pipe(CAPS, **kw)
    with pytest.raises(ValueError, match="generators"):
        pipe(CAPS, generator=[torch.Generator()] * 4, **ok)


def test_vae_calls_go_in_whole_stories_past_two_stories_at_512():
    pipe = _stage2_pipe()
    sizes = lambda x, scale=1: [c.shape[0] for c in pipe._vae_chunks(x, scale)]
    assert sizes(torch.zeros(5, 3, 512, 512)) == [5] and sizes(torch.zeros(5, 3, 1024, 1024)) == [5]   # one story: one call
    assert sizes(torch.zeros(15, 3, 128, 128)) == [15]                      # small frames: one call over 5 * S frames
    assert sizes(torch.zeros(40, 3, 256, 256)) == [40] and sizes(torch.zeros(45, 3, 256, 256)) == [40, 5]
    assert sizes(torch.zeros(10, 3, 512, 512)) == [10] and sizes(torch.zeros(25, 3, 512, 512)) == [10, 10, 5]
    assert sizes(torch.zeros(20, 4, 64, 64), 8) == [10, 10] and sizes(torch.zeros(10, 4, 128, 128), 8) == [5, 5]
    assert sizes(torch.zeros(15, 4, 16, 16), 8) == [15]
    x = torch.arange(20.0).view(20, 1, 1, 1).expand(20, 4, 64, 64)
    assert torch.equal(torch.cat(pipe._vae_chunks(x, 8)), x)


def test_stage1_npy_files_are_what_the_stage2_driver_loads(tmp_path):
    emb = torch.arange(5 * E, dtype=torch.float64).view(5, E) / 7          # any dtype in: fp32 on disk
    paths = ST.write_stage1_embeds(str(tmp_path / "embeds"), 42, emb)
    assert [p.split("/")[-1] for p in paths] == ["42_0.npy", "42_1.npy", "42_2.npy", "42_3.npy", "42_4.npy", "42.npy"]
    rows = []
    for j in range(1, 5):                                                  # stage2_batchtest_rcdms_model.py:291-294
        a = np.load("{}/{}_{}.npy".format(tmp_path / "embeds", 42, str(j)))
        assert a.dtype == np.float32 and a.shape == (E,)
        rows.append(torch.tensor(a).unsqueeze(0).unsqueeze(0))
    proj0 = torch.cat(rows, dim=0)
    assert tuple(proj0.shape) == (4, 1, E) and torch.equal(proj0[:, 0], emb[1:].float())
    whole = np.load(tmp_path / "embeds" / "42.npy")
    assert whole.dtype == np.float32 and whole.shape == (5, E) and np.array_equal(whole, emb.float().numpy())
    with pytest.raises(ValueError):
        ST.write_stage1_embeds(str(tmp_path), 1, torch.zeros(4, E))


class _CountingEncoder:
    """CLIP vision stand-in: image_embeds = per-channel mean of the pixel values, tiled to E."""
    config = types.SimpleNamespace(image_size=4)

    def __init__(self):
        self.batches = []

    def __call__(self, pixel_values):
        self.batches.append(pixel_values.shape[0])
        m = pixel_values.float().mean(dim=(2, 3))
        emb = torch.cat([m, m, m[:, :2]], dim=1)
        return types.SimpleNamespace(image_embeds=emb, last_hidden_state=emb[:, None, :].repeat(1, 3, 1))


class _Processor:
    def __call__(self, images=None, return_tensors="pt"):
        return types.SimpleNamespace(pixel_values=images.permute(0, 3, 1, 2).float() / 255.0)


class _EchoPrior:
    """Stage-1 stand-in: records its conditioning and returns imgs_proj_embeds1 + 1 as the embeddings."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def __call__(self, prompt, imgs_proj_embeds1, mask_label, **kw):
        self.calls.append((prompt, imgs_proj_embeds1.clone(), mask_label.clone()))
        return types.SimpleNamespace(image_embeds=imgs_proj_embeds1[:, :, 0] + 1.0)


def _frames(S):
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, 256, (S, 5, 6, 6, 3), dtype=torch.uint8, generator=g)


def test_runner_encodes_black_and_white_once():
    enc, prior = _CountingEncoder(), _EchoPrior()
    runner = ST.StoryRunner(prior, None, enc, clip_processor=_Processor())
    r1 = runner(_frames(3), [[c.upper() for c in s] for s in CAPS])
    assert enc.batches == [15, 2]                                          # the targets, then black + white in one forward
    r2 = runner(_frames(2), CAPS[:2])
    assert enc.batches == [15, 2, 10]                                      # the second call encodes its targets only
    assert prior.calls[0][0] == CAPS                                       # lower-cased, as the drivers do
    assert r1.videos is None and tuple(r1.image_embeds.shape) == (3, 5, E) and tuple(r2.cosine.shape) == (2, 5)
    # "continue": source [frame 0, black x 4], mask [white, black x 4]
    _, proj, label = prior.calls[0]
    black, white = torch.zeros(E), torch.ones(E)
    assert tuple(proj.shape) == (3, 5, 1, E) and torch.equal(proj[:, 0, 0], r1.target_embeds[:, 0])
    assert torch.equal(proj[:, 1:, 0], black.expand(3, 4, E)) and torch.equal(label[:, 0, 0], white.expand(3, E))
    assert torch.equal(label[:, 1:, 0], black.expand(3, 4, E))
    assert torch.equal(r1.cosine, torch.nn.functional.cosine_similarity(r1.image_embeds, r1.target_embeds, dim=-1))


def test_runner_modes_autoreg_passes_and_files(tmp_path):
    enc, prior = _CountingEncoder(), _EchoPrior()
    runner = ST.StoryRunner(prior, None, enc, clip_processor=_Processor())
    with pytest.raises(ValueError, match="stage2_batchtest_rcdms_model.py:367"):
        runner(_frames(1), CAPS[:1], mode="visualization", stage2=True)
    with pytest.raises(ValueError, match="check mode"):
        runner(_frames(1), CAPS[:1], mode="other")
    with pytest.raises(ValueError):
        runner(_frames(2), CAPS)                                           # two stories of frames, three of captions
    with pytest.raises(ValueError):
        runner(_frames(2), CAPS[:2], indices=[7])
    prior.calls.clear()
    res = runner(_frames(2), CAPS[:2], mode="visualization", autoreg=True, save_dir=str(tmp_path), indices=[7, 9])
    assert len(prior.calls) == 5
    black, white = torch.zeros(E), torch.ones(E)
    for i, (_, proj, label) in enumerate(prior.calls):
        # pass i: the i rows kept so far, then black; the first i mask entries white (pass 0: the mode's own rows)
        assert torch.equal(proj[:, :i, 0], res.image_embeds[:, :i]) and torch.equal(proj[:, i:, 0], black.expand(2, 5 - i, E))
        assert torch.equal(label[:, :i, 0], white.expand(2, i, E)) and torch.equal(label[:, i:, 0], black.expand(2, 5 - i, E))
    # the echo prior returns its input + 1: row i kept from pass i is (black + 1) = 1 for every i
    assert torch.equal(res.image_embeds, torch.ones(2, 5, E))
    assert np.array_equal(np.load(tmp_path / "9_3.npy"), np.ones(E, np.float32))
    assert np.load(tmp_path / "7.npy").shape == (5, E)
