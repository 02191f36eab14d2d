"""GPU: rcdms_amd.objective around the tiny UNet of tests/test_hip_unet.py — 16x16 latents, B = 3 stories with seen prefixes of
0, 1 and 4 frames at three distinct timesteps.  The device route against the torch-op route through the same unet.forward
(add_noise, cat, forward, float64 sums), bit for bit where the two must agree; the loss against the fp32 oracle on the CPU within
the bound that tests/test_hip_unet.py's own relative-RMS tolerance implies; isolation of the stories, graph replay,
StoryObjective on the tiny encoders of tests/test_story_gpu.py, and LossLog."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as UO
from rcdms_amd import synth
from tests import objective_oracle as O
from tests.test_hip_unet import build as build_unet
from tests.test_oracle_golden import weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, F, H, W, L, D = 3, 5, 16, 16, 13, 64
SEEN = (0, 1, 4)
T_STEPS = (37, 500, 981)
OFFSET = 0.1
RHO = 4e-3                      # tests/test_hip_unet.py::test_tiny_unet_vs_reference: rel-RMS of the whole tiny UNet, one call


def make_inputs(tag="objective"):
    n = lambda name, shape, seed: synth.normal_tensor(f"{tag}.{name}", shape, seed).to(DEV)
    mask = torch.tensor([[1.0 if i < k else 0.0 for i in range(F)] for k in SEEN])[:, None, :, None, None].expand(B, 1, F, H, W)
    return dict(latents=n("lat", (B, 4, F, H, W), 1), masked_latents=n("masked", (B, 4, F, H, W), 2), mask=mask.contiguous().to(DEV),
                context=n("ctx", (B * F, L, D), 3), noise=n("noise", (B, 4, F, H, W), 4), offsets=n("offs", (B, 4, F, 1, 1), 5),
                timesteps=torch.tensor(T_STEPS, dtype=torch.int64, device=DEV))


def rows_bits(r):
    """The int16 bits of a plan's row view, (M, C) on the host."""
    t = r.buf.t[2 * r.off:2 * r.off + 2 * r.M * r.ld].view(torch.int16).reshape(r.M, r.ld)[:, :r.C]
    torch.cuda.synchronize()
    return t.contiguous().cpu().numpy()


@pytest.fixture(scope="module")
def setup(hiplib):
    from rcdms_amd.objective import DenoisingObjective
    unet = build_unet("unet_tiny")
    obj = DenoisingObjective(unet, noise_offset=OFFSET)
    x = make_inputs()
    prog = unet.program(B, F, H, W, L, rank1_runs=unet._context_runs(x["context"]))
    # the torch-op route, what the parent of this feature can do: separate mul / add kernels, cat, forward, float64 sums
    n = x["noise"] + OFFSET * x["offsets"]
    xin = torch.cat([obj.scheduler.add_noise(x["latents"], n, x["timesteps"]), x["mask"], x["masked_latents"]], dim=1)
    with torch.no_grad():
        eps = unet(xin, x["timesteps"], x["context"], return_dict=False)[0]
    route_rows = rows_bits(prog.x_in)
    first = obj.loss(**x)
    fill_rows = rows_bits(prog.x_in)
    second = obj.loss(**x)
    return dict(unet=unet, obj=obj, x=x, prog=prog, n=n, xin=xin, eps=eps, route_rows=route_rows, fill_rows=fill_rows, first=first,
                second=second)


def test_fill_writes_the_rows_of_the_torch_route(setup):
    s = setup
    assert np.array_equal(s["fill_rows"], s["route_rows"])
    want = s["xin"].permute(0, 2, 3, 4, 1).reshape(-1, 9).half().view(torch.int16).cpu().numpy()
    assert np.array_equal(s["fill_rows"][:, :9], want) and not s["fill_rows"][:, 9:].any()


def test_sq_err_equals_the_float64_sums_of_the_torch_route(setup):
    s = setup
    r = s["first"]
    assert r.sq_err.dtype == torch.float64 and tuple(r.sq_err.shape) == (B, F) and r.sq_err.is_cuda
    d2 = (s["eps"].double() - s["n"].double()) ** 2                      # (B, 4, F, H, W)
    want = d2.sum(dim=(1, 3, 4)).cpu().numpy()
    got = r.sq_err.cpu().numpy()
    # both are sums of the same float64 terms in different orders: each within u (D + 3) sum of the exact sum (objective_oracle)
    tol = 2 * O.bound(1.0, H * W) * want
    print("sq_err", got, "torch route", want, "tolerance", tol)
    assert np.all(np.abs(got - want) <= tol)
    # and the kernel's own order on the UNet's f16 output rows, bit for bit
    eps_bits = s["eps"].permute(0, 2, 3, 4, 1).reshape(-1, 4).half().view(torch.int16).cpu().numpy().view(np.uint16)
    model = O.sqerr(eps_bits, s["x"]["noise"].cpu().numpy(), s["x"]["offsets"].reshape(B, 4, F).cpu().numpy(), OFFSET)
    assert O.same_bits(got, model)


def test_losses_are_consistent_with_sq_err(setup):
    r = setup["first"]
    sq = r.sq_err.cpu().numpy()
    per = 4 * H * W
    seen = np.array([[i < k for i in range(F)] for k in SEEN])
    assert np.array_equal(r.seen.cpu().numpy(), seen) and r.timesteps.tolist() == list(T_STEPS)
    close = lambda a, b: abs(float(a) - b) <= 32 * O.U * abs(b)          # two orders of at most 15 float64 additions each
    assert r.loss.dtype == torch.float64 and r.loss.dim() == 0
    assert close(r.loss, sq.sum() / (B * F * per))
    assert close(r.loss_seen, sq[seen].sum() / (seen.sum() * per)) and close(r.loss_unseen, sq[~seen].sum() / ((~seen).sum() * per))
    for b in range(B):
        assert close(r.per_story[b], sq[b].sum() / (F * per))
    # F.mse_loss(noise_pred, noise, reduction="mean") of the torch route, in float64
    want = torch.nn.functional.mse_loss(setup["eps"].double(), setup["n"].double()).item()
    assert abs(float(r.loss) - want) <= 2 * O.bound(1.0, H * W) * want


def test_loss_against_the_fp32_oracle(setup):
    """|L - L_o| <= 2 rho sqrt(L_o E) + rho^2 E with E = mean(eps_o^2): from ||eps - eps_o|| <= rho ||eps_o|| (the UNet's own
    bound) by the triangle inequality on sqrt(L) = ||eps - n|| / sqrt(N), and a^2 - b^2 = (a - b)(a + b)."""
    s = setup
    cfg = UO.tiny_config(width=64, cross_dim=64, layers_per_block=2)
    with torch.no_grad():
        eps_o = UO.unet_forward(weights("unet_tiny"), cfg, s["xin"].cpu(), s["x"]["timesteps"].cpu(), s["x"]["context"].cpu())
    n = s["n"].cpu().double()
    L_o = ((eps_o.double() - n) ** 2).mean().item()
    E = (eps_o.double() ** 2).mean().item()
    got = float(s["first"].loss)
    bound = 2 * RHO * (L_o * E) ** 0.5 + RHO ** 2 * E
    print(f"loss {got:.9e}, oracle {L_o:.9e}, |difference| {abs(got - L_o):.3e}, bound {bound:.3e}")
    assert abs(got - L_o) <= bound


def test_second_call_replays_the_first_calls_bits(setup):
    a, b = setup["first"], setup["second"]
    assert setup["prog"].graph is not None
    assert torch.equal(a.sq_err.view(torch.int64), b.sq_err.view(torch.int64)) and torch.equal(a.loss, b.loss)


def test_stories_are_isolated(setup):
    s = setup
    y = make_inputs("objective.other")
    x = {k: v.clone() for k, v in s["x"].items()}
    for k in ("latents", "masked_latents", "noise", "offsets"):
        x[k][1] = y[k][1]
    x["context"][F:2 * F] = y["context"][F:2 * F]
    x["timesteps"][1] = 640
    r = s["obj"].loss(**x)
    a, b = s["first"].sq_err.view(torch.int64), r.sq_err.view(torch.int64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


def test_drawn_operands_follow_the_documented_order(setup):
    s = setup
    x = {k: s["x"][k] for k in ("latents", "masked_latents", "mask", "context")}
    r = s["obj"].loss(**x, generator=torch.Generator(device=DEV).manual_seed(11))
    g = torch.Generator(device=DEV).manual_seed(11)
    noise = torch.randn((B, 4, F, H, W), generator=g, device=DEV)
    offs = torch.randn((B, 4, F, 1, 1), generator=g, device=DEV)
    t = torch.randint(0, 1000, (B,), generator=g, device=DEV)
    assert torch.equal(r.timesteps, t)
    again = s["obj"].loss(**x, noise=noise, offsets=offs, timesteps=t)
    assert torch.equal(r.sq_err.view(torch.int64), again.sq_err.view(torch.int64))


def test_a_mixed_mask_frame_is_refused_and_bad_timesteps_show(setup):
    s = setup
    x = dict(s["x"])
    x["mask"] = s["x"]["mask"].clone()
    x["mask"][1, 0, 2, 3, 3] = 1.0
    with pytest.raises(ValueError, match="please check mask label"):
        s["obj"].loss(**x)
    x = dict(s["x"])
    x["timesteps"] = torch.tensor([T_STEPS[0], 1000, T_STEPS[2]], dtype=torch.int64, device=DEV)
    r = s["obj"].loss(**x)
    nan = torch.isnan(r.sq_err).cpu()
    assert nan[1].all() and not nan[0].any() and not nan[2].any() and torch.isnan(r.loss)
    all_seen = dict(s["x"])
    all_seen["mask"] = torch.ones_like(s["x"]["mask"])
    r = s["obj"].loss(**all_seen)
    assert r.loss_unseen is None and abs(float(r.loss_seen) - float(r.loss)) <= 32 * O.U * float(r.loss)


def test_story_objective_equals_the_objective_on_its_batch(hiplib):
    from rcdms_amd import clip
    from rcdms_amd.image import ClipImageProcessor, FrameTransform
    from rcdms_amd.objective import DenoisingObjective, StoryObjective
    from tests.test_story_gpu import CAPS, T2, TEXT2_CFG, VISION_CFG, _ClipTok, clip_module, cuda_gen, stage2_bundle
    text, _ = clip_module(clip.CLIPTextEncoder, TEXT2_CFG, 32, with_projection=False)
    vision, _ = clip_module(clip.CLIPVisionEncoder, VISION_CFG, 33)
    tok = _ClipTok(T2)
    b = stage2_bundle(text, tok, VISION_CFG["hidden_size"], VISION_CFG["projection_dim"])
    pipe = b.pipe
    story = StoryObjective(DenoisingObjective(pipe.unet), pipe.vae, text, tok, vision, pipe.local_module, pipe.global_module,
                           frame_transform=FrameTransform(128, 128), clip_processor=ClipImageProcessor(size=56, crop_size=56))
    frames = torch.randint(0, 256, (B, 5, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    caps = [list(c) for c in CAPS]
    caps[1][3] = ""                                                       # a dropped caption
    t = torch.tensor(T_STEPS, dtype=torch.int64, device=DEV)
    got = story.loss(frames, caps, SEEN, timesteps=t, generator=cuda_gen(5))
    g = cuda_gen(5)
    batch = story.batch(frames, caps, SEEN, generator=g)
    assert tuple(batch["latents"].shape) == (B, 4, 5, 16, 16) and tuple(batch["mask"].shape) == (B, 1, 5, 16, 16)
    assert tuple(batch["context"].shape)[:2] == (B * 5, T2) and torch.isfinite(batch["context"]).all()
    seen = torch.tensor([[i < k for i in range(5)] for k in SEEN])
    assert torch.equal(batch["mask"][:, 0, :, 0, 0].cpu() == 1, seen)
    want = story.objective.loss(**batch, timesteps=t, generator=g)
    assert torch.equal(got.sq_err.view(torch.int64), want.sq_err.view(torch.int64)) and torch.equal(got.seen.cpu(), seen)
    assert torch.isfinite(got.sq_err).all() and got.loss_seen is not None and got.loss_unseen is not None
    # story 0 sees nothing and story 2 four frames: their source latents differ over those frames
    ml = batch["masked_latents"]
    assert ml.shape == batch["latents"].shape and not torch.equal(ml[2, :, :4], ml[0, :, :4])


def test_loss_log_of_two_appends_equals_one_of_the_concatenation(setup, tmp_path):
    from rcdms_amd.objective import LossLog, ObjectiveResult
    a, b = setup["first"], setup["obj"].loss(**{**setup["x"], "timesteps": torch.tensor([5, 999, 500], device=DEV)})
    two = LossLog(DEV).append(a).append(b)
    both = ObjectiveResult(sq_err=torch.cat([a.sq_err, b.sq_err]), loss=None, per_story=None,
                           timesteps=torch.cat([a.timesteps, b.timesteps]), seen=torch.cat([a.seen, b.seen]), loss_seen=None,
                           loss_unseen=None, frame_elements=a.frame_elements)
    one = LossLog(DEV).append(both)
    assert len(two) == len(one) == 2 * B
    ra, rb = two.result(bins=10), one.result(bins=10)
    for k in ("edges", "stories", "loss", "loss_seen", "loss_unseen"):
        x, y = getattr(ra, k), getattr(rb, k)
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), k
    assert ra.stories.tolist() == [2, 0, 0, 0, 0, 2, 0, 0, 0, 2] and ra.edges.tolist() == list(range(0, 1001, 100))
    sq = torch.cat([a.sq_err, b.sq_err]).cpu().numpy()
    rows = [0, 3]                                                          # timesteps 37 and 5: bin 0
    want = (sq[rows[0]].sum() + sq[rows[1]].sum()) / (2 * F * 4 * H * W)
    assert abs(ra.loss[0] - want) <= 32 * O.U * want and np.isnan(ra.loss[1])
    two.save(tmp_path / "log.npz")
    back = LossLog.load(tmp_path / "log.npz", DEV).result(bins=10)
    assert np.array_equal(back.loss.view(np.int64), ra.loss.view(np.int64)) and np.array_equal(back.stories, ra.stories)
