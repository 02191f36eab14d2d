"""GPU: guidance rescale and stochastic DDIM (eta > 0) on the HIP path.

  1. rcdm_cfg_rescale_factor against the float64 factor at the budget of tests/guide_ref.py (K_REL = 2^-17; the CPU test
     test_guidance_host shows that shifted fp32 sums meet it and raw one-pass sums do not), on poisoned / guarded operands
     and a NaN-filled workspace; bitwise repeatable; stories isolated; constant predictions give exactly 1.
     Measured on an MI355X: |k / k64 - 1| <= 2^-22.6 over all 48 cases.
  2. the three `_scaled` step entries: NULL and a vector of ones are the unscaled entry bit for bit; with computed factors,
     whole schedules against the host step() fed by rescale_noise_cfg in fp64 (2e-5 relative, as test_hip_sigma_step).
  3. DDIMScheduler.eta_table() through rcdm_cfg_sigma_step against step(eta=..., variance_noise=...).
  4. DenoiseLoop on the tiny UNet against a reference flow that rescales and steps on the host.
  5. the CFG-split mode with rescale against the batch-2S loop.
  6. RCDMsPipeline.__call__ with guidance_rescale / eta on the tiny stand-ins of tests/test_pipeline_e2e.py."""
import math

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from rcdms_amd import synth
from rcdms_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                 LMSDiscreteScheduler, PNDMScheduler, rescale_noise_cfg)
from tests import guide_ref as G
from tests.guard import check_in, check_out
from tests.test_hip_kernels import gout, gvec, h16, rows_from_5d, ws
from tests.test_hip_sigma_step import CASES, KW, _tiny
from tests.test_hip_unet import _tiny_story, build, check, rel_rms

pytestmark = pytest.mark.gpu
DEV = "cuda"


def eps_rows(eps, f, H, W, ld):
    """guide_ref's (2 S, f H W, 4) -> the guarded f16 rows the kernels read."""
    x = torch.from_numpy(eps).reshape(eps.shape[0], f, H, W, 4).permute(0, 4, 1, 2, 3).contiguous()
    return rows_from_5d(x, ld)


def factor_out(S):
    """fp32 [S] for the factors: NaN-filled, between NaN guard bands."""
    return gout(1, S, dtype=torch.float32, guard_rows=1)


def device_factor(rows, ld, S, f, H, W, g, phi):
    from rcdms_amd import hip
    nbytes = hip.cfg_rescale_workspace_bytes(S, f, H, W)
    work, fac = ws(nbytes), factor_out(S)
    hip.cfg_rescale_factor(rows.data_ptr(), ld, S, f, H, W, g, phi, work.data_ptr(), nbytes, fac.data_ptr())
    torch.cuda.synchronize()
    return fac


# ---- 1. the factor -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", G.RATIOS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=[str(s) for s in G.SHAPES])
def test_rescale_factor_vs_float64(hiplib, shape, ratio):
    S, f, H, W, ld = shape
    eps = G.make_eps(S, f, H, W, ratio, G.seed_of(shape, ratio))
    rows = eps_rows(eps, f, H, W, ld)
    for g in G.SCALES:
        for phi in G.PHIS:
            fac = device_factor(rows, ld, S, f, H, W, g, phi)
            k = fac[0].cpu().double().numpy()
            ref = G.k64(eps, g, phi)
            r = G.rel(k, ref)
            print(f"{shape} ratio {ratio} g {g} phi {phi}: |k / k64 - 1| = 2^{math.log2(r + 1e-30):.1f}  k = {k}")
            assert np.isfinite(k).all() and r <= G.K_REL, (g, phi, r, k, ref)
            again = device_factor(rows, ld, S, f, H, W, g, phi)
            assert torch.equal(fac[0], again[0]), "two calls on the same input differ"
            check_out(fac)
            check_in(rows)


def test_rescale_factor_constant_prediction_is_one(hiplib):
    """std(e) == 0: the guard — exactly 1.0f, not inf / nan; and a story next to it is computed as usual."""
    S, f, H, W, ld = 2, 3, 5, 7, 8
    eps = G.make_eps(S, f, H, W, 16, 5)
    eps[0], eps[S] = 0.75, -1.5                      # story 0: both halves constant
    fac = device_factor(eps_rows(eps, f, H, W, ld), ld, S, f, H, W, 7.5, 0.7)
    k = fac[0].cpu()
    assert k[0].item() == 1.0
    assert G.rel(k[1:].double().numpy(), G.k64(eps, 7.5, 0.7)[1:]) <= G.K_REL
    check_out(fac)


def test_rescale_factor_stories_are_isolated(hiplib):
    S, f, H, W, ld = G.SHAPES[0]
    a = G.make_eps(S, f, H, W, 16, 21)
    b = a.copy()
    other = G.make_eps(S, f, H, W, 0.35, 22)
    b[1], b[S + 1] = other[1], other[S + 1]         # story 1 swapped for another input
    ka = device_factor(eps_rows(a, f, H, W, ld), ld, S, f, H, W, 7.5, 0.7)[0].cpu()
    kb = device_factor(eps_rows(b, f, H, W, ld), ld, S, f, H, W, 7.5, 0.7)[0].cpu()
    assert torch.equal(ka[0], kb[0]) and torch.equal(ka[2], kb[2]) and not torch.equal(ka[1], kb[1])
    assert G.rel(kb.double().numpy(), G.k64(b, 7.5, 0.7)) <= G.K_REL


# ---- 2. the scaled steps -------------------------------------------------------------------------------------------
def _ddim(n):
    s = DDIMScheduler(clip_sample=False, steps_offset=1, **KW)
    s.set_timesteps(n)
    return s


def _pndm(n):
    s = PNDMScheduler(skip_prk_steps=True, steps_offset=1, **KW)
    s.set_timesteps(n)
    return s


def _sigma_case(name, n=None):
    _, cls, extra, steps = next(c for c in CASES if c[0] == name)
    s = cls(**KW, **extra)
    s.set_timesteps(n or steps)
    return s


class StepState:
    """The device state of one schedule: latents (and history / model_in / noise where the scheduler has them), each between
    NaN guard bands, with both the unscaled and the `_scaled` entry behind one call."""

    def __init__(self, kind, sched, lat, noise, S, f, H, W, gs, reps=2):
        from rcdms_amd import hip
        self.hip, self.kind, self.dims, self.gs, self.reps = hip, kind, (S, f, H, W), gs, reps
        n = lat.numel()
        self.lat_h = gout(1, n, dtype=torch.float32, guard_rows=1)
        self.lat_h[0].copy_(lat.reshape(-1))
        self.lat = self.lat_h.view(lat.shape)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.noise = None
        if kind == "ddim":
            self.tab = gvec(sched.coefficients())
        elif kind == "pndm":
            self.tab = gvec(sched.plms_table())
            self.hist = gout(5, n, dtype=torch.float32, guard_rows=1)
        else:
            self.tab = gvec(sched if torch.is_tensor(sched) else sched.sigma_table())
            self.hist = gout(3, n, dtype=torch.float32, guard_rows=1)
            self.xin_h = gout(1, n, dtype=torch.float32, guard_rows=1)
            self.model_in = self.xin_h.view(lat.shape)
            if noise is not None:
                self.noise = gvec(noise)

    def run(self, rows, ld, factor="unscaled"):
        """factor: "unscaled" -> the entry as it was; None -> `_scaled` with NULL; a tensor -> `_scaled` with it."""
        hip, (S, f, H, W), R = self.hip, self.dims, self.reps
        scaled = not isinstance(factor, str)
        k = () if not scaled else (0 if factor is None else factor.data_ptr(),)
        if self.kind == "ddim":
            fn = hip.cfg_ddim_step_scaled if scaled else hip.cfg_ddim_step
            fn(rows.data_ptr(), ld, self.lat.data_ptr(), S, R, f, H, W, self.gs, self.tab.data_ptr(), self.step.data_ptr(), *k)
        elif self.kind == "pndm":
            fn = hip.cfg_pndm_step_scaled if scaled else hip.cfg_pndm_step
            fn(rows.data_ptr(), ld, self.lat.data_ptr(), self.hist.data_ptr(), S, R, f, H, W, self.gs, self.tab.data_ptr(),
               self.step.data_ptr(), *k)
        else:
            fn = hip.cfg_sigma_step_scaled if scaled else hip.cfg_sigma_step
            fn(rows.data_ptr(), ld, self.lat.data_ptr(), self.model_in.data_ptr(), self.hist.data_ptr(),
               0 if self.noise is None else self.noise.data_ptr(), S, R, f, H, W, self.gs, self.tab.data_ptr(),
               self.step.data_ptr(), *k)
        hip.advance_step(self.step.data_ptr())
        torch.cuda.synchronize()

    def check(self):
        check_out(self.lat_h)
        check_in(self.tab)
        if self.kind != "ddim":
            check_out(self.hist)
        if self.kind == "sigma":
            check_out(self.xin_h)
            if self.noise is not None:
                check_in(self.noise)


SCHEDULES = [("ddim", "ddim", lambda: _ddim(10)), ("pndm", "pndm", lambda: _pndm(10)),
             ("euler_a", "sigma", lambda: _sigma_case("euler_a")), ("lms", "sigma", lambda: _sigma_case("lms")),
             ("dpmpp_2m", "sigma", lambda: _sigma_case("dpmpp_2m"))]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,kind,mk", SCHEDULES, ids=[c[0] for c in SCHEDULES])
def test_scaled_step_null_and_ones_are_the_unscaled_step(hiplib, name, kind, mk):
    """Three copies of the state through a whole schedule: the old entry, `_scaled` with NULL, `_scaled` with ones."""
    S, f, H, W, gs, ld = 2, 5, 8, 8, 7.5, 32
    g = torch.Generator().manual_seed(23)
    sched = mk()
    T = len(sched.timesteps)
    lat = torch.randn(S, 4, f, H, W, generator=g) * float(getattr(sched, "init_noise_sigma", 1.0))
    noise = torch.randn(T, S, 4, f, H, W, generator=g) if getattr(sched, "noise_needed", False) else None
    states = [StepState(kind, sched, lat, noise, S, f, H, W, gs) for _ in range(3)]
    ones = gvec(torch.ones(S))
    for i in range(T):
        rows = rows_from_5d(h16(torch.randn(2 * S, 4, f, H, W, generator=g)), ld)
        for st, fac in zip(states, ("unscaled", None, ones)):
            st.run(rows, ld, fac)
        for st in states[1:]:
            assert _bits_equal(st.lat, states[0].lat), (name, i)
            if kind == "sigma":
                assert _bits_equal(st.model_in, states[0].model_in), (name, i)
        check_in(rows)
    for st in states:
        st.check()
    check_in(ones)


def _host_step(sched, e, t, x, noise):
    if isinstance(sched, EulerAncestralDiscreteScheduler):
        return sched.step(e, t, x, noise=noise).prev_sample
    return sched.step(e, t, x).prev_sample


@pytest.mark.parametrize("name,kind,mk", SCHEDULES, ids=[c[0] for c in SCHEDULES])
def test_scaled_step_with_device_factors_vs_host(hiplib, name, kind, mk):
    """factor kernel + `_scaled` step over a whole schedule against rescale_noise_cfg + step() in fp64.  The stories' noise
    predictions get different scales and offsets, so their factors differ; LMS / DPM-Solver++ read the history, which has
    to hold the rescaled prediction (d of the table form), PNDM likewise."""
    from rcdms_amd import hip
    S, f, H, W, gs, phi, ld = 2, 5, 8, 8, 7.5, 0.7, 32
    g = torch.Generator().manual_seed(29)
    sched = mk()
    T = len(sched.timesteps)
    lat = torch.randn(S, 4, f, H, W, generator=g) * float(getattr(sched, "init_noise_sigma", 1.0))
    noise = torch.randn(T, S, 4, f, H, W, generator=g) if getattr(sched, "noise_needed", False) else None
    st = StepState(kind, sched, lat, noise, S, f, H, W, gs)
    nbytes = hip.cfg_rescale_workspace_bytes(S, f, H, W)
    x = lat.double()
    spread = torch.tensor([0.6, 1.7, 1.5, 0.5]).view(2 * S, 1, 1, 1, 1)   # (uncond s0, s1, cond s0, s1)
    for i, t in enumerate(sched.timesteps.tolist()):
        eps = h16(torch.randn(2 * S, 4, f, H, W, generator=g) * spread + 0.3)
        rows = rows_from_5d(eps, ld)
        work, fac = ws(nbytes), factor_out(S)
        hip.cfg_rescale_factor(rows.data_ptr(), ld, S, f, H, W, gs, phi, work.data_ptr(), nbytes, fac.data_ptr())
        st.run(rows, ld, fac[0])
        e_u, e_c = eps.double().chunk(2)
        e = e_u + gs * (e_c - e_u)
        e_r = rescale_noise_cfg(e, e_c, phi)
        k_ref = (e_r.reshape(S, -1)[:, 0] / e.reshape(S, -1)[:, 0]).numpy()
        assert G.rel(fac[0].cpu().double().numpy(), k_ref) <= G.K_REL and abs(k_ref[0] - k_ref[1]) > 1e-3, (i, k_ref)
        x = _host_step(sched, e_r, t, x, None if noise is None else noise[i].double())
        bound = 2e-5 * max(1.0, x.abs().max().item())
        err = (st.lat.cpu().double() - x).abs().max().item()
        assert err < bound, (name, i, err, bound)
        # the unrescaled update is far outside the bound: the test cannot pass on an ignored factor
        if i == 0:
            x_plain = _host_step(mk(), e, t, lat.double(), None if noise is None else noise[0].double())
            assert (x_plain - x).abs().max().item() > 100 * bound
        check_out(fac)
        check_in(rows)
    st.check()
    assert int(st.step.item()) == T


# ---- 3. eta --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reps", [2, 1])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_eta_table_through_sigma_step(hiplib, eta, reps):
    S, f, H, W, gs, n, ld = 2, 5, 8, 8, 2.5, 10, 32
    g = torch.Generator().manual_seed(31)
    sched = _ddim(n)
    tab = sched.eta_table(eta)
    lat = torch.randn(S, 4, f, H, W, generator=g)
    noise = torch.randn(n, S, 4, f, H, W, generator=g)
    st = StepState("sigma", tab, lat, noise, S, f, H, W, gs, reps=reps)
    x = lat.double()
    for i, t in enumerate(sched.timesteps.tolist()):
        eps = h16(torch.randn(reps * S, 4, f, H, W, generator=g))
        rows = rows_from_5d(eps, ld)
        st.run(rows, ld)
        e = eps.double()
        if reps == 2:
            e_u, e_c = e.chunk(2)
            e = e_u + gs * (e_c - e_u)
        x = sched.step(e, t, x, eta=eta, variance_noise=noise[i].double()).prev_sample
        bound = 2e-5 * max(1.0, x.abs().max().item())
        assert (st.lat.cpu().double() - x).abs().max().item() < bound, (eta, reps, i)
        assert (st.model_in.cpu().double() - x).abs().max().item() < bound, (eta, reps, i)       # cin_next = 1
        check_in(rows)
    st.check()


# ---- 4. the loop ---------------------------------------------------------------------------------------------------
def guided_flow(sd, cfg, sched, latents, mask, masked, ctx, n, gs, phi=0.0, eta=0.0, noises=None):
    """RCDMs_pipeline.py:480-497 with the host scheduler, rescale_noise_cfg between the CFG combine and step(), and eta /
    the per-step noise handed to step()."""
    sched.set_timesteps(n)
    x = latents * sched.init_noise_sigma
    for i, t in enumerate(sched.timesteps):
        xin = sched.scale_model_input(torch.cat([x] * 2), t)
        e_u, e_c = O.unet_forward(sd, cfg, torch.cat([xin, mask, masked], dim=1), t, ctx).chunk(2)
        eps = rescale_noise_cfg(e_u + gs * (e_c - e_u), e_c, phi)
        if isinstance(sched, DDIMScheduler):
            x = sched.step(eps, t, x, eta=eta, variance_noise=None if eta == 0.0 else noises[i]).prev_sample
        else:
            x = sched.step(eps, t, x).prev_sample
    return x


LOOP_GS = 2.0      # as test_denoise_loop_sigma_vs_reference_flow; the reference flows are ~0.1 apart with / without rescale
LOOP_CASES = [("ddim_rescale", lambda: DDIMScheduler(clip_sample=False, steps_offset=1, **KW), 0.7, 0.0),
              ("dpmpp_2m_rescale", lambda: DPMSolverMultistepScheduler(**KW), 0.7, 0.0),
              ("ddim_eta", lambda: DDIMScheduler(clip_sample=False, steps_offset=1, **KW), 0.0, 1.0)]


@pytest.mark.parametrize("name,mk,phi,eta", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_denoise_loop_guided_vs_reference_flow(hiplib, name, mk, phi, eta):
    from rcdms_amd.sampler import DenoiseLoop
    m, sd, cfg = _tiny()
    s = _tiny_story(1)
    n, gs = 5, LOOP_GS
    rms_tol, max_tol = 3.3e-3, 3e-3
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    loop = DenoiseLoop(m, 1, 5, 16, 16, 13, gs, mk(), n, guidance_rescale=phi, eta=eta)
    assert loop.phi == phi and loop.eta == eta and loop.sigma == (eta > 0 or name.startswith("dpmpp"))
    loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"], generator=gen() if eta else None)
    noises = None
    if eta:   # the T draws are T randn calls of the latents' shape, in step order, from the caller's generator
        g = gen()
        want = torch.stack([torch.randn(tuple(s["latents"].shape), generator=g, device=DEV) for _ in range(n)])
        assert torch.equal(loop.noise, want)
        noises = want.cpu()
    args = (s["latents"], s["mask"], s["masked_latents"], s["ctx"], n, gs)
    with torch.no_grad():
        ref = guided_flow(sd, cfg, mk(), *args, phi=phi, eta=eta, noises=noises)
        plain = guided_flow(sd, cfg, mk(), *args)
    # the argument matters: with it ignored the result would land on `plain`, more than 10 tolerances away
    apart = rel_rms(ref, plain)
    print(f"{name}: reference flows with and without the argument are {apart:.3e} apart (rel-RMS)")
    assert apart > 10 * rms_tol, apart
    out = loop.run().clone()
    check(out, ref, rms_tol, max_tol, f"{n}-step {name} loop")
    loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"], generator=gen() if eta else None)
    out2 = loop.run().clone()
    loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"], generator=gen() if eta else None)
    out3 = loop.run(use_graph=False).clone()
    assert torch.equal(out, out2), "a replay of the captured graph is not reproducible"
    assert torch.equal(out, out3), "graph != eager"


# ---- 5. CFG-split --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def comm1(hiplib):
    from rcdms_amd import hip
    c = hip.Comm(hip.Comm.unique_id(), 1, 0)
    yield c
    c.close()


def test_cfg_split_rescaled_loop_equals_unsplit_loop(comm1):
    """Pattern of test_cfg_split_sigma_loop_equals_unsplit_loop (LMS, halves 0 and 1 in lockstep on one device): the factors
    are computed from the gathered predictions on every rank, so both ranks scale alike and equal the batch-2S loop."""
    from rcdms_amd.dist import CfgSplit
    from rcdms_amd.sampler import DenoiseLoop
    m, m_other = build("unet_tiny"), build("unet_tiny")
    S, steps, phi = 2, 4, 0.7
    s = synth.synthetic_story(stories=S, latent_hw=(16, 16), ctx_len=13, ctx_dim=64, cfg=True, seed=21)
    s["masked_latents"][S:] += 0.05
    mk = lambda: LMSDiscreteScheduler(**KW)
    ref_loop = DenoiseLoop(m, S, 5, 16, 16, 13, 2.0, mk(), steps, guidance_rescale=phi)
    ref_loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
    ref = ref_loop.run().clone()
    plain_loop = DenoiseLoop(m, S, 5, 16, 16, 13, 2.0, mk(), steps)
    plain_loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
    assert not torch.equal(plain_loop.run(), ref)

    sent = []
    halves = [DenoiseLoop(mod, S, 5, 16, 16, 13, 2.0, mk(), steps, guidance_rescale=phi,
                          cfg_split=CfgSplit(h, lambda a, b, n, h=h: sent.append((h, a, b, n))))
              for h, mod in ((0, m), (1, m_other))]
    for lp in halves:
        lp.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
        assert lp.prog.b == S and lp.sigma and lp.factor is not None
    st = halves[0].prog.stream
    with torch.cuda.stream(st):
        for _ in range(steps):
            for lp in halves:
                for op in lp._pre:
                    op()
                lp.prog.run_body(skip_time=True)
            for lp in halves:
                lp._post[0]()
            (_, a0, _, n0), (_, a1, _, n1) = sent
            for lp in halves:
                comm1.allgather(a0, lp.eps_full.data_ptr(), n0)
                comm1.allgather(a1, lp.eps_full.data_ptr() + n0, n0)
            sent.clear()
            for lp in halves:
                for op in lp._post[1:]:
                    op()
        st.synchronize()
    assert torch.equal(halves[0].lat, halves[1].lat) and torch.equal(halves[0].factor, halves[1].factor)
    check(halves[0].lat, ref.cpu(), 3.5e-3, 5e-3, "CFG-split rescaled LMS loop vs batch-2S loop")


# ---- 6. the pipeline -----------------------------------------------------------------------------------------------
H6 = W6 = 128
h6 = w6 = 16
STEPS6, GS6, PHI6 = 3, LOOP_GS, 0.7
CAPS6 = [["pororo waves", "loopy sings", "eddy builds", "crong jumps", "poby fishes"],
         ["harry reads", "petty", "rody the robot walks in", "tongtong flies", "a snowy day"]]


@pytest.fixture(scope="module")
def guided(hiplib):
    """The pipeline of tests/test_story_gpu.py (the stand-ins of tests/test_pipeline_e2e.py with the HIP VAE, which the batch
    tolerance STAGE2_BOUND belongs to), two different stories, and the reference video of story s by the oracles."""
    from oracle import context_oracle as CO
    from oracle import vae_oracle as VO
    from tests.test_pipeline_e2e import _Text, _Tok
    from tests.test_story_gpu import stage2_bundle
    text, tok = _Text(), _Tok()
    b = stage2_bundle(text, tok, 32, 24)
    emb = text.emb.weight.detach().cpu().clone()
    b.src = [synth.normal_tensor("e2e.src", (5, 3, H6, W6), 2) * 0.5, synth.normal_tensor("guide.src", (5, 3, H6, W6), 6) * 0.8]
    b.img1 = [synth.normal_tensor("e2e.img1", (1, 9, 32), 3), synth.normal_tensor("guide.img1", (1, 9, 32), 7)]
    b.proj0 = [synth.normal_tensor("e2e.proj0", (4, 1, 24), 4), synth.normal_tensor("guide.proj0", (4, 1, 24), 8)]
    b.lat0 = [synth.normal_tensor("e2e.lat", (1, 4, 5, h6, w6), 5), synth.normal_tensor("guide.lat", (1, 4, 5, h6, w6), 9)]
    b.mask_label = torch.zeros(1, 5, h6, w6)
    b.mask_label[:, 0] = 1.0
    b.gen = lambda s: torch.Generator(device=DEV).manual_seed(9 + s)
    ml = torch.cat([b.mask_label[0], b.mask_label[0]])
    seen = (ml.reshape(10, -1) == 1).all(1)
    mk = lambda: DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)

    def call(s, **kw):
        return b.pipe(CAPS6[s], b.src[s].to(DEV), image_embeds_1=b.img1[s].to(DEV), proj_embeds_0=b.proj0[s].to(DEV),
                      mask_label=b.mask_label.to(DEV), video_length=5, height=H6, width=W6, num_inference_steps=STEPS6,
                      guidance_scale=GS6, latents=b.lat0[s].to(DEV), generator=b.gen(s), **kw).videos

    def draws(s):
        """What story s's generator hands out: the posterior noise of the VAE encode, then one draw per step."""
        g = b.gen(s)
        enc = torch.randn(5, 4, h6, w6, generator=g, device=DEV).cpu()
        return enc, torch.stack([torch.randn((1, 4, 5, h6, w6), generator=g, device=DEV) for _ in range(STEPS6)]).cpu()

    def videos(s, variants):
        """Reference videos (1, 3, 5, H, W) of story s, one per (phi, eta) of `variants`."""
        te = torch.cat([emb[tok([""] * 5).input_ids], emb[tok(CAPS6[s]).input_ids]])
        ctx = torch.cat([CO.context_stack_forward(b.sd_l, torch.cat([b.img1[s]] * 2), te[seen]),
                         CO.context_stack_forward(b.sd_g, torch.cat([b.proj0[s]] * 2), te[~seen])])
        enc, noises = draws(s)
        out = []
        with torch.no_grad():
            z = VO.vae_encode_sample(b.sd_vae, b.vcfg, b.src[s], enc)
            masked = torch.cat([z.reshape(1, 5, 4, h6, w6).permute(0, 2, 1, 3, 4) * 0.18215] * 2)
            for phi, eta in variants:
                lat = guided_flow(b.sd_unet, b.cfg, mk(), b.lat0[s], ml.view(2, 1, 5, h6, w6), masked, ctx, STEPS6, GS6,
                                  phi=phi, eta=eta, noises=noises)
                v = VO.vae_decode(b.sd_vae, b.vcfg, (lat / 0.18215).permute(0, 2, 1, 3, 4).reshape(5, 4, h6, w6))
                out.append((v.reshape(1, 5, 3, H6, W6).permute(0, 2, 1, 3, 4) / 2 + 0.5).clamp(0, 1))
        return out

    b.call, b.draws, b.videos = call, draws, videos
    return b


def test_pipeline_guidance_rescale_and_eta(guided):
    """One call with neither argument (unchanged code: its rel-RMS r0 against its reference flow is the yardstick), one with
    guidance_rescale, one with eta and a seeded generator: each within 2 r0 of its OWN reference flow, the references more
    than 10 r0 apart, so an ignored argument cannot pass."""
    b = guided
    pipe = b.pipe
    ref_plain, ref_phi, ref_eta = b.videos(0, [(0.0, 0.0), (PHI6, 0.0), (0.0, 1.0)])
    out_plain = b.call(0)
    assert tuple(out_plain.shape) == (1, 3, 5, H6, W6)
    r0 = rel_rms(out_plain.float(), ref_plain)
    loop_plain = pipe._loop
    assert loop_plain.phi == 0.0 and loop_plain.eta == 0.0 and not loop_plain.sigma and loop_plain.factor is None
    d_phi, d_eta = rel_rms(ref_phi, ref_plain), rel_rms(ref_eta, ref_plain)
    print(f"pipeline, plain call: r0 = {r0:.3e}; references apart: rescale {d_phi:.3e}, eta {d_eta:.3e}")
    assert d_phi > 10 * r0 and d_eta > 10 * r0, (r0, d_phi, d_eta)

    out_phi = b.call(0, guidance_rescale=PHI6)
    loop_phi = pipe._loop
    r_phi = rel_rms(out_phi.float(), ref_phi)
    out_eta = b.call(0, eta=1.0)
    loop_eta = pipe._loop
    r_eta = rel_rms(out_eta.float(), ref_eta)
    print(f"pipeline: guidance_rescale {PHI6}: {r_phi:.3e}; eta 1.0: {r_eta:.3e}  (bound 2 r0 = {2 * r0:.3e})")
    assert r_phi <= 2 * r0 and r_eta <= 2 * r0, (r0, r_phi, r_eta)
    assert loop_phi is not loop_plain and loop_phi.phi == PHI6
    assert loop_eta is not loop_phi and loop_eta.eta == 1.0 and loop_eta.sigma
    assert torch.equal(loop_eta.noise.cpu(), b.draws(0)[1])           # after the encode's draw, T draws in step order
    b.call(0, guidance_rescale=0.3)                                   # another phi: not the cached loop
    assert pipe._loop is not loop_eta and pipe._loop.phi == 0.3
    again = b.call(0, guidance_rescale=PHI6)
    assert torch.equal(again, out_phi)


def test_pipeline_two_stories_keep_their_own_factors(guided):
    """Two different stories in one call with guidance_rescale equal their two single-story calls at the batch tolerance of
    tests/test_story_gpu.py: the factor is per story, not per batch."""
    from tests.test_story_gpu import STAGE2_BOUND
    b = guided
    single = [b.call(s, guidance_rescale=PHI6) for s in range(2)]
    both = b.pipe(CAPS6, torch.stack(b.src).to(DEV), image_embeds_1=[t.to(DEV) for t in b.img1],
                  proj_embeds_0=[t.to(DEV) for t in b.proj0], mask_label=torch.cat([b.mask_label] * 2).to(DEV), video_length=5,
                  height=H6, width=W6, num_inference_steps=STEPS6, guidance_scale=GS6, latents=torch.cat(b.lat0).to(DEV),
                  generator=[b.gen(0), b.gen(1)], guidance_rescale=PHI6).videos
    loop = b.pipe._loop
    assert loop.S == 2 and loop.phi == PHI6 and tuple(loop.factor.shape) == (2,)
    k = loop.factor.cpu()
    print(f"pipeline, 2-story call: factors of the last step {k.tolist()}")
    assert abs(k[0].item() - k[1].item()) > 1e-3                      # the stories do differ
    for s in range(2):
        r = rel_rms(both[s:s + 1].float(), single[s].float())
        print(f"pipeline, story {s} of a 2-story call vs its own call: rel-RMS {r:.3e}")
        assert r <= STAGE2_BOUND, (s, r)
    assert rel_rms(single[0].float(), single[1].float()) > 10 * STAGE2_BOUND
