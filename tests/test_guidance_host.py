"""CPU: guidance rescale and stochastic DDIM (eta > 0) above the kernels.

  * the budget of tests/guide_ref.py is a real one: the fp32 emulation with shifted sums is inside K_REL on every case
    the GPU test runs, the raw one-pass emulation is outside it at |mean| / std = 64 and 256 on every shape;
  * rescale_noise_cfg against the float64 formula; DDIMScheduler.eta_table() / step(eta=...) against each other and against
    closed forms; DenoiseLoop's dispatch on a host-only UNet stand-in; argument validation and symbols of the new entries."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rcdms_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler, PNDMScheduler,
                                 rescale_noise_cfg)
from tests import guide_ref as G
from tests.test_cabi_symbols import declared_symbols

EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
KW = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


# ---- the budget ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.SHAPES, ids=[str(s[:4]) for s in G.SHAPES])
def test_budget_separates_shifted_from_one_pass(shape):
    S, f, H, W, _ = shape
    worst_shifted = 0.0
    for ratio in G.RATIOS:
        eps = G.make_eps(S, f, H, W, ratio, G.seed_of(shape, ratio))
        for g in G.SCALES:
            for phi in G.PHIS:
                ref = G.k64(eps, g, phi)
                a, b = G.rel(G.k32(eps, g, phi, True), ref), G.rel(G.k32(eps, g, phi, False), ref)
                print(f"{shape[:4]} ratio {ratio} g {g} phi {phi}: shifted 2^{math.log2(a + 1e-30):.1f}, "
                      f"one-pass 2^{math.log2(b + 1e-30):.1f}")
                assert a <= G.K_REL, (ratio, g, phi, a)
                if ratio >= 64:
                    assert b > G.K_REL, (ratio, g, phi, b)
                worst_shifted = max(worst_shifted, a)
    print(f"{shape[:4]}: worst shifted 2^{math.log2(worst_shifted):.1f} against K_REL 2^-17")


@pytest.mark.parametrize("ratio", G.RATIOS)
def test_generator_keeps_its_promises(ratio):
    S, f, H, W, _ = G.SHAPES[0]
    eps = G.make_eps(S, f, H, W, ratio, G.seed_of(G.SHAPES[0], ratio))
    assert eps.shape == (2 * S, f * H * W, 4) and eps.dtype == np.float32
    assert np.array_equal(eps, eps.astype(np.float16).astype(np.float32)) and np.isfinite(eps).all()
    x = eps.astype(np.float64).reshape(2 * S, -1)
    mean, std = x.mean(axis=1), x.std(axis=1, ddof=1)
    for s in range(S):
        assert np.sign(mean[s]) == np.sign(mean[S + s]) == (1.0 if s % 2 == 0 else -1.0)
    got = np.abs(mean) / std
    print(f"ratio {ratio}: |mean| / std after the f16 rounding {got}")
    assert np.all(np.abs(got / ratio - 1.0) < 0.05)
    if ratio != 0.35:
        assert np.all((np.abs(mean) > 3.9) & (np.abs(mean) < 1010.0))
        assert len({round(float(abs(m)), 3) for m in mean[:S]}) == S      # every story its own offset
    assert np.array_equal(eps, G.make_eps(S, f, H, W, ratio, G.seed_of(G.SHAPES[0], ratio)))


# ---- rescale_noise_cfg ---------------------------------------------------------------------------------------------
def _cfg_pair(S=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    e_u = torch.randn(S, 4, 5, 6, 7, generator=g, dtype=torch.float64) * 0.8 + 0.1
    e_c = torch.randn(S, 4, 5, 6, 7, generator=g, dtype=torch.float64) * torch.tensor([0.5, 1.0, 2.0]).view(S, 1, 1, 1, 1) - 0.2
    return e_u, e_c, e_u + 7.5 * (e_c - e_u)


def test_rescale_noise_cfg():
    e_u, e_c, e = _cfg_pair()
    assert rescale_noise_cfg(e, e_c, 0.0) is e                                # phi = 0: the input, bitwise
    out = rescale_noise_cfg(e, e_c, 1.0)                                       # phi = 1: the conditional prediction's std
    flat = lambda t: t.reshape(t.shape[0], -1)
    assert torch.allclose(flat(out).std(dim=1), flat(e_c).std(dim=1), rtol=1e-12, atol=0)
    for phi in (0.7, 0.25):
        out = rescale_noise_cfg(e, e_c, phi)
        k = phi * flat(e_c).std(dim=1) / flat(e).std(dim=1) + (1 - phi)
        assert torch.allclose(out, e * k.view(-1, 1, 1, 1, 1), rtol=1e-13, atol=0)
        kn = G.k64(np.concatenate([flat(e_u).numpy(), flat(e_c).numpy()]).reshape(6, -1, 4), 7.5, phi)
        assert np.allclose(k.numpy(), kn, rtol=1e-12, atol=0)
    # the guard: a constant guided prediction is left as it is (diffusers: inf / nan)
    const = torch.full((2, 4, 5, 2, 2), 0.25, dtype=torch.float64)
    assert torch.equal(rescale_noise_cfg(const, torch.randn(2, 4, 5, 2, 2, dtype=torch.float64), 0.7), const)
    # fp32 in, fp32 out
    assert rescale_noise_cfg(e.float(), e_c.float(), 0.7).dtype == torch.float32


# ---- DDIM eta ------------------------------------------------------------------------------------------------------
def _replay(tab, x, es, zs):
    """The row rule of include/rcdm.h in fp64 on the fp32 table."""
    t = tab.double()
    for i in range(t.shape[0]):
        px, pe, a, b, w1, w2, w3, c = t[i, :8].tolist()
        assert w1 == w2 == w3 == 0.0 and t[i, 9] == -1 and t[i, 8] == 1.0 and t[i, 13] == 1.0 and (px, pe) == (0.0, 1.0)
        d = px * x + pe * es[i]
        x = a * x + b * d + c * zs[i]
    return x


@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_eta_table_equals_step(eta):
    n = 10
    sched = DDIMScheduler(clip_sample=False, steps_offset=1, **KW)
    sched.set_timesteps(n)
    tab = sched.eta_table(eta)
    assert tuple(tab.shape) == (n, 16) and tab.dtype == torch.float32
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, 4, 5, 4, 4, generator=g, dtype=torch.float64)
    es = [torch.randn(2, 4, 5, 4, 4, generator=g, dtype=torch.float64) for _ in range(n)]
    zs = [torch.randn(2, 4, 5, 4, 4, generator=g, dtype=torch.float64) for _ in range(n)]
    x = x0
    for i, t in enumerate(sched.timesteps.tolist()):
        x = sched.step(es[i], t, x, eta=eta, variance_noise=zs[i]).prev_sample
    got = _replay(tab, x0, es, zs)
    scale = max(1.0, x.abs().max().item())
    err = (got - x).abs().max().item()
    print(f"eta {eta}: table replay vs step() {err:.2e} (scale {scale:.2f})")
    assert err <= 2e-6 * scale


def test_eta_closed_forms():
    n = 10
    sched = DDIMScheduler(clip_sample=False, steps_offset=1, **KW)
    sched.set_timesteps(n)
    ac = sched.alphas_cumprod.double()
    ratio = 1000 // n
    co = sched.coefficients().double()
    t0 = sched.eta_table(1e-30).double()                      # eta -> 0: the deterministic update
    for i, t in enumerate(sched.timesteps.tolist()):
        sa, s1a, sp, s1p = co[i].tolist()
        assert t0[i, 2].item() == pytest.approx(sp / sa, rel=1e-6)
        assert t0[i, 3].item() == pytest.approx(s1p - sp * s1a / sa, rel=1e-5, abs=1e-6)
        assert t0[i, 7].item() == pytest.approx(0.0, abs=1e-25)
    for eta in (0.3, 1.0):
        tab = sched.eta_table(eta).double()
        for i, t in enumerate(sched.timesteps.tolist()):
            a_t = ac[t].item()
            a_p = ac[t - ratio].item() if t - ratio >= 0 else 1.0
            sig = tab[i, 7].item()
            dirc = tab[i, 3].item() + a_p ** 0.5 * (1 - a_t) ** 0.5 / a_t ** 0.5      # sqrt(1 - a_p - sigma^2)
            assert dirc ** 2 + sig ** 2 == pytest.approx(1 - a_p, rel=1e-5, abs=1e-7)
            if eta == 1.0:                                     # the DDPM posterior variance between t and prev
                beta = 1 - a_t / a_p
                assert sig ** 2 == pytest.approx((1 - a_p) / (1 - a_t) * beta, rel=1e-5, abs=1e-12)
        # set_alpha_to_one: no noise is added by the last step
        assert tab[-1, 7].item() == 0.0 and (tab[:-1, 7] > 0).all()


def test_eta_step_draws_every_step_in_order():
    n = 4
    sched = DDIMScheduler(clip_sample=False, steps_offset=1, **KW)
    sched.set_timesteps(n)
    shape = (1, 4, 5, 2, 2)
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    x = y = torch.ones(shape)
    e = torch.full(shape, 0.5)
    for t in sched.timesteps.tolist():
        x = sched.step(e, t, x, eta=1.0, generator=g).prev_sample
        y = sched.step(e, t, y, eta=1.0, variance_noise=torch.randn(shape, generator=g2)).prev_sample
    assert torch.equal(x, y)
    # the last step (sigma = 0) consumed a draw all the same: both generators are in the same state
    assert torch.equal(torch.randn(3, generator=g), torch.randn(3, generator=g2))
    # eta = 0 draws nothing and is the update it was
    g3 = torch.Generator().manual_seed(5)
    sched.step(e, int(sched.timesteps[0]), x, eta=0.0, generator=g3)
    assert torch.equal(torch.randn(3, generator=g3), torch.randn(3, generator=torch.Generator().manual_seed(5)))
    with pytest.raises(ValueError, match="both"):
        sched.step(e, int(sched.timesteps[0]), x, eta=0.5, generator=g3, variance_noise=e)


# ---- DenoiseLoop dispatch ------------------------------------------------------------------------------------------
class FakeUNet:
    device = torch.device("cpu")


def test_denoise_loop_dispatch():
    _lib()
    from rcdms_amd.sampler import DenoiseLoop
    S, T = 2, 10
    ddim = lambda: DDIMScheduler(clip_sample=False, steps_offset=1, **KW)
    lp = DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, ddim(), T, eta=0.5)
    assert lp.sigma and not lp.pndm and not lp.multistep and lp.eta == 0.5
    assert tuple(lp.coef.shape) == (T, 16) and tuple(lp.noise.shape) == (T, S, 4, 5, 8, 8)
    assert lp.model_in is not None and lp.x_in is lp.model_in and lp.timesteps.dtype == torch.int64
    assert torch.equal(lp.coef, ddim_table(ddim(), T, 0.5))
    # the T draws: T randn calls of the latents' shape, in step order, one generator per story when a list is given
    g, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for _ in range(3):
        assert torch.equal(lp._randn(g), torch.randn(S, 4, 5, 8, 8, generator=g2))
    gs = [torch.Generator().manual_seed(4), torch.Generator().manual_seed(5)]
    per = torch.cat([torch.randn(1, 4, 5, 8, 8, generator=torch.Generator().manual_seed(k)) for k in (4, 5)])
    assert torch.equal(lp._randn(gs), per)

    lp = DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, ddim(), T)                     # eta = 0: as it was
    assert not lp.sigma and tuple(lp.coef.shape) == (T, 4) and lp.noise is None and lp.model_in is None
    assert lp.factor is None and lp.phi == 0.0 and lp.eta == 0.0
    for mk in (lambda: PNDMScheduler(skip_prk_steps=True, **KW), lambda: EulerDiscreteScheduler(**KW),
               lambda: DPMSolverMultistepScheduler(**KW)):                            # every other type ignores eta
        a, b = DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, mk(), T, eta=0.5), DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, mk(), T)
        assert a.eta == 0.0 and a.noise is None and torch.equal(a.coef, b.coef) and a.sigma == b.sigma and a.pndm == b.pndm

    lp = DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 7.5, ddim(), T, guidance_rescale=0.7)
    assert lp.phi == 0.7 and tuple(lp.factor.shape) == (S,) and lp.factor.dtype == torch.float32
    assert lp._guide_ws.numel() >= S * 16 and not lp.sigma
    lp = DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 1.0, ddim(), T, guidance_rescale=0.7)   # no CFG: nothing to rescale
    assert lp.reps == 1 and lp.phi == 0.0 and lp.factor is None

    class NoTable(DDIMScheduler):               # a DDIM-shaped scheduler from elsewhere: the stride, but no eta_table()
        def __getattribute__(self, k):
            if k == "eta_table":
                raise AttributeError(k)
            return super().__getattribute__(k)

    with pytest.raises(NotImplementedError, match="eta_table"):
        DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, NoTable(clip_sample=False, steps_offset=1, **KW), T, eta=0.5)
    with pytest.raises(NotImplementedError, match="clip_sample"):
        DenoiseLoop(FakeUNet(), S, 5, 8, 8, 13, 2.0, DDIMScheduler(clip_sample=True, **KW), T, eta=0.5)


def ddim_table(sched, T, eta):
    sched.set_timesteps(T)
    return sched.eta_table(eta)


def test_pipeline_signature_and_loop_key():
    import inspect

    from rcdms_amd.story import StoryRunner
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    p = inspect.signature(RCDMsPipeline.__call__).parameters
    assert p["guidance_rescale"].default == 0.0 and p["guidance_rescale"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert p["eta"].default == 0.0
    for fn in (RCDMsPipeline.denoise, RCDMsPipeline._sample_and_decode, RCDMsPipeline._call_stories, StoryRunner.__call__):
        q = inspect.signature(fn).parameters
        assert q["guidance_rescale"].default == 0.0 and q["eta"].default == 0.0, fn


# ---- the C ABI -----------------------------------------------------------------------------------------------------
NEW = ("rcdm_cfg_rescale_workspace_bytes", "rcdm_cfg_rescale_factor", "rcdm_cfg_ddim_step_scaled",
       "rcdm_cfg_pndm_step_scaled", "rcdm_cfg_sigma_step_scaled")


def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in NEW:
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name), name
    assert lib.rcdm_version() == 0x000300


def test_workspace_bytes():
    hip, lib = _lib()
    for S, f, H, W, _ in G.SHAPES:
        n = hip.cfg_rescale_workspace_bytes(S, f, H, W)
        assert n >= 16 * S and n % 16 == 0
        assert hip.cfg_rescale_workspace_bytes(2 * S, f, H, W) == 2 * n          # per story
    assert hip.cfg_rescale_workspace_bytes(1, 5, 64, 64) <= 4096                   # a few partials, not a slab
    for bad in ((0, 5, 8, 8), (1, 0, 8, 8), (1, 5, -1, 8), (1, 5, 8, 0)):
        assert hip.cfg_rescale_workspace_bytes(*bad) == 0


def test_rescale_factor_argument_checks():
    """Every refusal comes before any device work: the pointers are never dereferenced (on a box without a GPU a launch
    would come back as RCDM_ELAUNCH, not as the code asserted here)."""
    hip, lib = _lib()
    eps, ws, fac = 0x1000, 0x2000, 0x3000
    need = hip.cfg_rescale_workspace_bytes(2, 5, 8, 8)
    F = ctypes.c_float
    call = lambda **o: lib.rcdm_cfg_rescale_factor(o.get("eps", eps), o.get("ld", 32), o.get("S", 2), o.get("f", 5),
                                                   o.get("H", 8), o.get("W", 8), F(7.5), F(0.7), o.get("ws", ws),
                                                   o.get("nbytes", need), o.get("fac", fac), None)
    for bad in (dict(eps=None), dict(ws=None), dict(fac=None), dict(ld=3), dict(S=0), dict(f=0), dict(H=-1), dict(W=0),
                dict(ws=ws + 2)):
        assert call(**bad) == EINVAL, bad
    assert call(nbytes=need - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    assert call(S=70000, nbytes=1 << 30) == ESHAPE


def test_scaled_step_argument_checks():
    hip, lib = _lib()
    p, F = ctypes.c_void_p(16), ctypes.c_float(1.0)
    for factor in (None, p):
        ddim = lambda **o: lib.rcdm_cfg_ddim_step_scaled(o.get("eps", p), o.get("ld", 32), o.get("lat", p), o.get("S", 1),
                                                         o.get("reps", 2), 5, 8, o.get("W", 8), F, o.get("tab", p),
                                                         o.get("step", p), factor, None)
        pndm = lambda **o: lib.rcdm_cfg_pndm_step_scaled(o.get("eps", p), o.get("ld", 32), o.get("lat", p), o.get("hist", p),
                                                         o.get("S", 1), o.get("reps", 2), 5, 8, o.get("W", 8), F,
                                                         o.get("tab", p), o.get("step", p), factor, None)
        sigma = lambda **o: lib.rcdm_cfg_sigma_step_scaled(o.get("eps", p), o.get("ld", 32), o.get("lat", p), o.get("xin", p),
                                                           o.get("hist", p), None, o.get("S", 1), o.get("reps", 2), 5, 8,
                                                           o.get("W", 8), F, o.get("tab", p), o.get("step", p), factor, None)
        common = (dict(eps=None), dict(lat=None), dict(tab=None), dict(step=None), dict(reps=3), dict(reps=0), dict(ld=3),
                  dict(S=0), dict(W=-1))
        for bad in common:
            assert ddim(**bad) == EINVAL and pndm(**bad) == EINVAL and sigma(**bad) == EINVAL, bad
        assert pndm(hist=None) == EINVAL and sigma(hist=None) == EINVAL and sigma(xin=None) == EINVAL
