"""CPU: known-answer tests for the restated diffusers 0.24.0 Euler / Euler-ancestral / LMS / DPM-Solver schedulers
(rcdms_amd/scheduler.py) — "parity unpinned" by the reference (it holds no tests), pinned here by closed forms:
timestep / sigma tables, exact ODE solutions for point-mass data, convergence orders on Gaussian data — and the
sigma_table() rows that the fused rcdm_cfg_sigma_step kernel consumes, replayed in fp64 against step()."""
import math

import numpy as np
import pytest
import torch

from rcdms_amd.scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                 EulerDiscreteScheduler, LMSDiscreteScheduler)

KW = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ALL = [EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, LMSDiscreteScheduler, DPMSolverMultistepScheduler]


def train_sigmas(beta_schedule="scaled_linear", b0=0.00085, b1=0.012):
    if beta_schedule == "linear":
        betas = torch.linspace(b0, b1, 1000, dtype=torch.float32)
    else:
        betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1 - betas, 0).double().numpy()
    return np.sqrt((1 - ac) / ac)


# ---- timestep / sigma tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, LMSDiscreteScheduler])
def test_sigma_space_tables(cls):
    sig = train_sigmas()
    s = cls(**KW)                                          # 'linspace': fractional timesteps from 999 to 0
    s.set_timesteps(10)
    t = np.linspace(0, 999, 10)[::-1]
    assert np.allclose(s.timesteps.numpy(), t, atol=1e-4) and s.timesteps.dtype == torch.float32
    i0 = np.floor(t[1]).astype(int)
    want = sig[i0] + (t[1] - i0) * (sig[i0 + 1] - sig[i0])          # linear interpolation at t = 888
    assert abs(s.sigmas[1].item() - want) < 1e-5 * want
    assert s.sigmas[-1].item() == 0.0 and len(s.sigmas) == 11
    assert abs(s.init_noise_sigma - sig[999]) < 1e-9                 # sigma_max for 'linspace'
    assert 14.0 < s.init_noise_sigma < 15.0

    s = cls(timestep_spacing="leading", steps_offset=1, **KW)
    s.set_timesteps(20)
    assert s.timesteps.tolist() == [951.0 - 50 * i for i in range(20)]
    assert abs(s.sigmas[0].item() - sig[951]) < 1e-5 * sig[951]
    assert abs(s.init_noise_sigma - math.sqrt(sig[951] ** 2 + 1)) < 1e-9    # sqrt(sigma_max^2 + 1) otherwise

    s = cls(timestep_spacing="trailing", **KW)
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999.0, 749.0, 499.0, 249.0]
    assert abs(s.init_noise_sigma - sig[999]) < 1e-9
    x = torch.full((3,), 2.0, dtype=torch.float64)
    assert abs(s.scale_model_input(x, 999.0)[0].item() - 2.0 / math.sqrt(sig[999] ** 2 + 1)) < 1e-12


def test_karras_sigmas():
    sig = train_sigmas()
    for cls in (EulerDiscreteScheduler, LMSDiscreteScheduler):
        s = cls(use_karras_sigmas=True, **KW)
        s.set_timesteps(12)
        k = s._sig[:-1]
        assert abs(k[0] - sig[999]) < 1e-9 and abs(k[-1] - sig[0]) < 1e-9     # endpoints sigma_max, sigma_min
        rho = 7.0
        ramp = np.linspace(sig[999] ** (1 / rho), sig[0] ** (1 / rho), 12) ** rho
        assert np.allclose(k, ramp, rtol=1e-12)
        # _sigma_to_t: the timestep whose interpolated log-sigma is the Karras sigma
        ts = s.timesteps.double().numpy()
        back = np.exp(np.interp(ts, np.arange(1000), np.log(sig)))
        assert np.allclose(back, k, rtol=1e-5)
        assert ts[0] == pytest.approx(999.0) and ts[-1] == pytest.approx(0.0, abs=1e-4)
    e = EulerDiscreteScheduler(use_karras_sigmas=True, sigma_min=0.1, sigma_max=10.0, **KW)
    e.set_timesteps(5)
    assert e._sig[0] == pytest.approx(10.0) and e._sig[4] == pytest.approx(0.1)
    d = DPMSolverMultistepScheduler(use_karras_sigmas=True, **KW)
    d.set_timesteps(12)
    assert d.timesteps.dtype == torch.int64 and d.timesteps[0].item() == 999 and d.timesteps[-1].item() == 0
    assert d._sig[-1] == d._sig[-2] == pytest.approx(sig[0])                  # 0.24.0: the last Karras sigma repeated


def test_dpm_solver_timesteps():
    sig = train_sigmas()
    s = DPMSolverMultistepScheduler(**KW)
    s.set_timesteps(20)
    want = np.linspace(0, 999, 21).round()[::-1][:-1].astype(np.int64)
    assert s.timesteps.tolist() == want.tolist() and s.timesteps[0].item() == 999 and s.timesteps[-1].item() == 50
    assert s.init_noise_sigma == 1.0
    assert s._sig[-1] == pytest.approx(sig[0]) and s._sig[0] == pytest.approx(sig[999])   # final sigma: sigma(t = 0)
    s = DPMSolverMultistepScheduler(timestep_spacing="leading", steps_offset=1, **KW)
    s.set_timesteps(20)
    assert s.timesteps.tolist() == [47 * i + 1 for i in range(20, 0, -1)]          # 1000 // 21 = 47
    s = DPMSolverMultistepScheduler(timestep_spacing="trailing", **KW)
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 749, 499, 249]


def test_from_config_of_the_reference_ddim_config():
    """The usual idiom `Cls.from_config(ddim.config)` on the reference's DDIM (configs/testing.yaml: linear 0.00085 ..
    0.012, steps_offset forced to 1 by the pipeline): DDIM-only keys are dropped, leading spacing and the offset come along."""
    ddim = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    for cls in ALL:
        s = cls.from_config(ddim.config)
        assert s.config.timestep_spacing == "leading" and s.config.steps_offset == 1
        assert s.config.beta_schedule == "linear" and "clip_sample" not in s.config
        assert torch.equal(s.alphas_cumprod, ddim.alphas_cumprod)
    e = EulerDiscreteScheduler.from_config(ddim.config)
    e.set_timesteps(50)
    assert e.timesteps[:2].tolist() == [981.0, 961.0] and e.timesteps[-1].item() == 1.0
    d = DPMSolverMultistepScheduler.from_config(ddim.config, use_karras_sigmas=True)
    assert d.config.use_karras_sigmas and d.config.algorithm_type == "dpmsolver++"


# ---- closed-form solutions --------------------------------------------------------------------------------------------
def _drive(s, n, eps_fn, x_start=1.3):
    """The reference loop on a scalar 'image' in fp64: scale_model_input -> eps_fn(sigma-space x, sigma) -> step."""
    s.set_timesteps(n)
    x = torch.full((4,), x_start, dtype=torch.float64) * s.init_noise_sigma
    vp = isinstance(s, DPMSolverMultistepScheduler)
    g = torch.Generator().manual_seed(0)
    for i, t in enumerate(s.timesteps):
        sig = float(s._sig[i])
        xin = s.scale_model_input(x, t)
        xs = xin * math.sqrt(sig ** 2 + 1)                   # the model sees the VP sample; its sigma-space form
        e = eps_fn(xs, sig)
        kw = {"noise": torch.zeros(4, dtype=torch.float64)} if isinstance(s, EulerAncestralDiscreteScheduler) else {}
        x = s.step(e, t, x, **kw).prev_sample
    s0, s_end = float(s._sig[0]), float(s._sig[-1])
    xs0 = x_start * s.init_noise_sigma * (math.sqrt(s0 ** 2 + 1) if vp else 1.0)
    return x, xs0, s0, s_end, vp


DETERMINISTIC = [
    (EulerDiscreteScheduler, {}), (EulerDiscreteScheduler, dict(use_karras_sigmas=True)),
    (EulerDiscreteScheduler, dict(timestep_spacing="leading", steps_offset=1)),
    (LMSDiscreteScheduler, {}), (LMSDiscreteScheduler, dict(use_karras_sigmas=True)),
    (LMSDiscreteScheduler, dict(timestep_spacing="trailing")),
    (DPMSolverMultistepScheduler, dict(solver_order=1)), (DPMSolverMultistepScheduler, {}),
    (DPMSolverMultistepScheduler, dict(solver_order=3)), (DPMSolverMultistepScheduler, dict(solver_type="heun")),
    (DPMSolverMultistepScheduler, dict(algorithm_type="dpmsolver")),
    (DPMSolverMultistepScheduler, dict(use_karras_sigmas=True, solver_order=3, timestep_spacing="leading", steps_offset=1)),
]


@pytest.mark.parametrize("n", [3, 7, 25])
@pytest.mark.parametrize("cls,extra", DETERMINISTIC)
def test_point_mass_data_lands_on_the_ode_solution(cls, extra, n):
    """Data = a point mass at x0*: the exact noise prediction is (x - x0*) / sigma and the probability-flow ODE solution is
    x(sigma) = x0* + (x_T - x0*) sigma / sigma_T.  Every scheduler integrates it exactly, for any step count."""
    x0 = 0.3
    x, xs0, s0, s_end, vp = _drive(cls(**KW, **extra), n, lambda xs, sig: (xs - x0) / sig)
    want = x0 + (xs0 - x0) * s_end / s0
    if vp:
        want /= math.sqrt(s_end ** 2 + 1)                   # DPM-Solver's sample is the VP one, at sigma(t = 0)
    assert (x - want).abs().max().item() < 1e-12 * max(1.0, abs(xs0)), (x[0].item(), want)


def _gauss_error(cls, extra, n, s2=0.25):
    """Data ~ N(0, s2): optimal eps = sigma x / (s2 + sigma^2); ODE solution x(sigma) = x_T sqrt((s2 + sigma^2) / (s2 + sigma_T^2))."""
    x, xs0, s0, s_end, vp = _drive(cls(**KW, **extra), n, lambda xs, sig: sig * xs / (s2 + sig ** 2))
    want = xs0 * math.sqrt((s2 + s_end ** 2) / (s2 + s0 ** 2))
    if vp:
        want /= math.sqrt(s_end ** 2 + 1)
    return abs(x[0].item() - want)


@pytest.mark.parametrize("cls,extra,ns,lo,hi", [
    (EulerDiscreteScheduler, {}, (20, 40, 80), 1.7, 2.3),                       # first order: error halves
    (DPMSolverMultistepScheduler, dict(solver_order=1), (40, 80, 160), 1.7, 2.3),
    (DPMSolverMultistepScheduler, dict(use_karras_sigmas=True), (20, 40, 80), 4.0, 5.0),   # DPM++ 2M Karras: second order
    (DPMSolverMultistepScheduler, dict(use_karras_sigmas=True, solver_type="heun"), (20, 40, 80), 4.0, 5.0),
    (LMSDiscreteScheduler, dict(use_karras_sigmas=True), (20, 40, 80), 8.0, 20.0),  # order 4 (lower-order start)
    (LMSDiscreteScheduler, {}, (40, 80, 160), 6.0, 20.0),
])
def test_gaussian_data_convergence_order(cls, extra, ns, lo, hi):
    """The error against the closed-form ODE solution falls by ~2x per doubling of the steps for first-order schedulers
    and by >= 4x for DPM-Solver++ 2M and LMS: a wrong coefficient would show up as a lower order."""
    errs = [_gauss_error(cls, extra, n) for n in ns]
    for a, b in zip(errs, errs[1:]):
        assert lo <= a / b <= hi, errs


# ---- LMS coefficients -------------------------------------------------------------------------------------------------
def test_lms_coefficients_match_quadrature():
    """Exact integration of the Lagrange basis polynomials against the adaptive quadrature diffusers uses."""
    integrate = pytest.importorskip("scipy.integrate")
    s = LMSDiscreteScheduler(**KW)
    s.set_timesteps(12)
    sig = s._sig
    for t in (0, 1, 2, 5, 11):
        order = min(t + 1, 4)
        for cur in range(order):
            def basis(tau):
                p = 1.0
                for k in range(order):
                    if k != cur:
                        p *= (tau - sig[t - k]) / (sig[t - cur] - sig[t - k])
                return p
            q = integrate.quad(basis, sig[t], sig[t + 1], epsrel=1e-10)[0]
            assert abs(s.get_lms_coefficient(order, t, cur) - q) < 1e-6 * max(1.0, abs(q))
    assert s.get_lms_coefficient(1, 0, 0) == pytest.approx(sig[1] - sig[0])      # order 1: Euler


# ---- sigma_table() rows against step() --------------------------------------------------------------------------------
TABLE_CASES = [
    (EulerDiscreteScheduler, {}, 9), (EulerDiscreteScheduler, dict(use_karras_sigmas=True), 9),
    (EulerAncestralDiscreteScheduler, {}, 9), (EulerAncestralDiscreteScheduler, dict(timestep_spacing="leading", steps_offset=1), 6),
    (LMSDiscreteScheduler, {}, 9), (LMSDiscreteScheduler, dict(use_karras_sigmas=True, timestep_spacing="trailing"), 7),
    (DPMSolverMultistepScheduler, dict(solver_order=1), 8), (DPMSolverMultistepScheduler, {}, 8),
    (DPMSolverMultistepScheduler, {}, 20), (DPMSolverMultistepScheduler, dict(solver_type="heun"), 8),
    (DPMSolverMultistepScheduler, dict(solver_order=3), 8), (DPMSolverMultistepScheduler, dict(solver_order=3), 20),
    (DPMSolverMultistepScheduler, dict(algorithm_type="dpmsolver", solver_type="heun"), 8),
    (DPMSolverMultistepScheduler, dict(algorithm_type="dpmsolver", solver_order=3), 16),
    (DPMSolverMultistepScheduler, dict(use_karras_sigmas=True), 20),
    (DPMSolverMultistepScheduler, dict(euler_at_final=True, lower_order_final=False, timestep_spacing="leading",
                                       steps_offset=1), 8),
]


def apply_row(row, x, e, hist, noise):
    """What rcdm_cfg_sigma_step does with one row (rcdm.h), in fp64."""
    r = row.tolist()
    px, pe, a, b, w1, w2, w3, c, cin = r[:9]
    slot, ss = int(r[9]), [int(v) for v in r[10:13]]
    d = px * x + pe * e
    y = a * x + b * d
    for w, sl in zip((w1, w2, w3), ss):
        if w != 0.0:
            y = y + w * hist[sl]
    if c != 0.0:
        y = y + c * noise
    if 0 <= slot < 3:
        hist[slot] = d
    return y, cin * y


@pytest.mark.parametrize("cls,extra,n", TABLE_CASES)
def test_sigma_table_rows_reproduce_step(cls, extra, n):
    s = cls(**KW, **extra)
    s.set_timesteps(n)
    tab = s.sigma_table().double()
    T = len(s.timesteps)
    assert tab.shape == (T, 16) and torch.isfinite(tab).all()
    assert s.noise_needed == bool((tab[:, 7] != 0).any())
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64) * s.init_noise_sigma
    y = x.clone()
    assert torch.allclose(s.scale_model_input(x, s.timesteps[0]), tab[0, 13] * x, rtol=1e-6)
    hist = [torch.full_like(x, float("nan")) for _ in range(3)]          # never read before it is written
    for i, t in enumerate(s.timesteps):
        e = torch.randn(x.shape, generator=g, dtype=torch.float64)
        nz = torch.randn(x.shape, generator=g, dtype=torch.float64)
        kw = {"noise": nz} if cls is EulerAncestralDiscreteScheduler else {}
        x = s.step(e, t, x, **kw).prev_sample
        y, y_in = apply_row(tab[i], y, e, hist, nz)
        scale = max(1.0, x.abs().max().item())
        assert (x - y).abs().max().item() < 2e-6 * scale, i            # fp32 coefficients
        want_in = s.scale_model_input(x, s.timesteps[i + 1]) if i + 1 < T else x
        assert (want_in - y_in).abs().max().item() < 2e-6 * scale, i


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_unsupported_configurations_raise():
    for cls in ALL:
        with pytest.raises(NotImplementedError):
            cls(prediction_type="v_prediction")
        with pytest.raises(NotImplementedError):
            cls(prediction_type="sample")
        with pytest.raises(NotImplementedError):
            cls(beta_schedule="squaredcos_cap_v2")
    for kw in (dict(algorithm_type="sde-dpmsolver++"), dict(algorithm_type="sde-dpmsolver"), dict(thresholding=True),
               dict(use_lu_lambdas=True), dict(solver_order=4)):
        with pytest.raises(NotImplementedError):
            DPMSolverMultistepScheduler(**kw)
    with pytest.raises(NotImplementedError):
        EulerDiscreteScheduler(interpolation_type="log_linear")
    e = EulerDiscreteScheduler(**KW)
    e.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="s_churn"):
        e.step(torch.zeros(2), e.timesteps[0], torch.zeros(2), s_churn=1.0)


def test_denoise_loop_dispatch_host():
    """DenoiseLoop (host logic only: the launch plan is built on first load()) takes the table path for the new classes,
    with fp32 timesteps, and still refuses a diffusers-like object that has alphas_cumprod but no sigma_table()."""
    from rcdms_amd.sampler import DenoiseLoop

    class FakeUNet:
        device = torch.device("cpu")

    for cls, n, multistep, noisy in ((EulerDiscreteScheduler, 10, False, False),
                                     (EulerAncestralDiscreteScheduler, 10, False, True),
                                     (LMSDiscreteScheduler, 10, True, False), (DPMSolverMultistepScheduler, 10, True, False)):
        lp = DenoiseLoop(FakeUNet(), 1, 5, 8, 8, 13, 2.0, cls(**KW), n)
        assert lp.sigma and not lp.pndm and lp.T == n and tuple(lp.coef.shape) == (n, 16)
        assert lp.timesteps.dtype == torch.float32 and lp.multistep is multistep and (lp.noise is not None) is noisy
        assert lp.x_in is lp.model_in and tuple(lp.hist.shape) == (3, 4 * 5 * 8 * 8)
    lp = DenoiseLoop(FakeUNet(), 1, 5, 8, 8, 13, 2.0, DPMSolverMultistepScheduler(solver_order=1, **KW), 10)
    assert not lp.multistep
    lp = DenoiseLoop(FakeUNet(), 1, 5, 8, 8, 13, 2.0, DDIMScheduler(clip_sample=False, steps_offset=1, **KW), 10)
    assert not lp.sigma and lp.timesteps.dtype == torch.int64 and lp.x_in is lp.lat

    real = EulerDiscreteScheduler(**KW)

    class DiffusersLikeEuler:          # what `from diffusers import EulerDiscreteScheduler` would hand the pipeline
        config = real.config
        alphas_cumprod = real.alphas_cumprod
        init_noise_sigma = 14.6

        def set_timesteps(self, n, device=None):
            real.set_timesteps(n)
            self.timesteps = real.timesteps

    with pytest.raises(NotImplementedError, match="not a DDIM schedule"):
        DenoiseLoop(FakeUNet(), 1, 5, 8, 8, 13, 2.0, DiffusersLikeEuler(), 10)
