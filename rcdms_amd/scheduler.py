"""DDIM (and PNDM / Euler / Euler-ancestral / LMS / DPM-Solver / UnCLIP) schedulers with the object protocol
RCDMsPipeline expects from diffusers' DDIMScheduler
(reference: built at stage2_batchtest_rcdms_model.py:247 from configs/testing.yaml:18-21, mutated at
src/pipelines/RCDMs_pipeline.py:84-109, used at :455-456,483,497).

The arithmetic is diffusers==0.24.0's (not vendored by the reference, not installed here): restated from the
DDIM paper eq. (12) with eta = 0 / epsilon prediction — "parity unpinned" by any reference test, pinned by
closed-form known-answer tests (tests/test_scheduler.py).  `step()` is the host-visible (torch) form for
callers that drive the loop themselves; the product's hot loop uses the same coefficients through the fused
rcdm_cfg_ddim_step kernel (rcdms_amd/sampler.py)."""
from dataclasses import dataclass

import torch


class _FrozenDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", timestep_spacing="leading"):
        self._internal_dict = _FrozenDict(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
            beta_schedule=beta_schedule, trained_betas=trained_betas, clip_sample=clip_sample,
            set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, prediction_type=prediction_type,
            timestep_spacing=timestep_spacing)
        if prediction_type != "epsilon" or timestep_spacing != "leading":
            raise NotImplementedError("only epsilon prediction with 'leading' spacing (the reference's configuration)")
        if trained_betas is not None:
            betas = torch.as_tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for {self.__class__}")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    @property
    def config(self):
        return self._internal_dict

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {c.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        ratio = c.num_train_timesteps // num_inference_steps
        ts = (torch.arange(num_inference_steps) * ratio).flip(0).to(torch.int64) + c.steps_offset
        self.timesteps = ts.to(device) if device is not None else ts

    def coefficients(self):
        """[n][4] fp32 = sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev) per inference step (fp64 math)."""
        c = self.config
        ratio = c.num_train_timesteps // self.num_inference_steps
        ac = self.alphas_cumprod.double()
        rows = []
        for t in self.timesteps.tolist():
            prev = t - ratio
            a_t = ac[t]
            a_p = ac[prev] if prev >= 0 else self.final_alpha_cumprod.double()
            rows.append([a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()])
        return torch.tensor(rows, dtype=torch.float32)

    def _alphas(self, t):
        """(a_t, a_prev) of inference timestep t, fp64 tensors."""
        prev = int(t) - self.config.num_train_timesteps // self.num_inference_steps
        ac = self.alphas_cumprod.double()
        return ac[int(t)], (ac[prev] if prev >= 0 else self.final_alpha_cumprod.double())

    def eta_table(self, eta):
        """Stochastic DDIM (eta > 0; DDIM paper eq. (12) / (16), diffusers 0.24.0 `step`) as rows of rcdm_cfg_sigma_step:
        fp32 [n][16] in the SIGMA_ROW layout (module comment further down), computed in fp64.  With
          var = (1 - a_p) / (1 - a_t) (1 - a_t / a_p),  sigma = eta sqrt(var),
          x' = sqrt(a_p) x0 + sqrt(1 - a_p - sigma^2) e + sigma z,   x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t)
        the update is linear in x, e and z:  d = e (px 0, pe 1),  a = sqrt(a_p / a_t),
        b = sqrt(1 - a_p - sigma^2) - sqrt(a_p) sqrt(1 - a_t) / sqrt(a_t),  c = sigma,  cin = cin_next = 1, no history slot.
        clip_sample is not part of the table (DenoiseLoop refuses it)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        eta = float(eta)
        rows = []
        for t in self.timesteps.tolist():
            a_t, a_p = (float(v) for v in self._alphas(t))
            var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
            sig = eta * max(var, 0.0) ** 0.5
            row = [0.0] * 16
            row[0:9] = [0.0, 1.0, (a_p / a_t) ** 0.5,
                        max(1 - a_p - sig * sig, 0.0) ** 0.5 - a_p ** 0.5 * (1 - a_t) ** 0.5 / a_t ** 0.5,
                        0.0, 0.0, 0.0, sig, 1.0]
            row[9:14] = [-1.0, -1.0, -1.0, -1.0, 1.0]
            rows.append(row)
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        """eta > 0: sigma_t = eta sqrt(var_t) of noise is added, `variance_noise` if given, else one randn of model_output's
        shape from `generator` (on the generator's device, as diffusers' randn_tensor) — drawn at every step, the last one
        included, where sigma_t = 0 under set_alpha_to_one."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        c = self.config
        t = int(timestep)
        prev = t - c.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t].to(sample.device)
        a_p = (self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod).to(sample.device)
        x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        if c.clip_sample:
            x0 = x0.clamp(-1.0, 1.0)
        if use_clipped_model_output:   # diffusers 0.24: epsilon is re-derived from the clipped x0 only on request
            model_output = (sample - a_t ** 0.5 * x0) / (1 - a_t) ** 0.5
        if eta == 0.0:
            prev_sample = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * model_output
        else:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or "
                                 "`variance_noise` stays `None`.")
            var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
            sig = eta * var.clamp(min=0) ** 0.5
            prev_sample = a_p ** 0.5 * x0 + (1 - a_p - sig ** 2).clamp(min=0) ** 0.5 * model_output
            if variance_noise is None:
                dev = model_output.device
                gdev = generator.device if generator is not None else dev
                variance_noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=gdev,
                                             generator=generator).to(dev)
            prev_sample = prev_sample + sig * variance_noise
        if not return_dict:
            return (prev_sample,)
        return DDIMSchedulerOutput(prev_sample=prev_sample, pred_original_sample=x0)


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """Guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", §3.4; diffusers
    `rescale_noise_cfg`, restated — "parity unpinned"): the guided prediction rescaled to the per-sample standard deviation of
    the conditional one, mixed back with weight `guidance_rescale`:
        k = phi std(noise_pred_text) / std(noise_cfg) + (1 - phi),   returns k noise_cfg
    std over every axis but the first, unbiased (torch.std).  A deliberate guard: where std(noise_cfg) == 0 (a constant
    prediction) k = 1, where diffusers divides and returns inf / nan.  phi = 0 returns `noise_cfg` itself.  The host-visible
    form of rcdm_cfg_rescale_factor + rcdm_cfg_*_step_scaled (rcdms_amd/sampler.py)."""
    if guidance_rescale == 0.0:
        return noise_cfg
    dims = list(range(1, noise_cfg.dim()))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    zero = std_cfg == 0
    k = guidance_rescale * (std_text / torch.where(zero, torch.ones_like(std_cfg), std_cfg)) + (1 - guidance_rescale)
    return noise_cfg * torch.where(zero, torch.ones_like(k), k)


@dataclass
class PNDMSchedulerOutput:
    prev_sample: torch.Tensor


class PNDMScheduler:
    """PNDM / PLMS (the scheduler type RCDMsPipeline's constructor also accepts, src/pipelines/RCDMs_pipeline.py:72-79;
    the class an SD-1.5 `scheduler/scheduler_config.json` names) with `skip_prk_steps=True`, the only mode Stable
    Diffusion checkpoints configure.

    Arithmetic of diffusers==0.24.0 `PNDMScheduler` (not vendored by the reference, not installed here: restated from
    the published class — "parity unpinned", pinned by closed-form known-answer tests in tests/test_scheduler.py):
      * "leading" spacing: _t = arange(n) * (N // n) + steps_offset; the PLMS list is [_t[:-1], _t[-2], _t[-1]] reversed,
        i.e. n + 1 model evaluations with the second timestep repeated (981, 961, 961, 941, ... for n = 50, offset 1);
      * step_plms: a linear multistep combination of the last <= 4 noise predictions (Adams-Bashforth weights
        1 | 1/2,1/2 (the repeated call, restarting from the saved first sample) | 3/2,-1/2 | 23/12,-16/12,5/12 |
        55/24,-59/24,37/24,-9/24), then
        x' = sqrt(a'/a) x - (a' - a) e / (a sqrt(1 - a') + sqrt(a (1 - a) a'))            (`_get_prev_sample`).
    `step()` is the host-visible torch form (stateful, like diffusers'); `plms_table()` gives the per-call rows the fused
    rcdm_cfg_pndm_step kernel consumes (rcdms_amd/sampler.py)."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon",
                 timestep_spacing="leading", steps_offset=0):
        self._internal_dict = _FrozenDict(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
            beta_schedule=beta_schedule, trained_betas=trained_betas, skip_prk_steps=skip_prk_steps,
            set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
            steps_offset=steps_offset)
        if prediction_type != "epsilon" or timestep_spacing != "leading":
            raise NotImplementedError("only epsilon prediction with 'leading' spacing (the reference's configuration)")
        if not skip_prk_steps:
            raise NotImplementedError("PNDMScheduler: only skip_prk_steps=True (PLMS, what Stable Diffusion checkpoints "
                                      "configure) is built; the Runge-Kutta warm-up steps are not")
        if trained_betas is not None:
            betas = torch.as_tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for {self.__class__}")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)
        self.ets, self.counter, self.cur_sample = [], 0, None

    @property
    def config(self):
        return self._internal_dict

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {c.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        ratio = c.num_train_timesteps // num_inference_steps
        t = torch.arange(num_inference_steps, dtype=torch.int64) * ratio + c.steps_offset
        plms = torch.cat([t[:-1], t[-2:-1], t[-1:]]).flip(0).contiguous()
        self.timesteps = plms.to(device) if device is not None else plms
        self.ets, self.counter, self.cur_sample = [], 0, None

    def _ab(self, timestep, prev_timestep):
        """(sample coefficient, model-output coefficient) of `_get_prev_sample`, in fp64."""
        ac = self.alphas_cumprod.double()
        a_t = ac[timestep]
        a_p = ac[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod.double()
        denom = a_t * (1 - a_p).sqrt() + (a_t * (1 - a_t) * a_p).sqrt()
        return float((a_p / a_t).sqrt()), float(-(a_p - a_t) / denom)

    @staticmethod
    def _weights(n_hist):
        """Multistep weights over (newest, ..., oldest) for n_hist stored predictions."""
        return {1: (1.0,), 2: (1.5, -0.5), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[n_hist]

    def plms_table(self):
        """fp32 [n_calls][12] for rcdm_cfg_pndm_step, one row per model evaluation of the current schedule:
        (a, b, w_now, w1, w2, w3, slot_now (-1: this prediction is not stored), s1, s2, s3, mode, 0) with
        x' = a x_src + b (w_now e + w1 hist[s1] + w2 hist[s2] + w3 hist[s3]); mode 1: also save x as the restart sample
        (first call), mode 2: x_src is that saved sample (second call: the repeated timestep), else x_src = x."""
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        rows, stored = [], []   # stored: ring slots of the kept predictions, oldest first
        for i, t in enumerate(self.timesteps.tolist()):
            if i == 1:
                a, b = self._ab(t + ratio, t)
                rows.append([a, b, 0.5, 0.5, 0.0, 0.0, -1, stored[-1], 0, 0, 2, 0])
                continue
            a, b = self._ab(t, t - ratio)
            slot = i % 4 if i < 2 else (i - 1) % 4
            prev = stored[-3:]
            stored = prev + [slot]
            w = self._weights(len(stored))
            hist = list(reversed(prev))            # newest stored first
            ws = list(w[1:]) + [0.0] * (3 - len(hist))
            ss = hist + [0] * (3 - len(hist))
            rows.append([a, b, w[0], ws[0], ws[1], ws[2], slot, ss[0], ss[1], ss[2], 1 if i == 0 else 0, 0])
        return torch.tensor(rows, dtype=torch.float32)

    def step(self, model_output, timestep, sample, return_dict=True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        t = int(timestep)
        prev_t = t - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_t = t
            t = t + ratio
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])
        a, b = self._ab(t, prev_t)
        prev_sample = a * sample + b * model_output
        self.counter += 1
        return PNDMSchedulerOutput(prev_sample=prev_sample) if return_dict else (prev_sample,)


@dataclass
class UnCLIPSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class UnCLIPScheduler:
    """The stage-1 prior's scheduler (reference: `UnCLIPScheduler.from_pretrained(..., subfolder="scheduler")`,
    stage1_batchtest_rcdms_model.py:101; used at src/pipelines/prior_pipeline.py:293-294,338-344).

    Arithmetic of diffusers==0.24.0 `UnCLIPScheduler` (not vendored, not installed: restated, "parity unpinned"):
    squaredcos_cap_v2 betas, timesteps = round(arange(n) * (N-1)/(n-1))[::-1], and `step` for prediction_type "sample" |
    "epsilon" with variance_type "fixed_small_log".  Defaults are the published Kandinsky-2.2 prior scheduler config
    (clip_sample True, clip_sample_range 10, prediction_type "sample").  `coefficients()` gives the per-step
    (k0, k1, k2) of  prev = k0 x0 + k1 x_t + k2 noise  that the fused rcdm_cfg_unclip_step kernel consumes."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, variance_type="fixed_small_log", clip_sample=True, clip_sample_range=10.0,
                 prediction_type="sample", beta_schedule="squaredcos_cap_v2"):
        if variance_type != "fixed_small_log" or beta_schedule != "squaredcos_cap_v2":
            raise NotImplementedError("UnCLIPScheduler: fixed_small_log / squaredcos_cap_v2 only (the prior's config)")
        if prediction_type not in ("sample", "epsilon"):
            raise NotImplementedError(f"prediction_type {prediction_type}")
        self._internal_dict = _FrozenDict(num_train_timesteps=num_train_timesteps, variance_type=variance_type,
                                          clip_sample=clip_sample, clip_sample_range=clip_sample_range,
                                          prediction_type=prediction_type, beta_schedule=beta_schedule)
        import math
        ab = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2
        n = num_train_timesteps
        betas = [min(1 - ab((i + 1) / n) / ab(i / n), 0.999) for i in range(n)]
        self.betas = torch.tensor(betas, dtype=torch.float64)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.timesteps = torch.arange(n - 1, -1, -1, dtype=torch.int64)
        self.num_inference_steps = None

    @property
    def config(self):
        return self._internal_dict

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        n = self.config.num_train_timesteps
        ratio = (n - 1) / (num_inference_steps - 1)
        import numpy as np
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    def _coef(self, t, prev_t):
        ac = self.alphas_cumprod
        a_t = ac[t]
        a_prev = ac[prev_t] if prev_t >= 0 else torch.tensor(1.0, dtype=torch.float64)
        b_t, b_prev = 1 - a_t, 1 - a_prev
        if prev_t == t - 1:
            beta, alpha = self.betas[t], self.alphas[t]
        else:
            beta = 1 - a_t / a_prev
            alpha = 1 - beta
        k0 = a_prev.sqrt() * beta / b_t
        k1 = alpha.sqrt() * b_prev / b_t
        std = torch.tensor(0.0, dtype=torch.float64)
        if t > 0:
            var = torch.clamp(b_prev / b_t * beta, min=1e-20)
            std = torch.exp(0.5 * torch.log(var))
        return k0, k1, std, a_t, b_t

    def coefficients(self):
        """fp32 [n_steps][3] = (k0, k1, std) for the current timesteps (prev_timestep = the next entry, None at the end:
        prior_pipeline.py:335-338)."""
        ts = self.timesteps.tolist()
        rows = []
        for i, t in enumerate(ts):
            prev = ts[i + 1] if i + 1 < len(ts) else t - 1
            k0, k1, std, _, _ = self._coef(t, prev)
            rows.append([float(k0), float(k1), float(std)])
        return torch.tensor(rows, dtype=torch.float32)

    def step(self, model_output, timestep, sample, prev_timestep=None, generator=None, return_dict=True, noise=None):
        t = int(timestep)
        prev_t = t - 1 if prev_timestep is None else int(prev_timestep)
        k0, k1, std, a_t, b_t = self._coef(t, prev_t)
        if self.config.prediction_type == "epsilon":
            x0 = (sample - b_t.sqrt().to(sample.dtype) * model_output) / a_t.sqrt().to(sample.dtype)
        else:
            x0 = model_output
        if self.config.clip_sample:
            x0 = torch.clamp(x0, -self.config.clip_sample_range, self.config.clip_sample_range)
        prev = k0.to(sample.dtype) * x0 + k1.to(sample.dtype) * sample
        if t > 0:
            if noise is None:
                noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=model_output.device,
                                    generator=generator)
            prev = prev + std.to(sample.dtype) * noise
        return UnCLIPSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)


# ---------------------------------------------------------------------------------------------------------------------
# Sigma-space and DPM-Solver schedulers (the other four types RCDMsPipeline's constructor accepts, RCDMs_pipeline.py:72-79).
#
# Arithmetic of diffusers==0.24.0 EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, LMSDiscreteScheduler and
# DPMSolverMultistepScheduler (not vendored by the reference, not installed here: restated from the published classes —
# "parity unpinned", pinned by closed-form known-answer tests in tests/test_sigma_schedulers.py).  Epsilon prediction only.
# The sigmas are kept in fp64 (diffusers rounds them to fp32; the two agree to ~1e-7 relative).  Every update the pipeline
# drives is linear in the sample, the CFG-combined noise prediction, at most three stored quantities and one noise tensor,
# so each class also lays its schedule out as rows of the fused rcdm_cfg_sigma_step kernel (`sigma_table()`):
#
#   d  = px x + pe e                 (Euler / LMS: d = e;  DPM-Solver++: d = x0 = (x - sigma_t e) / alpha_t)
#   x' = a x + b d + w1 hist[s1] + w2 hist[s2] + w3 hist[s3] + c noise[step];   hist[slot_now] = d
#   model_in = cin_next x'           (scale_model_input of the next step)
#
# Row (16 fp32, computed in fp64): px, pe, a, b, w1, w2, w3, c, cin_next, slot_now, s1, s2, s3, cin, 0, 0 — slot_now -1:
# d is not stored; cin: this step's scale_model_input factor (staged by DenoiseLoop.load for step 0; the kernel does not
# read it).
import inspect

import numpy as np

SIGMA_ROW = 16


@dataclass
class SigmaSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


def _train_betas(c):
    n = c.num_train_timesteps
    if c.trained_betas is not None:
        return torch.as_tensor(c.trained_betas, dtype=torch.float32)
    if c.beta_schedule == "linear":
        return torch.linspace(c.beta_start, c.beta_end, n, dtype=torch.float32)
    if c.beta_schedule == "scaled_linear":
        return torch.linspace(c.beta_start ** 0.5, c.beta_end ** 0.5, n, dtype=torch.float32) ** 2
    raise NotImplementedError(f"beta_schedule {c.beta_schedule!r}: only 'linear', 'scaled_linear' and trained_betas")


class DDPMScheduler:
    """The training-side scheduler (reference: `DDPMScheduler(...)` at train_stage2.py:299-301, `add_noise` at :457): the
    forward-diffusion step only, no `step()`.

    Arithmetic of diffusers==0.24.0 `DDPMScheduler.add_noise` (not vendored by the reference, not installed here: restated —
    "parity unpinned", pinned by closed-form tests in tests/test_objective_host.py):
        noisy = alphas_cumprod[t] ** 0.5 * x0 + (1 - alphas_cumprod[t]) ** 0.5 * noise,   alphas_cumprod fp32.
    The two coefficients of every training timestep are formed ONCE on the host by those expressions (`_table`, fp32 [T][2]);
    `add_noise` (torch) and rcdm_diffuse_assemble (through `noise_table(device)`) both read that table, so the two use the same
    coefficient bits whatever the device's pow rounds to."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None):
        self._internal_dict = _FrozenDict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                          beta_schedule=beta_schedule, trained_betas=trained_betas)
        self.betas = _train_betas(self.config)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        ac = self.alphas_cumprod
        self._table = torch.stack([ac ** 0.5, (1 - ac) ** 0.5], dim=1).contiguous()
        self._tables = {}
        self.init_noise_sigma = 1.0
        self.timesteps = torch.arange(len(self.betas) - 1, -1, -1, dtype=torch.int64)

    @property
    def config(self):
        return self._internal_dict

    def noise_table(self, device=None):
        """fp32 [T][2] = (alphas_cumprod ** 0.5, (1 - alphas_cumprod) ** 0.5), computed on the host; device: where a copy is
        kept (uploaded once per device)."""
        if device is None:
            return self._table
        device = torch.device(device)
        if device not in self._tables:
            self._tables[device] = self._table.to(device)
        return self._tables[device]

    def add_noise(self, original_samples, noise, timesteps):
        """timesteps: int64, one per leading element, each in [0, T)."""
        tab = self.noise_table(original_samples.device).to(original_samples.dtype)
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        t = timesteps.to(original_samples.device)
        sqrt_alpha_prod = tab[t, 0].reshape(shape)
        sqrt_one_minus_alpha_prod = tab[t, 1].reshape(shape)
        return sqrt_alpha_prod * original_samples + sqrt_one_minus_alpha_prod * noise


def _convert_to_karras(in_sigmas, n, sigma_min=None, sigma_max=None):
    """Karras et al. (2022) eq. (5), rho = 7, between the given endpoints (default: the ends of in_sigmas)."""
    lo = float(in_sigmas[-1]) if sigma_min is None else float(sigma_min)
    hi = float(in_sigmas[0]) if sigma_max is None else float(sigma_max)
    rho = 7.0
    ramp = np.linspace(0, 1, n)
    return (hi ** (1 / rho) + ramp * (lo ** (1 / rho) - hi ** (1 / rho))) ** rho


def _sigma_to_t(sigma, log_sigmas):
    """The (fractional) training timestep whose sigma is `sigma`: linear interpolation in log sigma."""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    t = (1 - w) * low_idx + w * high_idx
    return t.reshape(np.shape(sigma))


class _SigmaScheduler:
    """Shared part: config, betas, spacing, step index and the table form.  Subclasses set `_sig` (fp64 numpy, one sigma
    per inference step plus the final one) and `timesteps` (fp32) in set_timesteps, and implement `_rows()`."""
    order = 1
    noise_needed = False
    _timestep_dtype = torch.float32

    def _setup(self, kw):
        self._internal_dict = _FrozenDict(kw)
        c = self.config
        if c.prediction_type != "epsilon":
            raise NotImplementedError(f"{type(self).__name__}: prediction_type {c.prediction_type!r} (epsilon only)")
        if c.timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        self.betas = _train_betas(c)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        ac = self.alphas_cumprod.double().numpy()
        self._train_sig = np.sqrt((1 - ac) / ac)          # sigma of every training timestep, fp64
        self.num_inference_steps = None
        self._step_index = None
        self._sig = np.concatenate([self._train_sig[::-1], [0.0]])
        self.timesteps = torch.from_numpy(np.linspace(0, c.num_train_timesteps - 1, c.num_train_timesteps)[::-1].copy()
                                          ).to(torch.float32)

    @property
    def config(self):
        return self._internal_dict

    @classmethod
    def from_config(cls, config, **kwargs):
        """`cls(**config)` without the keys cls does not take (e.g. DDIM's clip_sample), then `kwargs` on top."""
        params = inspect.signature(cls.__init__).parameters
        kw = {k: v for k, v in dict(config).items() if k in params and k != "self"}
        kw.update(kwargs)
        return cls(**kw)

    @property
    def sigmas(self):
        return torch.from_numpy(self._sig.astype(np.float32))

    @property
    def step_index(self):
        return self._step_index

    def _init_step_index(self, timestep):
        cand = (self.timesteps == float(timestep)).nonzero()
        if len(cand) == 0:
            self._step_index = len(self.timesteps) - 1
        else:
            self._step_index = int(cand[1 if len(cand) > 1 else 0])

    def _spaced(self, n):
        """fp32 inference timesteps of the Euler / LMS family (descending; fractional for 'linspace')."""
        c = self.config
        N = c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            return np.linspace(0, N - 1, n, dtype=np.float32)[::-1].copy()
        if c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (N // n)).round()[::-1].copy().astype(np.float32)
            return ts + np.float32(c.steps_offset)
        return np.arange(N, 0, -N / n).round().copy().astype(np.float32) - np.float32(1)

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {self.config.num_train_timesteps}")
        self.num_inference_steps = int(num_inference_steps)
        ts, sig = self._schedule(self.num_inference_steps)
        self._sig = sig
        t = torch.from_numpy(np.ascontiguousarray(ts)).to(self._timestep_dtype)
        self.timesteps = t.to(device) if device is not None else t
        self._step_index = None
        self._reset_state()

    def _reset_state(self):
        pass

    def _karras(self, sig, n):
        return _convert_to_karras(sig, n)

    def _sigma_space_schedule(self, n, karras):
        ts = self._spaced(n)
        sig = np.interp(ts.astype(np.float64), np.arange(0, len(self._train_sig)), self._train_sig)
        if karras:
            sig = self._karras(sig, n)
            ts = np.array([_sigma_to_t(s, np.log(self._train_sig)) for s in sig]).astype(np.float32)
        return ts, np.concatenate([sig, [0.0]])

    @property
    def init_noise_sigma(self):
        smax = float(self._sig.max())
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return smax
        return (smax ** 2 + 1) ** 0.5

    def scale_model_input(self, sample, timestep=None):
        if self._step_index is None:
            self._init_step_index(timestep)
        return sample / ((self._sig[self._step_index] ** 2 + 1) ** 0.5)

    def _cin(self, i):
        """scale_model_input factor of step i (1 after the last step: the final sample is returned as is)."""
        return 1.0 / (self._sig[i] ** 2 + 1) ** 0.5 if i < len(self.timesteps) else 1.0

    def sigma_table(self):
        """fp32 [num_steps][16] rows of rcdm_cfg_sigma_step for the current schedule (layout: module comment above)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        rows = []
        for i, r in enumerate(self._rows()):
            row = [0.0] * SIGMA_ROW
            px, pe, a, b, w, c, slot, ss = r
            w, ss = list(w) + [0.0] * (3 - len(w)), list(ss) + [0] * (3 - len(ss))
            row[0:9] = [px, pe, a, b, w[0], w[1], w[2], c, self._cin(i + 1)]
            row[9:14] = [slot, ss[0], ss[1], ss[2], self._cin(i)]
            rows.append(row)
        return torch.tensor(np.array(rows, dtype=np.float64), dtype=torch.float32)


class EulerDiscreteScheduler(_SigmaScheduler):
    """Euler (Karras et al. 2022, Algorithm 2) in sigma space, diffusers 0.24.0 `EulerDiscreteScheduler` with s_churn = 0
    (the only value the pipeline passes: prepare_extra_step_kwargs forwards just `generator`):
      x' = x + (sigma_next - sigma) (x - x0) / sigma,   x0 = x - sigma e;   sigmas interpolated at the (float) timesteps,
    0 appended; optional Karras sigmas.  interpolation_type 'log_linear', timestep_type 'continuous' and s_churn > 0 raise."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False,
                 sigma_min=None, sigma_max=None, timestep_spacing="linspace", timestep_type="discrete", steps_offset=0):
        self._setup(dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type,
                         interpolation_type=interpolation_type, use_karras_sigmas=use_karras_sigmas, sigma_min=sigma_min,
                         sigma_max=sigma_max, timestep_spacing=timestep_spacing, timestep_type=timestep_type,
                         steps_offset=steps_offset))
        if interpolation_type != "linear" or timestep_type != "discrete":
            raise NotImplementedError("EulerDiscreteScheduler: interpolation_type 'linear' / timestep_type 'discrete' only")
        self.use_karras_sigmas = use_karras_sigmas

    def _karras(self, sig, n):
        return _convert_to_karras(sig, n, self.config.sigma_min, self.config.sigma_max)

    def _schedule(self, n):
        return self._sigma_space_schedule(n, self.config.use_karras_sigmas)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
             generator=None, return_dict=True):
        if s_churn != 0.0:
            raise NotImplementedError("EulerDiscreteScheduler: s_churn > 0 (stochastic Euler) is not built")
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma, nxt = self._sig[self._step_index], self._sig[self._step_index + 1]
        x0 = sample - sigma * model_output
        prev = sample + (sample - x0) / sigma * (nxt - sigma)
        self._step_index += 1
        return SigmaSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def _rows(self):
        s = self._sig
        return [(0.0, 1.0, 1.0, s[i + 1] - s[i], (), 0.0, -1, ()) for i in range(len(self.timesteps))]


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """Ancestral Euler, diffusers 0.24.0 `EulerAncestralDiscreteScheduler`: from sigma to sigma_next via
      sigma_up = sqrt(sigma_next^2 (sigma^2 - sigma_next^2) / sigma^2),  sigma_down = sqrt(sigma_next^2 - sigma_up^2),
      x' = x + (sigma_down - sigma) e + sigma_up n,   n ~ N(0, I): one fresh randn of the sample's shape per step, drawn
    from the caller's generator (also at the last step, where sigma_up = 0).  No Karras option in this version."""
    noise_needed = True

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0):
        self._setup(dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type,
                         timestep_spacing=timestep_spacing, steps_offset=steps_offset))

    def _schedule(self, n):
        return self._sigma_space_schedule(n, False)

    def _up_down(self, i):
        s, nxt = self._sig[i], self._sig[i + 1]
        up = (nxt ** 2 * (s ** 2 - nxt ** 2) / s ** 2) ** 0.5
        return up, max(nxt ** 2 - up ** 2, 0.0) ** 0.5

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """noise: the step's N(0, I) draw, if the caller has it; else randn of model_output's shape from `generator`
        (on the generator's device when that is the CPU, as diffusers' randn_tensor)."""
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self._sig[self._step_index]
        up, down = self._up_down(self._step_index)
        x0 = sample - sigma * model_output
        prev = sample + (sample - x0) / sigma * (down - sigma)
        if noise is None:
            dev = model_output.device
            gdev = generator.device if generator is not None else dev
            noise = torch.randn(model_output.shape, dtype=model_output.dtype, device=gdev, generator=generator).to(dev)
        prev = prev + noise * up
        self._step_index += 1
        return SigmaSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def _rows(self):
        rows = []
        for i in range(len(self.timesteps)):
            up, down = self._up_down(i)
            rows.append((0.0, 1.0, 1.0, down - self._sig[i], (), up, -1, ()))
        return rows


class LMSDiscreteScheduler(_SigmaScheduler):
    """Linear multistep in sigma space, diffusers 0.24.0 `LMSDiscreteScheduler` with step(order=4):
      x' = x + sum_k c_k d_{i-k},   d = (x - x0) / sigma = e,   c_k = integral over [sigma_i, sigma_{i+1}] of the Lagrange
    basis polynomial of node sigma_{i-k} on the nodes sigma_i .. sigma_{i-m+1}, m = min(i + 1, order).  diffusers integrates
    with scipy.integrate.quad (epsrel 1e-4); here the polynomial is integrated exactly (numpy.polynomial)."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, use_karras_sigmas=False, prediction_type="epsilon", timestep_spacing="linspace",
                 steps_offset=0):
        self._setup(dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, use_karras_sigmas=use_karras_sigmas,
                         prediction_type=prediction_type, timestep_spacing=timestep_spacing, steps_offset=steps_offset))
        self.use_karras_sigmas = use_karras_sigmas
        self.derivatives = []
        self.set_timesteps(num_train_timesteps)

    def _schedule(self, n):
        return self._sigma_space_schedule(n, self.config.use_karras_sigmas)

    def _reset_state(self):
        self.derivatives = []

    def get_lms_coefficient(self, order, t, current_order):
        """Exact integral of the Lagrange basis polynomial of node sigma[t - current_order] from sigma[t] to sigma[t + 1]."""
        s = self._sig
        poly = np.polynomial.Polynomial([1.0])
        for k in range(order):
            if k != current_order:
                poly = poly * np.polynomial.Polynomial([-s[t - k], 1.0]) / (s[t - current_order] - s[t - k])
        anti = poly.integ()
        return float(anti(s[t + 1]) - anti(s[t]))

    def _coeffs(self, i, order=4):
        m = min(i + 1, order)
        return [self.get_lms_coefficient(m, i, k) for k in range(m)]

    def step(self, model_output, timestep, sample, order=4, return_dict=True):
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self._sig[self._step_index]
        x0 = sample - sigma * model_output
        self.derivatives.append((sample - x0) / sigma)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        coeffs = self._coeffs(self._step_index, order)
        prev = sample + sum(c * d for c, d in zip(coeffs, reversed(self.derivatives)))
        self._step_index += 1
        return SigmaSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def _rows(self):
        n = len(self.timesteps)
        rows = []
        for i in range(n):
            c = self._coeffs(i)
            slot = i % 3 if i + 1 < n else -1      # the derivative is read by the next three steps
            ss = [(i - k) % 3 for k in range(1, len(c))]
            rows.append((0.0, 1.0, 1.0, c[0], c[1:], 0.0, slot, ss))
        return rows


class DPMSolverMultistepScheduler(_SigmaScheduler):
    """DPM-Solver / DPM-Solver++ multistep (Lu et al. 2022), diffusers 0.24.0 `DPMSolverMultistepScheduler`:
    algorithm_type 'dpmsolver++' (model output converted to x0 = (x - sigma_t e) / alpha_t) and 'dpmsolver' (e itself),
    solver_type 'midpoint' / 'heun', solver_order 1-3, lower_order_final / euler_at_final (below 15 steps the last two
    steps drop to orders 1 and 2), integer timesteps linspace(0, last_t - 1, n + 1).round()[::-1][:-1] ('linspace'), and
    Karras sigmas (timesteps then the rounded _sigma_to_t of each).  alpha_t = 1 / sqrt(sigma^2 + 1), sigma_t = sigma
    alpha_t, lambda = log(alpha_t / sigma_t).

    Final sigma: 0.24.0 appends the sigma of training timestep 0 (Karras: the last Karras sigma, which is the same value),
    not 0 — later diffusers releases made that configurable (final_sigmas_type).  This class follows 0.24.0, so the result
    keeps the small noise level sigma(t=0).  Where a step has h = 0 (Karras: the appended sigma equals the last one) the
    h -> 0 limit is used, the sample unchanged — what 0.24.0 computes for first and second order midpoint steps (its
    heun and third-order forms divide 0 by 0 there).
    Refused: sde-dpmsolver / sde-dpmsolver++, thresholding, prediction types other than epsilon, use_lu_lambdas."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                 solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False,
                 use_lu_lambdas=False, lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace",
                 steps_offset=0):
        if algorithm_type == "deis":            # diffusers maps these onto the nearest built form
            algorithm_type = "dpmsolver++"
        if solver_type in ("logrho", "bh1", "bh2"):
            solver_type = "midpoint"
        self._setup(dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                         beta_schedule=beta_schedule, trained_betas=trained_betas, solver_order=solver_order,
                         prediction_type=prediction_type, thresholding=thresholding,
                         dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
                         algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                         euler_at_final=euler_at_final, use_karras_sigmas=use_karras_sigmas, use_lu_lambdas=use_lu_lambdas,
                         lambda_min_clipped=lambda_min_clipped, variance_type=variance_type,
                         timestep_spacing=timestep_spacing, steps_offset=steps_offset))
        if algorithm_type in ("sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"DPMSolverMultistepScheduler: {algorithm_type} (SDE variants) is not built")
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{algorithm_type} does is not implemented for {self.__class__}")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{solver_type} does is not implemented for {self.__class__}")
        if thresholding:
            raise NotImplementedError("DPMSolverMultistepScheduler: thresholding is not built")
        if use_lu_lambdas:
            raise NotImplementedError("DPMSolverMultistepScheduler: use_lu_lambdas is not built")
        if variance_type is not None:
            raise NotImplementedError("DPMSolverMultistepScheduler: learned variance is not built")
        if solver_order not in (1, 2, 3):
            raise NotImplementedError(f"DPMSolverMultistepScheduler: solver_order {solver_order} (1-3)")
        self.use_karras_sigmas = use_karras_sigmas
        self._reset_state()

    init_noise_sigma = 1.0    # a plain attribute here, not the sigma-space property
    _timestep_dtype = torch.int64

    def _reset_state(self):
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _cin(self, i):
        return 1.0

    def _schedule(self, n):
        c = self.config
        N = c.num_train_timesteps
        ac = self.alphas_cumprod.double()
        lam = torch.log(ac.sqrt()) - torch.log((1 - ac).sqrt())
        clipped = int(torch.searchsorted(torch.flip(lam, [0]), torch.tensor(float(c.lambda_min_clipped), dtype=lam.dtype)))
        last = N - clipped
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (last // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        else:
            ts = np.arange(last, 0, -N / n).round().copy().astype(np.int64) - 1
        sig = self._train_sig
        if c.use_karras_sigmas:
            ks = _convert_to_karras(sig[::-1].copy(), n)
            ts = np.array([_sigma_to_t(s, np.log(sig)) for s in ks]).round().astype(np.int64)
            sig_out = np.concatenate([ks, ks[-1:]])
        else:
            sig_out = np.concatenate([np.interp(ts.astype(np.float64), np.arange(0, len(sig)), sig), [sig[0]]])
        return ts, sig_out

    def set_timesteps(self, num_inference_steps=None, device=None):
        super().set_timesteps(num_inference_steps, device)
        self.num_inference_steps = len(self.timesteps)

    @staticmethod
    def _alpha_sigma(sigma):
        alpha = 1.0 / (sigma ** 2 + 1) ** 0.5
        return alpha, sigma * alpha

    def _lam(self, i):
        a, s = self._alpha_sigma(self._sig[i])
        return np.log(a) - np.log(s)

    def _order_at(self, i):
        """The order 0.24.0's step() uses at step i (lower_order_nums = min(i, solver_order) there)."""
        c, n = self.config, len(self.timesteps)
        final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15))
        second = i == n - 2 and c.lower_order_final and n < 15
        if c.solver_order == 1 or i < 1 or final:
            return 1
        if c.solver_order == 2 or i < 2 or second:
            return 2
        return 3

    def _convert(self, i):
        """(px, pe) of the converted model output at step i."""
        if self.config.algorithm_type == "dpmsolver":
            return 0.0, 1.0
        a, s = self._alpha_sigma(self._sig[i])
        return 1.0 / a, -s / a

    def _update(self, i, order, sample, ms):
        """The solver update of step i from `sample` and the converted model outputs ms (newest last), restated from
        dpm_solver_first_order_update / multistep_dpm_solver_second_order_update / ..._third_order_update.  Linear in
        sample and ms, so sigma_table() evaluates it on unit vectors."""
        c = self.config
        pp = c.algorithm_type == "dpmsolver++"
        a_t, s_t = self._alpha_sigma(self._sig[i + 1])
        a_0, s_0 = self._alpha_sigma(self._sig[i])
        h = self._lam(i + 1) - self._lam(i)
        em = np.expm1(-h) if pp else np.expm1(h)                   # e^{-h} - 1 (++) or e^{h} - 1
        base = (s_t / s_0) * sample if pp else (a_t / a_0) * sample
        k0 = -a_t * em if pp else -s_t * em
        m0 = ms[-1]
        if order == 1:
            return base + k0 * m0
        if h == 0:      # the h -> 0 limit (Karras' repeated last sigma): sample unchanged
            return base + k0 * m0
        g1 = em / h + 1.0 if pp else em / h - 1.0                  # (e^{-h} - 1) / h + 1  |  (e^{h} - 1) / h - 1
        h0 = self._lam(i) - self._lam(i - 1)
        inv_r0 = h / h0
        if order == 2:
            D1 = inv_r0 * (m0 - ms[-2])
            if c.solver_type == "midpoint":
                return base + k0 * m0 + 0.5 * k0 * D1
            return base + k0 * m0 + (a_t * g1 if pp else -s_t * g1) * D1
        h1 = self._lam(i - 1) - self._lam(i - 2)
        r0, r1 = h0 / h, h1 / h
        D1_0, D1_1 = inv_r0 * (m0 - ms[-2]), (1.0 / r1) * (ms[-2] - ms[-3])
        D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
        D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
        if pp:
            g2 = (em + h) / h ** 2 - 0.5
            return base + k0 * m0 + a_t * g1 * D1 - a_t * g2 * D2
        g2 = (em - h) / h ** 2 - 0.5
        return base + k0 * m0 - s_t * g1 * D1 - s_t * g2 * D2

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        px, pe = self._convert(i)
        m = px * sample + pe * model_output
        self.model_outputs = self.model_outputs[1:] + [m]
        order = self._order_at(i)
        prev = self._update(i, order, sample, [x for x in self.model_outputs if x is not None][-order:])
        self.lower_order_nums = min(self.lower_order_nums + 1, self.config.solver_order)
        self._step_index += 1
        return SigmaSchedulerOutput(prev_sample=prev) if return_dict else (prev,)

    def _rows(self):
        n = len(self.timesteps)
        keep = self.config.solver_order - 1          # how many past outputs a later step may read
        rows = []
        for i in range(n):
            order = self._order_at(i)
            e = np.eye(4)
            v = self._update(i, order, e[0], [e[3], e[2], e[1]][-order:])   # sample, m_{i-2}, m_{i-1}, m_i
            px, pe = self._convert(i)
            w = [v[2], v[3]][:order - 1]
            slot = i % 3 if keep > 0 and i + 1 < n else -1
            ss = [(i - k) % 3 for k in range(1, order)]
            rows.append((px, pe, v[0], v[1], w, 0.0, slot, ss))
        return rows
