"""The stage-2 denoising loop on MI355X: T replays of ONE captured hipGraph per story batch.

Reference: the `for t in timesteps` body of RCDMsPipeline.__call__ (src/pipelines/RCDMs_pipeline.py:480-503):
cat([latents]*2) -> cat([x, mask, masked_latents], 1) -> unet -> CFG combine -> scheduler.step.  Here one graph
holds [this step's time_emb_proj rows from a per-schedule table | assemble the 9-channel rows | ~10^3 UNet kernels |
fused CFG + scheduler update | step++]; the step index
and the coefficient table live in device memory, so the host issues exactly one hipGraphLaunch per step and never
touches a parameter.  Generalised over the reference's hard-coded batch 1 / 64x64 (:408,:476) to S stories."""
import torch

from . import hip
from . import switches as SW
from .engine import CIN_PAD, full_rank_runs, plan_rank1_runs


class DenoiseLoop:
    def __init__(self, unet, stories, frames, height, width, ctx_len, guidance_scale, scheduler, num_steps,
                 share_cfg_prefix=True, cfg_split=None, rank1_context=True, guidance_rescale=0.0, eta=0.0):
        """guidance_rescale (phi): with classifier-free guidance on, the guided prediction of every story is rescaled towards
        the standard deviation of its conditional one (rcdms_amd.scheduler.rescale_noise_cfg) — two more launches ahead of
        the step (rcdm_cfg_rescale_factor), which then takes the per-story factors; ignored without CFG, as diffusers does.
        eta: stochastic DDIM for a DDIMScheduler (its eta_table() through the table step, one N(0, I) draw per step staged
        by load()); every other scheduler type ignores it, as the reference's prepare_extra_step_kwargs does.
        cfg_split (rcdms_amd.dist.CfgSplit or anything with .half and .allgather(send_ptr, recv_ptr, nbytes)): the
        two-GPUs-per-story latency mode — this rank evaluates only CFG half `half` of the UNet (batch S instead of 2S),
        the halves' noise predictions are all-gathered inside the step graph and every rank applies the same CFG +
        DDIM update.  load() still takes the full CFG batch of mask / masked latents / context."""
        self.unet, self.S, self.f, self.H, self.W = unet, stories, frames, height, width
        self.gs = float(guidance_scale)
        self.reps = 2 if guidance_scale > 1.0 else 1
        self.phi = float(guidance_rescale) if self.reps == 2 else 0.0
        self.eta = 0.0
        self.T = int(num_steps)
        dev = unet.device
        self.device = dev
        # Euler / Euler-ancestral / LMS / DPM-Solver (rcdms_amd.scheduler): the whole schedule as rows of rcdm_cfg_sigma_step
        self.sigma = hasattr(scheduler, "sigma_table")
        if not hasattr(scheduler, "alphas_cumprod"):
            raise NotImplementedError(f"{type(scheduler).__name__}: only rcdms_amd.scheduler's DDIM / PNDM / Euler / "
                                      "Euler-ancestral / LMS / DPM-Solver schedulers have a fused HIP step")
        cfg = getattr(scheduler, "config", {})
        if getattr(cfg, "prediction_type", "epsilon") != "epsilon":
            raise NotImplementedError("only epsilon prediction")
        # the fused rcdm_cfg_ddim_step is DDIM eq. (12) with eta = 0 and no clipping / thresholding — what the reference
        # pipeline configures (RCDMs_pipeline.py:84-109 forces clip_sample False); anything else must not run silently
        if getattr(cfg, "clip_sample", False) or getattr(cfg, "thresholding", False):
            raise NotImplementedError("DenoiseLoop: clip_sample / thresholding are not built into the fused DDIM step "
                                      "(the reference pipeline sets clip_sample=False)")
        scheduler.set_timesteps(int(num_steps), device=None)
        # fractional on the sigma path (Euler / LMS 'linspace', Karras sigmas): the time embedding takes them as they are
        ts = torch.as_tensor(scheduler.timesteps).to("cpu", torch.float32 if self.sigma else torch.int64)
        self.timesteps = ts
        # PNDM (RCDMs_pipeline.py:72-79 accepts it; PLMS form): num_steps + 1 model evaluations, the multistep combination and
        # the update in rcdm_cfg_pndm_step from the scheduler's own per-call table
        self.pndm = hasattr(scheduler, "plms_table")
        self.T = len(ts)
        self._pndm_next = 0   # multistep only: the schedule row the history in self.hist is valid for (run() checks it)
        self.noise = None
        self.model_in = None
        if self.sigma:
            self.pndm = False
            self.coef = scheduler.sigma_table().to(dev)
            n = stories * 4 * frames * height * width
            self.hist = torch.empty(3, n, dtype=torch.float32, device=dev)      # the kernel needs no initialisation
            # the table reads the history (LMS, DPM-Solver order >= 2): a run can only continue where the last one stopped
            self.multistep = bool((self.coef[:, 4:7] != 0).any())
            self._cin0 = float(self.coef[0, 13])
            self.model_in = torch.zeros(stories, 4, frames, height, width, dtype=torch.float32, device=dev)
            if scheduler.noise_needed:
                self.noise = torch.zeros(self.T, stories, 4, frames, height, width, dtype=torch.float32, device=dev)
        elif self.pndm:
            self.coef = scheduler.plms_table().to(dev)
            self.hist = torch.zeros(5, stories * 4 * frames * height * width, dtype=torch.float32, device=dev)
        else:
            # the fused step is DDIM: the timestep list must be DDIM's — strictly decreasing at the constant stride
            # num_train_timesteps // T.  A multistep scheduler without plms_table() (e.g. a diffusers PNDMScheduler object:
            # alphas_cumprod, but N + 1 timesteps with the second one repeated) must not be run with DDIM coefficients.
            ratio = int(cfg.get("num_train_timesteps", 1000)) // self.T
            tl = ts.tolist()
            if getattr(cfg, "skip_prk_steps", None) is not None or any(a - b != ratio for a, b in zip(tl, tl[1:])):
                raise NotImplementedError(
                    f"{type(scheduler).__name__}: its timesteps are not a DDIM schedule of stride {ratio} (a multistep "
                    "scheduler?) — pass rcdms_amd.scheduler.DDIMScheduler, PNDMScheduler, EulerDiscreteScheduler, "
                    "EulerAncestralDiscreteScheduler, LMSDiscreteScheduler or DPMSolverMultistepScheduler")
            ac = torch.as_tensor(scheduler.alphas_cumprod).double().cpu()
            final = torch.as_tensor(getattr(scheduler, "final_alpha_cumprod", 1.0)).double().cpu()
            rows = []
            for t in ts.tolist():
                prev = t - ratio
                a_t, a_p = ac[t], (ac[prev] if prev >= 0 else final)
                rows.append([a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()])
            self.coef = torch.tensor(rows, dtype=torch.float32).to(dev)
            if float(eta) != 0.0:
                # stochastic DDIM is linear in x, e and one noise tensor: a row of the table kernel, no step kernel of its own
                if not hasattr(scheduler, "eta_table"):
                    raise NotImplementedError(f"{type(scheduler).__name__}: eta > 0 needs rcdms_amd.scheduler.DDIMScheduler "
                                              "(its eta_table())")
                self.eta = float(eta)
                self.sigma = True
                self.coef = scheduler.eta_table(self.eta).to(dev)
                self.hist = torch.empty(3, stories * 4 * frames * height * width, dtype=torch.float32, device=dev)
                self.multistep = False
                self._cin0 = 1.0
                self.model_in = torch.zeros(stories, 4, frames, height, width, dtype=torch.float32, device=dev)
                self.noise = torch.zeros(self.T, stories, 4, frames, height, width, dtype=torch.float32, device=dev)
        self.ts_dev = ts.to(torch.float32).to(dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.init_noise_sigma = float(getattr(scheduler, "init_noise_sigma", 1.0))

        self.factor = self._guide_ws = None
        if self.phi != 0.0:
            # per-story rescale factors and the fixed-order partial sums they are made from (written anew every step)
            self.factor = torch.empty(stories, dtype=torch.float32, device=dev)
            self._guide_ws = torch.empty(hip.cfg_rescale_workspace_bytes(stories, frames, height, width), dtype=torch.uint8,
                                         device=dev)
        self.ctx_len = ctx_len
        S, R, f, H, W = stories, self.reps, frames, height, width
        self.lat = torch.zeros(S, 4, f, H, W, dtype=torch.float32, device=dev)
        self.x_in = self.model_in if self.sigma else self.lat   # what the UNet input is assembled from
        self.mask = torch.zeros(R * S, 1, f, H, W, dtype=torch.float32, device=dev)
        self.masked = torch.zeros(R * S, 4, f, H, W, dtype=torch.float32, device=dev)
        # Two launch plans, built on first use: the general one, and the "shared prefix" one for the case the reference
        # pipeline always produces under CFG (RCDMs_pipeline.py:481-482: latents, mask and masked latents of the two
        # halves are the same tensors) where the part of the UNet ahead of the first cross-attention is evaluated once.
        self.split = cfg_split
        if cfg_split is not None and self.reps != 2:
            raise ValueError("cfg_split needs classifier-free guidance (guidance_scale > 1)")
        self.share_allowed = share_cfg_prefix and cfg_split is None
        self.rank1_allowed = bool(rank1_context) and SW.RANK1_CTX
        # (share, runs) -> the plan, its closures and its captured graph.  The model owns the plans: it keeps at most
        # MAX_LIVE_PLANS of them and tells this loop which ones it let go (plan_dropped), so no entry outlives its plan there —
        # the stage-2 autoregression walks four seen-frame patterns, i.e. four entries, per call
        self._variants = {}
        self._v = None
        if hasattr(unet, "watch_plans"):
            unet.watch_plans(self)

    def plan_dropped(self, prog):
        """The model evicted `prog` (its LRU bound, or new weights): forget the variant built around it, graph included.  The
        variant selected by the last load() stays usable until the next one — it is in use, not merely kept."""
        for key in [k for k, v in self._variants.items() if v["prog"] is prog]:
            del self._variants[key]

    def _select(self, share, runs=None):
        """share: the shared-CFG-prefix plan; runs: the full-rank image runs of the context (engine.full_rank_runs) when some
        images' context rows are all equal — the rank-1-context plan — else None."""
        # keyed by the runs the plan really uses (None where the rank-1 form is declined), as the model keys its own cache
        b = self.S * (1 if self.split is not None else self.reps)
        runs = plan_rank1_runs(runs, b * self.f, self.ctx_len) if SW.RANK1_CTX else None
        v = self._variants.get((share, runs))
        if v is not None:
            # also marks the plan as the model's most recently used one
            kept = self.unet.program(b, self.f, self.H, self.W, self.ctx_len, shared_prefix=share and self.split is None,
                                     rank1_runs=runs)
            if kept is not v["prog"]:       # not the model's plan for this key any more: build on the one it has now
                del self._variants[(share, runs)]
                v = None
        if v is None:
            S, R, f, H, W = self.S, self.reps, self.f, self.H, self.W
            if self.split is not None:
                # one CFG half here: batch rows [half * S, (half + 1) * S) of the reference's cat([latents] * 2)
                half, b = self.split.half, S
                p = self.unet.program(b, f, H, W, self.ctx_len, shared_prefix=False, rank1_runs=runs)
                eps = p.eps_out
                nbytes = eps.M * eps.ld * 2
                self.eps_full = torch.empty(2 * eps.M, eps.ld, dtype=torch.float16, device=self.device)
                m_off = half * S * f * H * W * 4          # fp32 (R*S, 1, f, H, W)
                k_off = half * S * 4 * f * H * W * 4      # fp32 (R*S, 4, f, H, W)
                table = p.time_table(self.timesteps.tolist())
                pre = [
                    lambda: hip.load_table_row(table.data_ptr(), self.step_dev.data_ptr(), p.tproj.data_ptr(), table.shape[1]),
                    lambda: hip.assemble_input(self.x_in.data_ptr(), self.mask.data_ptr() + m_off,
                                               self.masked.data_ptr() + k_off, S, 1, f, H, W, p.x_in.ptr, p.x_in.ld, CIN_PAD),
                ]
                post = [
                    lambda: self.split.allgather(eps.ptr, self.eps_full.data_ptr(), nbytes),
                    lambda: self._sched_step(self.eps_full.data_ptr(), eps.ld),
                    lambda: hip.advance_step(self.step_dev.data_ptr()),
                ]
            else:
                b = R * S
                p = self.unet.program(b, f, H, W, self.ctx_len, shared_prefix=share, rank1_runs=runs)
                # the timestep-embedding chain and all time_emb_proj rows for the T steps of the schedule, once
                table = p.time_table(self.timesteps.tolist())
                pre = [
                    lambda: hip.load_table_row(table.data_ptr(), self.step_dev.data_ptr(), p.tproj.data_ptr(), table.shape[1]),
                    lambda: hip.assemble_input(self.x_in.data_ptr(), self.mask.data_ptr(), self.masked.data_ptr(), S, R, f, H, W,
                                               p.x_in.ptr, p.x_in.ld, CIN_PAD),
                ]
                post = [
                    lambda: self._sched_step(p.eps_out.ptr, p.eps_out.ld),
                    lambda: hip.advance_step(self.step_dev.data_ptr()),
                ]
            v = self._variants[(share, runs)] = dict(prog=p, pre=pre, post=post, graph=None)
        self.shared = share
        self.rank1_runs = v["prog"].rank1_runs
        self._v = v

    def _sched_step(self, eps_ptr, ld):
        """CFG combine + scheduler.step (RCDMs_pipeline.py:492-497) on the device-resident latents, row `step` of the table."""
        S, R, f, H, W = self.S, self.reps, self.f, self.H, self.W
        if self.factor is not None:
            # guidance rescale: the factors first, from the same eps rows (the gathered ones in CFG-split mode)
            hip.cfg_rescale_factor(eps_ptr, ld, S, f, H, W, self.gs, self.phi, self._guide_ws.data_ptr(),
                                   self._guide_ws.numel(), self.factor.data_ptr())
            k = self.factor.data_ptr()
            if self.sigma:
                hip.cfg_sigma_step_scaled(eps_ptr, ld, self.lat.data_ptr(), self.model_in.data_ptr(), self.hist.data_ptr(),
                                          0 if self.noise is None else self.noise.data_ptr(), S, R, f, H, W, self.gs,
                                          self.coef.data_ptr(), self.step_dev.data_ptr(), k)
            elif self.pndm:
                hip.cfg_pndm_step_scaled(eps_ptr, ld, self.lat.data_ptr(), self.hist.data_ptr(), S, R, f, H, W, self.gs,
                                         self.coef.data_ptr(), self.step_dev.data_ptr(), k)
            else:
                hip.cfg_ddim_step_scaled(eps_ptr, ld, self.lat.data_ptr(), S, R, f, H, W, self.gs, self.coef.data_ptr(),
                                         self.step_dev.data_ptr(), k)
        elif self.sigma:
            hip.cfg_sigma_step(eps_ptr, ld, self.lat.data_ptr(), self.model_in.data_ptr(), self.hist.data_ptr(),
                               0 if self.noise is None else self.noise.data_ptr(), S, R, f, H, W, self.gs,
                               self.coef.data_ptr(), self.step_dev.data_ptr())
        elif self.pndm:
            hip.cfg_pndm_step(eps_ptr, ld, self.lat.data_ptr(), self.hist.data_ptr(), S, R, f, H, W, self.gs, self.coef.data_ptr(),
                              self.step_dev.data_ptr())
        else:
            hip.cfg_ddim_step(eps_ptr, ld, self.lat.data_ptr(), S, R, f, H, W, self.gs, self.coef.data_ptr(),
                              self.step_dev.data_ptr())

    def _cur(self):
        if self._v is None:   # a program is ~6 GB of packed weights and buffers: never build one as a side effect
            raise hip.RcdmError("DenoiseLoop: no launch plan selected yet — call load() first")
        return self._v

    prog = property(lambda self: self._cur()["prog"])
    _pre = property(lambda self: self._cur()["pre"])
    _post = property(lambda self: self._cur()["post"])

    @property
    def graph(self):
        return self._cur()["graph"]

    @graph.setter
    def graph(self, g):
        self._cur()["graph"] = g

    def _one_step_eager(self):
        for op in self._pre:
            op()
        self.prog.run_body(skip_time=True)
        for op in self._post:
            op()

    def load(self, latents, mask, masked_latents, ctx, *, noise=None, generator=None):
        """Stage the loop inputs in HBM (this is outside the timed hot loop: inputs resident when it starts).  latents: the
        unit-variance initial noise (scaled by the scheduler's init_noise_sigma here).  noise / generator: Euler-ancestral
        and DDIM with eta > 0 only — the T per-step noise tensors (T, S, 4, f, H, W), else drawn as T randn calls of shape (S, 4, f, H, W) in step
        order from `generator`, on its device (what the scheduler's step() draws, one call per step)."""
        S, R = self.S, self.reps
        assert tuple(latents.shape) == tuple(self.lat.shape), (latents.shape, self.lat.shape)
        assert tuple(mask.shape) == tuple(self.mask.shape), (mask.shape, self.mask.shape)
        assert tuple(masked_latents.shape) == tuple(self.masked.shape)
        self.lat.copy_(latents.to(self.device, torch.float32) * self.init_noise_sigma)
        if self.sigma:
            torch.mul(self.lat, self._cin0, out=self.model_in)      # scale_model_input of step 0
            if self.noise is not None:
                if noise is None:
                    noise = torch.stack([self._randn(generator) for _ in range(self.T)])
                assert noise.numel() == self.noise.numel(), (tuple(noise.shape), tuple(self.noise.shape))
                self.noise.copy_(noise.to(self.device, torch.float32).reshape(self.noise.shape))
        self.mask.copy_(mask.to(self.device, torch.float32))
        self.masked.copy_(masked_latents.to(self.device, torch.float32))
        # the CFG halves share their UNet input exactly when mask and masked latents repeat (the latents always do)
        share = (self.share_allowed and R == 2 and bool(torch.equal(self.mask[:S], self.mask[S:]))
                 and bool(torch.equal(self.masked[:S], self.masked[S:])))
        if self.split is not None:
            n = S * self.f                          # context rows per CFG half: (R*S*f, L, D), unconditional half first
            ctx = ctx[self.split.half * n:(self.split.half + 1) * n]
        # images whose L context rows are all equal (the reference's unseen frames): their cross-attention is
        # query-independent — the plan variant that skips it, selected per context the way the shared prefix is per story
        runs = None
        if self.rank1_allowed:
            runs = full_rank_runs(ctx.detach().to(self.device))
            if sum(i1 - i0 for i0, i1 in runs) >= ctx.shape[0]:
                runs = None
        self._select(share, runs)
        self.prog.set_context(ctx, force=True)   # ~3 MB + 16 small GEMMs per story: never trust a cache here
        self.step_dev.zero_()
        self._pndm_next = 0
        torch.cuda.current_stream(self.device).synchronize()

    def _randn(self, generator):
        """One N(0, I) draw of the latents' shape, as diffusers' randn_tensor makes it: on the generator's device, one
        sample per generator when given a list of them."""
        shape = tuple(self.lat.shape)
        if isinstance(generator, (list, tuple)):
            return torch.cat([torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=torch.float32).to(self.device)
                              for g in generator])
        gdev = generator.device if generator is not None else self.device
        return torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(self.device)

    def run(self, callback=None, callback_steps=1, use_graph=True, start=0, steps=None):
        """Run steps [start, start + steps) of the T-step schedule (default: all T) on the program's stream from the
        latents staged by load(); returns the latents (S,4,f,H,W) fp32 (device) after the last step run."""
        p = self.prog
        start = int(start)
        stop = self.T if steps is None else start + int(steps)
        if not (0 <= start < stop <= self.T):
            raise ValueError(f"steps [{start}, {stop}) outside the {self.T}-step schedule")
        if (self.pndm or (self.sigma and self.multistep)) and start not in (0, self._pndm_next):
            # the PLMS / LMS / DPM-Solver step is stateful (stored predictions in self.hist): a run can only continue where
            # the previous one stopped, or start over
            what = "PNDM" if self.pndm else "multistep scheduler"
            raise ValueError(f"{what}: run(start={start}) but the multistep history is valid for step {self._pndm_next} "
                             "(continue there, or start at 0 after load())")
        cur = torch.cuda.current_stream(self.device)
        p.stream.wait_stream(cur)
        with torch.cuda.stream(p.stream):
            if use_graph and self.graph is None:
                # warm every kernel up once outside capture (lazy function loading), then restore the state
                lat0 = self.lat.clone()
                # (table row 0 overwrites a history slot, PNDM's saved sample, and the sigma path's model_in)
                hist0 = self.hist.clone() if (self.pndm or self.sigma) else None
                xin0 = self.model_in.clone() if self.sigma else None
                self.step_dev.zero_()   # the warm-up step reads table / coefficient row `step`: keep it inside the tables
                self._one_step_eager()
                self.lat.copy_(lat0)
                if hist0 is not None:
                    self.hist.copy_(hist0)
                if xin0 is not None:
                    self.model_in.copy_(xin0)
                self.step_dev.zero_()
                p.stream.synchronize()
                self.graph = p.capture(pre=self._pre, post=self._post, skip_time=True)
            self.step_dev.fill_(start)
            for i in range(start, stop):
                if use_graph:
                    self.graph.launch()
                else:
                    self._one_step_eager()
                if callback is not None and i % callback_steps == 0:
                    p.stream.synchronize()
                    callback(i, self.timesteps[i].item(), self.lat)
        self._pndm_next = stop
        cur.wait_stream(p.stream)
        return self.lat


class PriorLoop:
    """The stage-1 sampling loop (reference: `for i, t in enumerate(timesteps)` of Seq_Inpaint_Prior_Pipeline.__call__,
    src/pipelines/prior_pipeline.py:311-344) as T replays of one captured hipGraph: [load t | time embedding | sequence
    assembly | ~600 transformer launches | CFG combine + UnCLIP step | step++].  The scheduler's noise for all T steps is
    drawn up front (from the caller's generator, or supplied), so the captured step is a pure function of device state."""

    def __init__(self, prior, frames, num_text_tokens, guidance_scale, scheduler, num_steps, stories=1):
        """stories: S stories per replay — n = frames * S latent rows in the order (s f), the CFG batch
        [uncond: s0 f0..4, s1 f0..4, ...; cond: the same], so batch row r * S + s holds the 5 frames of story s."""
        self.prior = prior
        self.gs = float(guidance_scale)
        self.reps = 2 if guidance_scale > 1.0 else 1   # do_classifier_free_guidance, prior_pipeline.py:236-238
        self.S = int(stories)
        if self.S < 1:
            raise ValueError(f"stories must be >= 1, got {stories}")
        self.n = int(frames) * self.S
        self.T = int(num_steps)
        dev = prior.device
        self.device = dev
        if not hasattr(scheduler, "coefficients") or not hasattr(scheduler, "alphas_cumprod"):
            raise NotImplementedError(f"{type(scheduler).__name__}: only rcdms_amd.scheduler.UnCLIPScheduler has a fused step")
        if scheduler.config.prediction_type != "sample":
            raise NotImplementedError("the prior predicts the sample (Kandinsky-2.2 prior scheduler config)")
        scheduler.set_timesteps(self.T, device=None)
        self.timesteps = torch.as_tensor(scheduler.timesteps).to("cpu", torch.int64)
        self.coef = scheduler.coefficients().to(dev)
        self.clip = float(scheduler.config.clip_sample_range) if scheduler.config.clip_sample else 0.0
        self.ts_dev = self.timesteps.to(torch.float32).to(dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.init_noise_sigma = float(getattr(scheduler, "init_noise_sigma", 1.0))
        B = self.reps * self.n
        self.prog = prior._program(B, num_text_tokens)
        E = self.prog.E
        self.lat = torch.zeros(self.n, E, dtype=torch.float32, device=dev)
        self.noise = torch.zeros(self.T, self.n, E, dtype=torch.float32, device=dev)
        self.stream = torch.cuda.Stream(device=dev)
        p = self.prog
        self._ops = ([lambda: hip.load_timestep(self.ts_dev.data_ptr(), self.step_dev.data_ptr(), p.t_dev.data_ptr(), 1)]
                     + p.step_ops(self.lat, self.n)
                     + [lambda: hip.cfg_unclip_step(p.out16.ptr, p.out16.ld, self.lat.data_ptr(), self.n, self.reps, E,
                                                    self.gs, self.clip, self.coef.data_ptr(), self.noise.data_ptr(),
                                                    self.step_dev.data_ptr()),
                        lambda: hip.advance_step(self.step_dev.data_ptr())])
        self.graph = None
        self._graph_causal = None

    def load(self, latents, proj_embedding, encoder_hidden_states, proj_embedding1, mask_label, attention_mask,
             noise=None, generator=None):
        """Stage the inputs in HBM.  latents (n, E) initial noise; the conditioning tensors already hold the CFG batch
        (B = reps * n rows, unconditional half first, as the reference's _encode_prompt / torch.cat([x] * 2) produce)."""
        assert tuple(latents.shape) == tuple(self.lat.shape), (latents.shape, self.lat.shape)
        self.lat.copy_(latents.to(self.device, torch.float32) * self.init_noise_sigma)
        if noise is None:
            noise = torch.randn(self.noise.shape, dtype=torch.float32, device=self.device, generator=generator)
        self.noise.copy_(noise.to(self.device, torch.float32))
        self.prog.set_context(proj_embedding, encoder_hidden_states, proj_embedding1, mask_label, attention_mask)
        self.step_dev.zero_()
        torch.cuda.current_stream(self.device).synchronize()

    def _one_step_eager(self):
        for op in self._ops:
            op()

    def run(self, use_graph=True):
        """All T steps; returns the final latents (n, E) fp32 on the device (before post_process_latents)."""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            if use_graph and self.graph is not None and self._graph_causal != self.prog.causal:
                self.graph = None             # the mask mode is baked into the captured launches
            if use_graph and self.graph is None:
                self._graph_causal = self.prog.causal
                lat0 = self.lat.clone()
                self.step_dev.zero_()   # the warm-up step reads table / coefficient row `step`: keep it inside the tables
                self._one_step_eager()        # load every kernel once outside capture, then restore the state
                self.lat.copy_(lat0)
                self.step_dev.zero_()
                self.stream.synchronize()
                g = hip.Graph()
                g.begin()
                try:
                    self._one_step_eager()
                finally:
                    g.end()
                self.stream.synchronize()
                self.step_dev.zero_()
                self.lat.copy_(lat0)
                self.graph = g
            for _ in range(self.T):
                if use_graph:
                    self.graph.launch()
                else:
                    self._one_step_eager()
        cur.wait_stream(self.stream)
        return self.lat
