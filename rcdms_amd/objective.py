"""The stage-2 denoising objective on the HIP path: F.mse_loss(noise_pred, noise) at one random timestep per story
(reference: train_stage2.py:420-486), evaluated forward only — the loss of a checkpoint on held-out stories, per timestep and
split into the frames the model is given and the frames it has to invent.

  DenoisingObjective   latents, masked latents, mask labels and the context in, sums of squared errors out.  Two launches
                       surround the UNet plan: rcdm_diffuse_assemble writes the noised 9-channel f16 input rows straight into the
                       plan's input buffer (the bits of ncfhw_to_rows(cat([scheduler.add_noise(x0, n, t), mask, masked], 1))),
                       rcdm_eps_sqerr folds the plan's f16 output rows against the noise into float64 sums per (story, frame), in
                       a fixed order.  No fp32 NCFHW tensor is formed on either side of the network.
  StoryObjective       frames and captions in: what PororosvDataset.__getitem__ and train_stage2.py:420-480 build for a story
                       whose first k frames are seen, from the encoders of the test path.  No kernel of its own.
  LossLog              (timestep, seen, squared error) rows kept on the device across calls; one read-back folds them into
                       timestep bins on the host.

Parity: restated from train_stage2.py and the diffusers formula, unpinned: diffusers is not installed.  Out of scope: the
backward pass and the optimiser, the stage-1 objective, min-SNR or other loss weightings, v-prediction, reading the h5 files,
caption dropping (pass "" for a dropped caption)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import hip
from .scheduler import DDPMScheduler
from .unet_program import CIN_PAD

FRAMES = 5
LATENT_SCALE = 0.18215          # train_stage2.py:428,436


@dataclass
class ObjectiveResult:
    """sq_err (B, f) float64: the sum over a frame's 4 h w elements of (eps - noise)^2; loss: 0-dim float64, the sum of sq_err
    over B 4 f h w elements — F.mse_loss(..., reduction="mean"); per_story (B,); timesteps (B,) int64; seen (B, f) bool: the
    frame's mask label is 1; loss_seen / loss_unseen: the mean over the elements of the seen / unseen frames, None where the
    batch has no such frame.  Every tensor is on the device."""
    sq_err: torch.Tensor
    loss: torch.Tensor
    per_story: torch.Tensor
    timesteps: torch.Tensor
    seen: torch.Tensor
    loss_seen: Optional[torch.Tensor]
    loss_unseen: Optional[torch.Tensor]
    frame_elements: int = 0      # 4 h w


def frame_labels(mask):
    """mask (B, 1, f, h, w) on the device -> (B, f) int8 on the host: 1 where the frame is all 1, 0 where it is all 0.  A frame
    that is neither is the reference's ValueError('please check mask label') (train_stage2.py:34-43)."""
    B, _, f = mask.shape[:3]
    m = mask.reshape(B, f, -1)
    code = torch.where((m == 1).all(-1), 1, torch.where((m == 0).all(-1), 0, 2)).to(torch.int8).cpu()
    if bool((code == 2).any()):
        raise ValueError("please check mask label")
    return code


class DenoisingObjective:
    """unet: the src.models.unet.UNet3DConditionModel of the HIP path (9 input channels); scheduler: a DDPMScheduler, None:
    the training script's, DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    (train_stage2.py:299-301; configs/testing.yaml samples on "linear" — the reference's own choice);
    noise_offset: train_stage2.py:445-449, 0 leaves the term out."""

    def __init__(self, unet, scheduler=None, noise_offset=0.0):
        if scheduler is None:
            scheduler = DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
        if not hasattr(scheduler, "noise_table"):
            raise TypeError("the objective needs a scheduler with a noise_table (rcdms_amd.scheduler.DDPMScheduler)")
        if noise_offset < 0:
            raise ValueError(f"noise_offset is >= 0, got {noise_offset}")
        self.unet, self.scheduler, self.noise_offset = unet, scheduler, float(noise_offset)
        self._workspace = None
        self._labels = None          # (mask tensor, its version, seen on the device, the number of seen frames)

    @property
    def device(self):
        return self.unet.device

    def _frame_labels(self, mask):
        """(seen (B, f) bool on the mask's device, the number of seen frames) of a mask tensor; read from the device once per
        tensor and version."""
        try:
            ver = mask._version
        except RuntimeError:
            ver = None
        c = self._labels
        if ver is not None and c is not None and c[0] is mask and c[1] == ver:
            return c[2], c[3]
        code = frame_labels(mask)
        seen, n_seen = (code == 1).to(mask.device), int((code == 1).sum())
        self._labels = (mask, ver, seen, n_seen) if ver is not None else None
        return seen, n_seen

    @torch.no_grad()
    def loss(self, latents, masked_latents, mask, context, timesteps=None, noise=None, generator=None, offsets=None):
        """latents, masked_latents (B, 4, f, h, w); mask (B, 1, f, h, w) of 0 / 1, constant over a frame; context (B f, L, D):
        the UNet's encoder_hidden_states; B stories, one timestep each, no CFG doubling.
        What is not given is drawn on the device from `generator`, in the training script's order: noise = randn(B, 4, f, h, w);
        with noise_offset > 0 the offset draw randn(B, 4, f, 1, 1) (`offsets`, where given, takes its place); timesteps =
        randint(0, T, (B,)).  A timestep outside [0, T) makes its story's loss NaN.
        Nothing of the latents, the noise, the timesteps or the result is read back.  The (B, f) frame labels of a NEW mask
        tensor are read once (cached on the tensor and its version), as unet.forward reads the rank pattern of a new context:
        they decide on the host whether the mask is valid and whether there are seen and unseen frames."""
        dev = self.device
        if dev.type != "cuda":
            raise hip.RcdmError("the denoising objective runs on the HIP path only: move the UNet to a CUDA/HIP device")
        if latents.dim() != 5 or latents.shape[1] != 4:
            raise ValueError(f"latents are (B, 4, f, h, w), got {tuple(latents.shape)}")
        B, _, f, h, w = latents.shape
        if tuple(masked_latents.shape) != (B, 4, f, h, w) or tuple(mask.shape) != (B, 1, f, h, w):
            raise ValueError(f"masked_latents are {(B, 4, f, h, w)} and mask {(B, 1, f, h, w)}, got "
                             f"{tuple(masked_latents.shape)} and {tuple(mask.shape)}")
        if context.dim() != 3 or context.shape[0] != B * f:
            raise ValueError(f"context is (B f, L, D) = ({B * f}, L, D), got {tuple(context.shape)}")
        f32 = lambda x: x.detach().to(dev, torch.float32).contiguous()
        mask_dev = mask if mask.device == dev else mask.to(dev)
        seen, n_seen = self._frame_labels(mask_dev)
        x0, masked, mask32 = f32(latents), f32(masked_latents), f32(mask_dev)
        if noise is None:
            noise = torch.randn((B, 4, f, h, w), generator=generator, device=dev, dtype=torch.float32)
        elif tuple(noise.shape) != (B, 4, f, h, w):
            raise ValueError(f"noise is {(B, 4, f, h, w)}, got {tuple(noise.shape)}")
        noise = f32(noise)
        offs = None
        if self.noise_offset > 0:
            if offsets is None:
                offsets = torch.randn((B, 4, f, 1, 1), generator=generator, device=dev, dtype=torch.float32)
            elif offsets.numel() != B * 4 * f:
                raise ValueError(f"offsets hold {B * 4 * f} values, got {tuple(offsets.shape)}")
            offs = f32(offsets).reshape(B, 4, f)
        T = int(self.scheduler.config.num_train_timesteps)
        if timesteps is None:
            timesteps = torch.randint(0, T, (B,), generator=generator, device=dev)
        t = timesteps.detach().to(dev, torch.int64).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"one timestep per story: {B}, got {t.numel()}")
        table = self.scheduler.noise_table(dev)

        prog = self.unet.program(B, f, h, w, context.shape[1], rank1_runs=self.unet._context_runs(context))
        nbytes = hip.eps_sqerr_workspace_bytes(B, f, h, w)
        if self._workspace is None or self._workspace.numel() * 8 < nbytes or self._workspace.device != dev:
            self._workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        ws, sq = self._workspace, torch.empty(B, f, dtype=torch.float64, device=dev)
        scale, optr = self.noise_offset, hip.ptr(offs)

        def fill(rows):
            hip.diffuse_assemble(x0.data_ptr(), noise.data_ptr(), optr, scale, t.data_ptr(), table.data_ptr(), T,
                                 mask32.data_ptr(), masked.data_ptr(), B, f, h, w, rows.ptr, rows.ld, CIN_PAD)

        def read(rows):
            hip.eps_sqerr(rows.ptr, rows.ld, noise.data_ptr(), optr, scale, B, f, h, w, sq.data_ptr(), ws.data_ptr(), nbytes)

        prog.forward_rows(fill, t, context, read)
        for x in (x0, masked, mask32, noise, offs, t, sq):
            if x is not None:
                x.record_stream(prog.stream)

        per = 4 * h * w
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        part = lambda sel, count: torch.where(sel, sq, zero).sum() / (count * per) if count else None
        return ObjectiveResult(sq_err=sq, loss=sq.sum() / (B * f * per), per_story=sq.sum(dim=1) / (f * per), timesteps=t,
                               seen=seen, loss_seen=part(seen, n_seen), loss_unseen=part(~seen, B * f - n_seen),
                               frame_elements=per)


class StoryObjective:
    """The training batch of train_stage2.py from frames and captions, through the test path's encoders.

    objective: a DenoisingObjective; vae: rcdms_amd.vae.AutoencoderKL; text_encoder / tokenizer: the stage-2 text tower and
    its tokenizer; image_encoder: the CLIP vision tower with projection; local_module / global_module: context.fine_stack /
    semantic_stack; frame_transform: frames -> VAE input (default rcdms_amd.image.FrameTransform at the UNet's sample size);
    clip_processor: frames -> pixel values (default ClipImageProcessor at the encoder's image size)."""

    def __init__(self, objective, vae, text_encoder, tokenizer, image_encoder, local_module, global_module, frame_transform=None,
                 clip_processor=None):
        self.objective, self.vae, self.text_encoder, self.tokenizer = objective, vae, text_encoder, tokenizer
        self.image_encoder, self.local_module, self.global_module = image_encoder, local_module, global_module
        if frame_transform is None:
            from .image import FrameTransform
            side = objective.unet.config.sample_size * 2 ** (len(vae.config.block_out_channels) - 1)
            frame_transform = FrameTransform(side, side)
        if clip_processor is None:
            from .image import ClipImageProcessor
            size = int(image_encoder.config.image_size)
            clip_processor = ClipImageProcessor(size=size, crop_size=size)
        self.frame_transform, self.clip_processor = frame_transform, clip_processor

    @property
    def device(self):
        return self.objective.device

    def _latents(self, frames_u8, generator):
        B = frames_u8.shape[0]
        z = self.vae.encode_frames(frames_u8.reshape(B * FRAMES, *frames_u8.shape[2:]), self.frame_transform)
        z = z.latent_dist.sample(generator) * LATENT_SCALE
        return z.reshape(B, FRAMES, *z.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()

    @torch.no_grad()
    def batch(self, frames_u8, texts, seen_lengths, generator=None):
        """frames_u8 (B, 5, h, w, 3) uint8; texts: B lists of 5 captions ("" for a dropped one); seen_lengths: B integers in
        0 .. 4, the length of each story's seen prefix (PororosvDataset draws it with random.randint(0, 4)).
        -> dict(latents, masked_latents, mask, context), the arguments of DenoisingObjective.loss:
          latents         encode_frames(target frames).latent_dist.sample(generator) * 0.18215, (B, 4, 5, h/8, w/8)
          masked_latents  the same of the source frames — the target frames, black beyond the prefix —, drawn second
          mask            (B, 1, 5, h/8, w/8): 1 over the prefix
          context         per story cat([local_module(hidden states of the seen frames, their text states),
                          global_module(projections of the unseen frames, their text states)]) (train_stage2.py:184-189): for a
                          prefix that is frame order.  The unseen frames' projections are the target frames' own, as in
                          training (stage 1's output takes their place at test time)."""
        from .clip import tokenizer_keywords
        dev = self.device
        if frames_u8.dim() != 5 or frames_u8.shape[1] != FRAMES or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8:
            raise ValueError(f"frames are uint8 (B, {FRAMES}, h, w, 3), got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        B = frames_u8.shape[0]
        lengths = [int(k) for k in seen_lengths]
        if len(lengths) != B or not all(0 <= k < FRAMES for k in lengths):
            raise ValueError(f"seen_lengths are {B} integers in 0..{FRAMES - 1}, got {list(seen_lengths)}")
        if len(texts) != B or not all(len(story) == FRAMES for story in texts):
            raise ValueError(f"texts are {B} lists of {FRAMES} captions")
        frames = frames_u8.to(dev)
        label = torch.tensor([[1.0 if i < k else 0.0 for i in range(FRAMES)] for k in lengths], dtype=torch.float32, device=dev)
        latents = self._latents(frames, generator)
        source = frames * label.to(torch.uint8)[:, :, None, None, None]            # black beyond the prefix
        masked = self._latents(source, generator)
        h, w = latents.shape[-2:]
        mask = label[:, None, :, None, None].expand(B, 1, FRAMES, h, w).contiguous()

        flat = [c for story in texts for c in story]
        max_len = self.text_encoder.max_position_embeddings
        tok = self.tokenizer(flat, padding="max_length", max_length=max_len, truncation=False, return_tensors="pt")
        text = self.text_encoder(tok.input_ids.to(dev), **tokenizer_keywords(self.tokenizer, self.text_encoder, tok)).last_hidden_state
        vis = self.image_encoder(self.clip_processor(images=frames.reshape(B * FRAMES, *frames.shape[2:]),
                                                     return_tensors="pt").pixel_values)
        hidden, proj = vis.last_hidden_state, vis.image_embeds.unsqueeze(1)
        seen_rows = [b * FRAMES + i for b, k in enumerate(lengths) for i in range(k)]
        unseen_rows = [b * FRAMES + i for b, k in enumerate(lengths) for i in range(k, FRAMES)]
        context = None
        for rows, module, feats in ((seen_rows, self.local_module, hidden), (unseen_rows, self.global_module, proj)):
            if rows:
                idx = torch.tensor(rows, dtype=torch.int64, device=dev)
                out = module(feats[idx], text[idx])
                if context is None:
                    context = torch.empty(B * FRAMES, *out.shape[1:], dtype=out.dtype, device=dev)
                context[idx] = out
        return dict(latents=latents, masked_latents=masked, mask=mask, context=context)

    @torch.no_grad()
    def loss(self, frames, texts, seen_lengths, timesteps=None, generator=None):
        """batch(), then DenoisingObjective.loss on it: the generator serves the two posterior draws, then the objective's."""
        return self.objective.loss(**self.batch(frames, texts, seen_lengths, generator), timesteps=timesteps, generator=generator)


@dataclass
class LossBins:
    """edges (bins + 1,) int64: bin k holds timesteps edges[k] <= t < edges[k + 1]; stories (bins,): how many rows fell into it;
    loss / loss_seen / loss_unseen (bins,) float64: the mean squared error over all / the seen / the unseen frames' elements
    of those rows, NaN where there are none."""
    edges: np.ndarray
    stories: np.ndarray
    loss: np.ndarray
    loss_seen: np.ndarray
    loss_unseen: np.ndarray


class LossLog:
    """Rows (timestep, seen (f,), sq_err (f,)) of the stories evaluated so far, kept on one device and grown geometrically
    (as rcdms_amd.kid.FeatureBank grows).  result() is the one read-back."""

    def __init__(self, device, num_train_timesteps=1000):
        self.device = torch.device(device)
        self.T = int(num_train_timesteps)
        self.n, self.f, self.frame_elements = 0, None, None
        self._buf = None             # (capacity, 1 + 2 f) float64: t | seen | sq_err — all exact in float64

    def __len__(self):
        return self.n

    def append(self, result):
        if not isinstance(result, ObjectiveResult):
            raise TypeError(f"append takes an ObjectiveResult, got {type(result).__name__}")
        B, f = result.sq_err.shape
        if self.f is None:
            self.f, self.frame_elements = f, int(result.frame_elements)
        if (f, int(result.frame_elements)) != (self.f, self.frame_elements):
            raise ValueError(f"the log holds stories of {self.f} frames of {self.frame_elements} elements, got {f} of "
                             f"{result.frame_elements}")
        rows = torch.cat([result.timesteps.to(self.device, torch.float64)[:, None], result.seen.to(self.device, torch.float64),
                          result.sq_err.to(self.device)], dim=1)
        need = self.n + B
        if self._buf is None or need > self._buf.shape[0]:
            cap = max(need, 2 * (0 if self._buf is None else self._buf.shape[0]), 64)      # geometric growth
            buf = torch.empty(cap, 1 + 2 * f, dtype=torch.float64, device=self.device)
            if self.n:
                buf[:self.n] = self._buf[:self.n]
            self._buf = buf
        self._buf[self.n:need] = rows
        self.n = need
        return self

    def rows(self):
        """(t (n,) int64, seen (n, f) bool, sq_err (n, f) float64) on the host: the one read-back."""
        if self.n == 0:
            raise ValueError("no rows yet")
        r = self._buf[:self.n].cpu().numpy()
        f = self.f
        return r[:, 0].astype(np.int64), r[:, 1:1 + f] != 0, np.ascontiguousarray(r[:, 1 + f:])

    def result(self, bins=10):
        """Mean loss, mean over the seen and mean over the unseen frames per timestep bin (bin = t * bins // T; a timestep
        outside [0, T) is left out).  Folded on the host in float64 in row order, a row's frames in ascending order: the same
        rows give the same bits, however they were appended."""
        bins = int(bins)
        if not 1 <= bins <= self.T:
            raise ValueError(f"bins is 1..{self.T}, got {bins}")
        t, seen, sq = self.rows()
        sums, counts = np.zeros((3, bins)), np.zeros((3, bins), np.int64)
        stories = np.zeros(bins, np.int64)
        for i in range(t.shape[0]):
            if not 0 <= t[i] < self.T:
                continue
            k = int(t[i]) * bins // self.T
            stories[k] += 1
            for j in range(self.f):
                for which in (0, 1 if seen[i, j] else 2):
                    sums[which, k] = sums[which, k] + sq[i, j]
                    counts[which, k] += 1
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(counts > 0, sums / (counts * float(self.frame_elements)), np.nan)
        edges = np.array([-(-k * self.T // bins) for k in range(bins + 1)], np.int64)
        return LossBins(edges=edges, stories=stories, loss=mean[0], loss_seen=mean[1], loss_unseen=mean[2])

    def save(self, path):
        """.npz with `t`, `seen`, `sq_err`, `frame_elements`, `num_train_timesteps`."""
        t, seen, sq = self.rows()
        np.savez(path, t=t, seen=seen, sq_err=sq, frame_elements=self.frame_elements, num_train_timesteps=self.T)

    @classmethod
    def load(cls, path, device):
        with np.load(path) as z:
            t, seen, sq = z["t"], z["seen"], z["sq_err"]
            per, T = int(z["frame_elements"]), int(z["num_train_timesteps"])
        if sq.ndim != 2 or seen.shape != sq.shape or t.shape != (sq.shape[0],) or sq.dtype != np.float64:
            raise ValueError(f"`sq_err` is (n, f) float64 with `seen` of its shape and `t` (n,), got {sq.dtype} {sq.shape}")
        self = cls(device, T)
        dev = self.device
        self.append(ObjectiveResult(sq_err=torch.from_numpy(sq).to(dev), loss=None, per_story=None,
                                    timesteps=torch.from_numpy(t.astype(np.int64)).to(dev), seen=torch.from_numpy(seen).to(dev),
                                    loss_seen=None, loss_unseen=None, frame_elements=per))
        return self
