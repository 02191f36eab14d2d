"""Mirror of the reference's src/pipelines/RCDMs_pipeline.py interface: `RCDMsPipeline` (and the alias
`AnimationPipeline` that stage2_batchtest_rcdms_model.py:246 actually instantiates), `RCDMsPipelineOutput`,
`local_feature`, same constructor (RCDMs_pipeline.py:64-80) and `__call__` signature (:374-398).

What runs where:
  * the denoising loop (:455-503) — T x [UNet + CFG + scheduler step] — runs on MI355X as replays of one captured hipGraph
    (rcdms_amd.sampler.DenoiseLoop); this is the hot path and has no torch fallback;
  * prompt / VAE / context-stack glue around it calls the user-supplied torch modules exactly as the reference
    does (they are inputs of this pipeline, not part of it).
Reference quirks kept by default: exactly 5 frames per story, batch 1 per call, and the context
rows re-joined as cat([seen, unseen]) (:450) — pass fix_context_order=True to restore (b f) row order.
Generalised: any (height, width) divisible by 64, CFG on or off; a `prompt` of S lists of five captions runs S stories through
one captured loop (`_call_stories`), each computing what its single-story call computes."""
import inspect
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import numpy as np
import torch
import torch.nn as nn

from rcdms_amd.clip import tokenizer_keywords
from rcdms_amd.sampler import DenoiseLoop
from rcdms_amd.story import check_story_axis, place_story_rows, story_count, story_generators
from ..models.unet import UNet3DConditionModel, _Config


class local_feature(nn.Module):
    """Text-queries x visual-keys MHA "stack" (reference RCDMs_pipeline.py:35-52): user-side torch module."""

    def __init__(self, text_dim, vis_dim, hidden_dim, num_heads):
        super().__init__()
        self.hidden_dim, self.num_heads = hidden_dim, num_heads
        self.text_fc = nn.Linear(text_dim, hidden_dim)
        self.vis_fc = nn.Linear(vis_dim, hidden_dim)
        self.multihead_attn = nn.MultiheadAttention(embed_dim=hidden_dim, num_heads=num_heads)

    def forward(self, vis_f, text_f):
        q = self.text_fc(text_f).transpose(0, 1)
        kv = self.vis_fc(vis_f).transpose(0, 1)
        return self.multihead_attn(q, kv, kv)[0].transpose(0, 1)


@dataclass
class RCDMsPipelineOutput:
    videos: Union[torch.Tensor, np.ndarray]
    frames_u8: Optional[torch.Tensor] = None   # return_uint8=True: the bytes of `videos`, device uint8 (b, f, H, W, 3)


def _force_config(obj, key, value):
    cfg = dict(obj.config)
    cfg[key] = value
    obj._internal_dict = _Config(cfg)


class RCDMsPipeline:
    _optional_components = []
    FRAMES = 5  # hard-coded in the reference (:261,:430,:476); the PE table of the motion modules has 5 rows

    def __init__(self, vae, text_encoder, tokenizer, unet: UNet3DConditionModel, local_module, global_module, scheduler,
                 vae_decoder=None):
        # the two scheduler-config mutations of the reference ctor (:84-109)
        if hasattr(scheduler, "config"):
            if hasattr(scheduler.config, "steps_offset") and scheduler.config.steps_offset != 1:
                _force_config(scheduler, "steps_offset", 1)
            if hasattr(scheduler.config, "clip_sample") and scheduler.config.clip_sample is True:
                _force_config(scheduler, "clip_sample", False)
        if hasattr(unet, "config") and getattr(unet.config, "sample_size", None) is not None \
                and unet.config.sample_size < 64 and hasattr(unet.config, "_diffusers_version"):
            _force_config(unet, "sample_size", 64)
        self.vae, self.text_encoder, self.tokenizer, self.unet = vae, text_encoder, tokenizer, unet
        # optional rcdms_amd.vae.AutoencoderKLDecoder: decodes the 5 frames in one HIP launch plan instead of five
        # `self.vae.decode` calls (:281); `vae` is still used for `encode`.  Passing rcdms_amd.vae.AutoencoderKL as
        # `vae` itself puts both halves on the HIP path.
        from rcdms_amd.vae import AutoencoderKLDecoder
        if vae_decoder is None and isinstance(vae, AutoencoderKLDecoder):
            vae_decoder = vae
        self.vae_decoder = vae_decoder
        self.local_module, self.global_module, self.scheduler = local_module, global_module, scheduler
        boc = getattr(getattr(vae, "config", None), "block_out_channels", None)
        self.vae_scale_factor = 2 ** (len(boc) - 1) if boc is not None else 8
        self._loop = None
        self._loop_key = None
        self._progress_bar_config = {}

    # ---- DiffusionPipeline conveniences used by the reference's callers ------------------------------------------
    @property
    def components(self):
        return dict(vae=self.vae, text_encoder=self.text_encoder, tokenizer=self.tokenizer, unet=self.unet,
                    local_module=self.local_module, global_module=self.global_module, scheduler=self.scheduler)

    def to(self, device):
        for m in (self.vae, self.text_encoder, self.unet, self.local_module, self.global_module):
            if isinstance(m, nn.Module):
                m.to(device)
        return self

    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    def enable_sequential_cpu_offload(self, gpu_id=0):
        raise NotImplementedError("the HIP path keeps the UNet resident in HBM (288 GB); CPU offload is not supported")

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    def progress_bar(self, total):
        from tqdm import tqdm
        return tqdm(total=total, **self._progress_bar_config)

    # ---- glue identical in behaviour to the reference ----------------------------------------------------------------
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt):
        """(:175-256) tokenise to text_encoder.max_position_embeddings, take last_hidden_state; uncond rows first."""
        batch_size = len(prompt) if isinstance(prompt, list) else 1
        max_len = self.text_encoder.max_position_embeddings

        def embed(texts):
            tok = self.tokenizer(texts, padding="max_length", max_length=max_len, truncation=False, return_tensors="pt")
            return self.text_encoder(tok.input_ids.to(device),
                                     **tokenizer_keywords(self.tokenizer, self.text_encoder, tok)).last_hidden_state

        text = embed(prompt)
        if not do_classifier_free_guidance:
            return text
        if negative_prompt is None:
            uncond_tokens = [""] * batch_size
        elif type(prompt) is not type(negative_prompt):
            raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                            f" {type(prompt)}.")
        elif isinstance(negative_prompt, str):
            uncond_tokens = [negative_prompt]
        elif batch_size != len(negative_prompt):
            raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                             f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt`"
                             " matches the batch size of `prompt`.")
        else:
            uncond_tokens = negative_prompt
        uncond = embed(uncond_tokens)
        seq = uncond.shape[1]
        uncond = uncond.repeat(1, num_videos_per_prompt, 1).view(batch_size * num_videos_per_prompt, seq, -1)
        return torch.cat([uncond, text])

    def encode_mask(self, mask_label, num_videos_per_prompt, do_classifier_free_guidance):
        """(:259-272) (5, h, w) -> (10, h, w): the same mask for the unconditional half."""
        if not do_classifier_free_guidance:
            return mask_label
        seq_len = mask_label.shape[1]
        uncond = mask_label.repeat(1, num_videos_per_prompt, 1).view(self.FRAMES * num_videos_per_prompt, seq_len, -1)
        return torch.cat([uncond, mask_label])

    def mask2list_label(self, mask_label, encoder_hidden_states, do_classifier_free_guidance):
        """(:350-371) split the text rows into seen (mask all 1) / unseen (mask all 0) frames."""
        seen = self._seen_rows(mask_label)
        return encoder_hidden_states[seen], encoder_hidden_states[~seen]

    @staticmethod
    def _seen_rows(mask_label):
        flat = mask_label.reshape(mask_label.shape[0], -1)
        all0, all1 = (flat == 0).all(dim=1), (flat == 1).all(dim=1)
        if not bool((all0 | all1).all()):
            raise ValueError('please check mask label')
        return all1.cpu()

    def build_context(self, text_embeddings, masked_label, image_embeds_1, proj_embeds_0, fix_context_order=False):
        """(:444-450) rich context = cat([local(seen rows), global(unseen rows)]); the reference's row order is
        seen-first, which differs from the latents' (b f) order whenever CFG is on."""
        dev, dt = text_embeddings.device, text_embeddings.dtype
        ehs_1, ehs_0 = self.mask2list_label(masked_label, text_embeddings, True)
        seen = self._seen_rows(masked_label)
        feature_1 = self.local_module(image_embeds_1.to(dtype=dt, device=dev), ehs_1)
        feature_0 = self.global_module(proj_embeds_0.to(dtype=dt, device=dev), ehs_0)
        ctx = torch.cat([feature_1, feature_0], dim=0)
        if fix_context_order:
            order = torch.cat([torch.nonzero(seen).flatten(), torch.nonzero(~seen).flatten()])
            fixed = torch.empty_like(ctx)
            fixed[order.to(ctx.device)] = ctx
            ctx = fixed
        return ctx

    # One VAE launch plan holds at most this many pixels: the convolution kernels address an activation through 32-bit byte
    # offsets (RCDM_ESHAPE beyond 2 GB: 16 frames of 512 x 512 at the SD-1.5 VAE's 256 f16 channels at full resolution).  Two
    # stories at 512 x 512 is the largest plan that has been run; 5 * S frames beyond it go in runs of whole stories.
    VAE_PIXELS_PER_CALL = 10 * 512 * 512

    def _vae_chunks(self, x, scale=1):
        """x (n, c, h, w), n a multiple of the 5 frames of a story (`scale`: pixels per entry of h and w) -> x in the fewest
        runs of whole stories whose frames hold at most VAE_PIXELS_PER_CALL pixels, one story at the least: [x] for a single
        story at any size, and for any batch of small frames."""
        n, f = x.shape[0], self.FRAMES
        px = f * x.shape[2] * x.shape[3] * scale * scale
        per = f * max(1, self.VAE_PIXELS_PER_CALL // px)
        if n <= per or n % f:
            return [x]
        return [x[i:i + per] for i in range(0, n, per)]

    def decode_latents(self, latents, with_uint8=False):
        """(:274-287) one frame at a time through the user's VAE.  with_uint8: -> (video, bytes) — the same decode also
        truncated to bytes on the device (rcdms_amd.image.frames_to_uint8), uint8 (b, f, H, W, 3)."""
        f = latents.shape[2]
        latents = (1 / 0.18215 * latents).permute(0, 2, 1, 3, 4).reshape(-1, latents.shape[1], *latents.shape[3:])
        if self.vae_decoder is not None:
            video = torch.cat([self.vae_decoder.decode(z).sample for z in self._vae_chunks(latents, self.vae_scale_factor)])
        else:
            frames = [self.vae.decode(latents[i:i + 1]).sample for i in range(latents.shape[0])]
            video = torch.cat(frames)
        video = video.reshape(-1, f, *video.shape[1:]).permute(0, 2, 1, 3, 4)
        out = (video / 2 + 0.5).clamp(0, 1).cpu().float().numpy()
        if with_uint8:
            from rcdms_amd.image import frames_to_uint8
            return out, frames_to_uint8(video)
        return out

    def decode_latents_uint8(self, latents):
        """output_type="uint8": the frames of decode_latents truncated to bytes — trunc(clamp(x / 2 + 0.5, 0, 1) * 255), the
        driver's `(x * 255).astype(uint8)` — as a device uint8 tensor (b, f, H, W, 3).  With the HIP decoder the bytes come
        straight from its f16 pixel rows (decode_uint8); with any other `vae` from its fp32 sample (frames_to_uint8)."""
        from rcdms_amd.image import frames_to_uint8
        f = latents.shape[2]
        latents = (1 / 0.18215 * latents).permute(0, 2, 1, 3, 4).reshape(-1, latents.shape[1], *latents.shape[3:])
        if self.vae_decoder is not None:
            frames = torch.cat([self.vae_decoder.decode_uint8(z) for z in self._vae_chunks(latents, self.vae_scale_factor)])
        else:
            frames = frames_to_uint8(torch.cat([self.vae.decode(latents[i:i + 1]).sample for i in range(latents.shape[0])]))
        return frames.reshape(-1, f, *frames.shape[1:])

    def prepare_extra_step_kwargs(self, generator, eta):
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in params:
            kw["eta"] = eta
        if "generator" in params:
            kw["generator"] = generator
        return kw

    def check_inputs(self, prompt, height, width, callback_steps):
        if not isinstance(prompt, str) and not isinstance(prompt, list):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type"
                             f" {type(callback_steps)}.")

    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, dtype, device, generator,
                        latents=None):
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective"
                             f" batch size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            if isinstance(generator, list):
                latents = torch.cat([torch.randn(shape, generator=g, device=device, dtype=dtype) for g in generator], dim=0)
            else:
                latents = torch.randn(shape, generator=generator, device=device, dtype=dtype)
        elif latents.shape != shape:
            raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
        return latents.to(device) * self.scheduler.init_noise_sigma

    # ---- the hot loop ----------------------------------------------------------------------------------------------
    def denoise(self, latents, mask, masked_latents, context, num_inference_steps, guidance_scale, callback=None,
                callback_steps=1, generator=None, noise=None, guidance_rescale=0.0, eta=0.0):
        """latents (S,4,f,h,w) unit-variance noise (DenoiseLoop.load applies init_noise_sigma); mask (R*S,1,f,h,w);
        masked_latents (R*S,4,f,h,w); context (R*S*f, L, D); generator: the per-step noise of Euler-ancestral and of DDIM
        with eta > 0; guidance_rescale / eta: as DenoiseLoop takes them (both are part of the cached loop's key)."""
        S, _, f, h, w = latents.shape
        key = (S, f, h, w, context.shape[1], float(guidance_scale), int(num_inference_steps), id(self.scheduler),
               id(self.unet), self.unet._weights_gen, float(guidance_rescale), float(eta))
        if self._loop is None or self._loop_key != key:
            self._loop = DenoiseLoop(self.unet, S, f, h, w, context.shape[1], guidance_scale, self.scheduler,
                                     num_inference_steps, guidance_rescale=guidance_rescale, eta=eta)
            self._loop_key = key
        self._loop.load(latents, mask, masked_latents, context, noise=noise, generator=generator)
        return self._loop.run(callback=callback, callback_steps=callback_steps)

    @torch.no_grad()
    def __call__(self, prompt, source_img, image_embeds_1, proj_embeds_0, mask_label, video_length: Optional[int],
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, negative_prompt=None, num_videos_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "tensor", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: Optional[int] = 1,
                 fix_context_order: bool = False, png_match: bool = False, guidance_rescale: float = 0.0,
                 return_uint8: bool = False, **kwargs):
        """guidance_rescale (what the reference driver passes, stage2_batchtest_rcdms_model.py:352): Lin et al. 2023 §3.4 on
        the guided noise prediction, inside the captured step; 0 is off.  eta: stochastic DDIM with a DDIMScheduler (the
        per-step noise from `generator`), ignored by every other scheduler type (prepare_extra_step_kwargs, :289-298).
        return_uint8: with the float output types, also `frames_u8` in the result — the same decode truncated to bytes on the
        device, what output_type="uint8" holds (the frames the stage-2 autoregression hands to its next pass)."""
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        if video_length != self.FRAMES:
            raise ValueError(f"a story has exactly {self.FRAMES} frames (reference RCDMs_pipeline.py:261,430,476)")
        if story_count(prompt, video_length) is not None:
            return self._call_stories(prompt, source_img, image_embeds_1, proj_embeds_0, mask_label, height, width,
                                      num_inference_steps, guidance_scale, negative_prompt, num_videos_per_prompt, generator,
                                      latents, output_type, return_dict, callback, callback_steps, fix_context_order,
                                      png_match, guidance_rescale, eta, return_uint8)
        batch_size = 1
        device = self._execution_device
        cfg_on = guidance_scale > 1.0
        reps = 2 if cfg_on else 1

        prompt = prompt if isinstance(prompt, list) else [prompt] * batch_size
        if negative_prompt is not None and not isinstance(negative_prompt, list):
            negative_prompt = [negative_prompt] * batch_size
        text_embeddings = self._encode_prompt(prompt, device, num_videos_per_prompt, cfg_on, negative_prompt)

        # source frames -> masked latents (:427-432)
        src = source_img.unsqueeze(0)
        src = src.reshape(-1, *src.shape[2:])
        masked_latents = self.vae.encode(src.to(dtype=text_embeddings.dtype, device=device)).latent_dist.sample(
            generator=generator)
        masked_latents = masked_latents.reshape(-1, self.FRAMES, *masked_latents.shape[1:]).permute(0, 2, 1, 3, 4) * 0.18215
        masked_latents = torch.cat([masked_latents] * reps * num_videos_per_prompt) if cfg_on else masked_latents

        masked_label = mask_label.squeeze().to(dtype=text_embeddings.dtype, device=device)
        masked_label = self.encode_mask(masked_label, num_videos_per_prompt, cfg_on)
        if cfg_on:
            image_embeds_1 = torch.cat([image_embeds_1] * 2 * num_videos_per_prompt)
            proj_embeds_0 = torch.cat([proj_embeds_0] * 2 * num_videos_per_prompt)
        context = self.build_context(text_embeddings, masked_label, image_embeds_1, proj_embeds_0, fix_context_order)

        latents = self.prepare_latents(batch_size * num_videos_per_prompt, 4, video_length, height, width,
                                       text_embeddings.dtype, device, generator, latents)
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        mask5 = masked_label.view(reps, 1, self.FRAMES, h, w)   # the reference hard-codes (2,1,5,64,64) at :476

        return self._sample_and_decode(latents, mask5, masked_latents, context, text_embeddings.dtype, num_inference_steps,
                                       guidance_scale, generator, None, callback, callback_steps, output_type, return_dict,
                                       png_match, guidance_rescale, eta, return_uint8)

    def _sample_and_decode(self, latents, mask5, masked_latents, context, dtype, num_inference_steps, guidance_scale,
                           generator, noise, callback, callback_steps, output_type, return_dict, png_match,
                           guidance_rescale=0.0, eta=0.0, return_uint8=False):
        """The captured loop on the staged inputs, then the VAE decode by `output_type` (:455-513); the batch axis of
        `latents` is the story axis."""
        with self.progress_bar(total=num_inference_steps) as bar:
            def on_step(i, t, lat):
                bar.update()
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, lat)
            # prepare_latents applied init_noise_sigma (as the reference does); DenoiseLoop.load applies it itself
            final = self.denoise(latents / self.scheduler.init_noise_sigma, mask5, masked_latents, context,
                                 num_inference_steps, guidance_scale, callback=on_step if (callback is not None) else None,
                                 callback_steps=1, generator=generator, noise=noise, guidance_rescale=guidance_rescale,
                                 eta=eta)
            if callback is None:
                bar.update(num_inference_steps)

        if output_type in ("uint8", "png"):
            video = self.decode_latents_uint8(final.to(dtype))
            if output_type == "png":                       # [[bytes] * f] * b: one PNG file per frame, encoded on the device
                from rcdms_amd.image import encode_png
                b, f = video.shape[:2]
                files = encode_png(video.reshape(b * f, *video.shape[2:]), match=png_match)
                video = [files[i * f:(i + 1) * f] for i in range(b)]
            return RCDMsPipelineOutput(videos=video) if return_dict else video
        frames_u8 = None
        if return_uint8:
            video, frames_u8 = self.decode_latents(final.to(dtype), with_uint8=True)
        else:
            video = self.decode_latents(final.to(dtype))
        if output_type == "tensor":
            video = torch.from_numpy(video)
        if not return_dict:
            return (video, frames_u8) if return_uint8 else video
        return RCDMsPipelineOutput(videos=video, frames_u8=frames_u8)

    def _call_stories(self, prompt, source_img, image_embeds_1, proj_embeds_0, mask_label, height, width,
                      num_inference_steps, guidance_scale, negative_prompt, num_videos_per_prompt, generator, latents,
                      output_type, return_dict, callback, callback_steps, fix_context_order, png_match,
                      guidance_rescale=0.0, eta=0.0, return_uint8=False):
        """`prompt` is S lists of five captions: S stories through one captured loop.  Story s is the single-story call on
        story s's inputs with story s's generator (one generator: the S calls made one after the other with it).  Every
        story's ten context rows and mask rows are built as in that call and then placed at the loop's batch rows r * S + s
        (rcdms_amd.story.place_story_rows); the prompts take one text-encoder call and the 5 * S source frames one VAE
        encode.  source_img (S, 5, 3, H, W), mask_label (S, 5, h, w), image_embeds_1 / proj_embeds_0 lists of S tensors,
        latents (S, 4, 5, h, w) -> videos (S, 3, 5, H, W)."""
        f = self.FRAMES
        S = story_count(prompt, f)
        if num_videos_per_prompt != 1:
            raise NotImplementedError("num_videos_per_prompt != 1 with a story axis")
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        check_story_axis("source_img", source_img, (S, f, 3, height, width))
        check_story_axis("mask_label", mask_label, (S, f, h, w))
        for name, v in (("image_embeds_1", image_embeds_1), ("proj_embeds_0", proj_embeds_0)):
            if not isinstance(v, (list, tuple)) or len(v) != S:
                raise ValueError(f"`{name}` is a list of {S} tensors, one per story (the seen-frame count may differ), got "
                                 f"{type(v).__name__}" + (f" of length {len(v)}" if isinstance(v, (list, tuple)) else ""))
        if latents is not None:
            check_story_axis("latents", latents, (S, 4, f, h, w))
        gens = story_generators(generator, S)
        device = self._execution_device
        cfg_on = guidance_scale > 1.0
        reps = 2 if cfg_on else 1

        flat = [c for story in prompt for c in story]
        if isinstance(negative_prompt, list):
            if story_count(negative_prompt, f) != S:
                raise ValueError(f"`negative_prompt` must be one string or {S} lists of {f} strings, as `prompt`")
            negative_prompt = [c for story in negative_prompt for c in story]
        elif negative_prompt is not None:
            negative_prompt = [negative_prompt] * (S * f)
        # rows [uncond: s0 f0..4, s1 f0..4, ...; cond: the same]
        text = self._encode_prompt(flat, device, 1, cfg_on, negative_prompt)
        dt = text.dtype

        src = source_img.reshape(S * f, *source_img.shape[2:]).to(dtype=dt, device=device)
        # one encode over the 5 * S frames (in runs of whole stories past VAE_PIXELS_PER_CALL)
        dists = [self.vae.encode(x).latent_dist for x in self._vae_chunks(src)]
        per_story = all(hasattr(d, "mean") and hasattr(d, "std") for d in dists)
        if per_story:
            mean, std = torch.cat([d.mean for d in dists]), torch.cat([d.std for d in dists])
        need_noise = hasattr(self.scheduler, "sigma_table") and bool(getattr(self.scheduler, "noise_needed", False))
        # stochastic DDIM draws per step too (the scheduler types that ignore eta have sigma_table() or plms_table())
        need_noise = need_noise or (float(eta) != 0.0 and hasattr(self.scheduler, "eta_table"))
        T = int(num_inference_steps)
        if need_noise:
            self.scheduler.set_timesteps(T, device=None)
            T = len(self.scheduler.timesteps)
        z, lat, ctx, masks, noise = [], [], [], [], []
        for s in range(S):
            g = gens[s]
            # the draws of the single-story call, in its order: posterior noise, initial latents, the per-step noise
            if per_story:
                m, sd = mean[s * f:(s + 1) * f], std[s * f:(s + 1) * f]
                z.append(m + sd * torch.randn(m.shape, generator=g, device=m.device, dtype=m.dtype))
            else:
                z.append(self.vae.encode(src[s * f:(s + 1) * f]).latent_dist.sample(generator=g))
            lat.append(self.prepare_latents(1, 4, f, height, width, dt, device, g, None if latents is None
                                            else latents[s:s + 1]))
            if need_noise:
                gdev = g.device if g is not None else device
                noise.append(torch.stack([torch.randn((1, 4, f, h, w), generator=g, device=gdev, dtype=torch.float32).to(device)
                                          for _ in range(T)]))
            label = self.encode_mask(mask_label[s].to(dtype=dt, device=device), 1, cfg_on)
            text_s = torch.cat([text[(r * S + s) * f:(r * S + s + 1) * f] for r in range(reps)])
            img1, proj0 = image_embeds_1[s], proj_embeds_0[s]
            if cfg_on:
                img1, proj0 = torch.cat([img1] * 2), torch.cat([proj0] * 2)
            ctx.append(self.build_context(text_s, label, img1, proj0, fix_context_order))
            masks.append(label)
        z = torch.stack(z).permute(0, 2, 1, 3, 4) * 0.18215            # (S, 4, 5, h, w)
        masked_latents = torch.cat([z] * reps)                          # batch row r * S + s
        mask5 = place_story_rows(masks, reps).view(reps * S, 1, f, h, w)
        context = place_story_rows(ctx, reps)
        noise = torch.cat(noise, dim=1) if need_noise else None         # (T, S, 4, 5, h, w)
        return self._sample_and_decode(torch.cat(lat), mask5, masked_latents, context, dt, num_inference_steps,
                                       guidance_scale, None, noise, callback, callback_steps, output_type, return_dict,
                                       png_match, guidance_rescale, eta, return_uint8)


# stage2_batchtest_rcdms_model.py:30 imports RCDMsPipeline but :246 instantiates AnimationPipeline
AnimationPipeline = RCDMsPipeline
