"""Story batches: S stories through stage 1 and stage 2 in one process.

The reference runs a test set as two processes — stage1_batchtest_rcdms_model.py writes `{index}_{j}.npy` embeddings,
stage2_batchtest_rcdms_model.py reads them back — one story per pipeline call.  Here:
  * the helpers both public pipelines use for their story axis (a `prompt` of S lists of five captions): the argument
    checks and `place_story_rows`, which puts every story's CFG rows where the captured loops expect them;
  * `write_stage1_embeds`, the files of stage1…:260,264 for a stage-2 process of the old kind;
  * `StoryRunner`: uint8 frames + captions -> CLIP vision forward -> stage 1 -> cosine figure -> hand-off -> stage 2,
    batched over S, all tensors staying on the device; on request the per-frame SSIM / PSNR / CLIP-I of the generated frames
    against their targets (rcdms_amd.metrics); on request stage 2's autoregression — five passes at batch S, the kept
    frames handed on as device bytes (`source_from_bytes`) — and the stage-2 driver's PNG files (`write_story_pngs`).
The hot paths are the two captured loops (rcdms_amd.sampler) at batch S; this module is glue around them."""
import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

FRAMES = 5


# ---- the story axis of the two pipelines ---------------------------------------------------------------------------------

def story_count(prompt, frames=FRAMES):
    """None for a call in the single-story form (a string, or a flat list of strings); S for a list of S lists of `frames`
    strings.  Anything in between — flat and nested entries mixed, a story with another number of captions, no story at
    all — is a ValueError."""
    if not isinstance(prompt, (list, tuple)):
        return None
    nested = [isinstance(p, (list, tuple)) for p in prompt]
    if not any(nested):
        return None
    if not all(nested):
        raise ValueError("`prompt` mixes captions and lists of captions: pass either a flat list of captions (one story) or a "
                         "list of S lists (S stories)")
    for s, story in enumerate(prompt):
        if len(story) != frames or not all(isinstance(c, str) for c in story):
            raise ValueError(f"`prompt[{s}]` must hold {frames} caption strings, one per frame, got {len(story)} entries")
    return len(prompt)


def check_story_axis(name, value, shape):
    """ValueError unless `value` is a tensor of exactly `shape` (whose leading entry is the story count)."""
    got = tuple(value.shape) if hasattr(value, "shape") else None
    if got != tuple(shape):
        raise ValueError(f"`{name}` must be {tuple(shape)} for {shape[0]} stories, got "
                         f"{got if got is not None else type(value).__name__}")


def story_generators(generator, stories):
    """One generator per story: a list of S generators as given, one generator (or None) for every story — the S stories
    then draw from it one after the other, as S single-story calls would."""
    if isinstance(generator, (list, tuple)):
        if len(generator) != stories:
            raise ValueError(f"a list of {len(generator)} generators for {stories} stories: pass one generator, or one per story")
        return list(generator)
    return [generator] * stories


def place_story_rows(rows, reps, frames=FRAMES):
    """rows: S tensors (reps * frames, ...), story s's rows as the single-story call builds them (CFG half r, frame f at row
    r * frames + f).  -> (reps * S * frames, ...) in the order of the captured loops, whose batch row is r * S + s
    (rcdms_amd.sampler.DenoiseLoop): out[(r * S + s) * frames + f] = rows[s][r * frames + f].  S = 1 is the identity."""
    S = len(rows)
    for s, t in enumerate(rows):
        if t.shape[0] != reps * frames or t.shape[1:] != rows[0].shape[1:]:
            raise ValueError(f"story {s} holds rows {tuple(t.shape)}, expected ({reps * frames}, ...) like story 0 "
                             f"{tuple(rows[0].shape)}")
    x = torch.stack(list(rows))                                       # (S, reps * frames, ...)
    x = x.reshape(S, reps, frames, *x.shape[2:]).transpose(0, 1)      # (reps, S, frames, ...)
    return x.reshape(reps * S * frames, *x.shape[3:])


def write_stage1_embeds(save_dir, index, embeds):
    """The files the stage-1 driver leaves for story `index` (stage1_batchtest_rcdms_model.py:260,264): `{index}_{j}.npy`,
    the fp32 embedding (E,) of frame j, j = 0..4, and `{index}.npy`, all five (5, E).  The stage-2 driver reads
    `{index}_{1..4}.npy` back (stage2_batchtest_rcdms_model.py:291-294).  -> the paths written."""
    e = embeds.detach().to("cpu", torch.float32).numpy() if isinstance(embeds, torch.Tensor) else np.asarray(embeds, np.float32)
    if e.ndim != 2 or e.shape[0] != FRAMES:
        raise ValueError(f"a story's embeddings are ({FRAMES}, E), got {e.shape}")
    os.makedirs(save_dir, exist_ok=True)
    paths = []
    for j in range(FRAMES):
        paths.append(os.path.join(save_dir, f"{index}_{j}.npy"))
        np.save(paths[-1], np.ascontiguousarray(e[j]))
    paths.append(os.path.join(save_dir, f"{index}.npy"))
    np.save(paths[-1], np.ascontiguousarray(e))
    return paths


# ---- stage 1 -> stage 2 --------------------------------------------------------------------------------------------------

@dataclass
class StoryResult:
    videos: Any                       # by output_type; None when stage 2 did not run
    image_embeds: torch.Tensor        # (S, 5, E) stage-1 output
    target_embeds: torch.Tensor       # (S, 5, E) CLIP embeddings of the five given frames
    cosine: torch.Tensor              # (S, 5) the figure the stage-1 driver prints (:239,258)
    ssim: Optional[torch.Tensor] = None    # (S, 5) float64, generated frame against its resized target (metrics=("ssim",))
    psnr: Optional[torch.Tensor] = None    # (S, 5) float64, inf for identical frames (metrics=("psnr",))
    clip_i: Optional[torch.Tensor] = None  # (S, 5) cosine of the generated frames' CLIP embeddings and target_embeds ("clip_i")
    lpips: Optional[torch.Tensor] = None   # (S, 5) float64, LPIPS of the generated frame and its resized target (metrics=("lpips",))
    frames_u8: Optional[torch.Tensor] = None   # (S, 5, H, W, 3) device uint8: the kept frames a stage-2 autoregressive run handed on


METRICS = ("ssim", "psnr", "clip_i", "lpips")
FEATURE_SOURCES = ("clip", "inception")
AUTOREG_OUTPUTS = ("tensor", "uint8", "png")


def source_from_bytes(frames_u8):
    """uint8 frames (..., H, W, 3) -> fp32 (..., 3, H, W) in [-1, 1]: what the driver's reg_augment (ToTensor, then
    Normalize([0.5], [0.5]), no resize) makes of a PNG file it wrote from those bytes (stage2…:306-343) — (b / 255 - 0.5) / 0.5
    element by element, on the frames' device.  The 256 values are computed once on the host, where `/ 255` is the IEEE
    division ToTensor makes (a device kernel may multiply by a rounded 1 / 255 instead), and looked up by byte there."""
    table = _SOURCE_VALUES.get(frames_u8.device)
    if table is None:
        table = ((torch.arange(256, dtype=torch.float32) / 255 - 0.5) / 0.5).to(frames_u8.device)
        _SOURCE_VALUES[frames_u8.device] = table
    return table[frames_u8.to(torch.int32)].movedim(-1, -3)


_SOURCE_VALUES = {}


def write_story_pngs(frames_dir, grid_dir, indices, frames_u8, targets_u8=None, files=None):
    """The stage-2 driver's files for S stories, encoded on the device (image.encode_png, checkpoint.story_grid_png):
    frames_dir: `{index}_{i}.png`, frame i of story `index` (stage2…:362,384); grid_dir: `{index}.png`, the 2 x 5 grid of the
    five generated frames over the five targets (:389-401).  frames_u8 / targets_u8: device uint8 (S, 5, H, W, 3); files:
    the S x 5 frame files where the caller has encoded them already.  A directory that is None is skipped.  -> the files."""
    S = frames_u8.shape[0]
    if frames_dir is not None:
        if files is None:
            from .image import encode_png
            flat = encode_png(frames_u8.reshape(S * FRAMES, *frames_u8.shape[2:]))
            files = [flat[s * FRAMES:(s + 1) * FRAMES] for s in range(S)]
        os.makedirs(frames_dir, exist_ok=True)
        for s, index in enumerate(indices):
            for i in range(FRAMES):
                with open(os.path.join(frames_dir, f"{index}_{i}.png"), "wb") as f:
                    f.write(files[s][i])
    if grid_dir is not None:
        from .checkpoint import story_grid_png
        os.makedirs(grid_dir, exist_ok=True)
        for s, index in enumerate(indices):
            with open(os.path.join(grid_dir, f"{index}.png"), "wb") as f:
                f.write(story_grid_png([*frames_u8[s], *targets_u8[s]], 2, FRAMES))
    return files


class StoryRunner:
    """What the two drivers do per story (stage1…:146-261, stage2…:267-376), for S stories per call.

    prior_pipe: Seq_Inpaint_Prior_Pipeline; stage2_pipe: RCDMsPipeline (None: stage 1 only); image_encoder: the CLIP vision
    tower with projection (`.image_embeds`, `.last_hidden_state`); clip_processor: frames -> pixel values (default
    rcdms_amd.image.ClipImageProcessor at the encoder's image size); frame_transform: frames -> stage-2 source frames in
    [-1, 1] (default rcdms_amd.image.FrameTransform at the UNet's sample size); inception: an
    rcdms_amd.inception.InceptionV3Features (uint8 frames -> (n, 2048) fp32), the extractor of feature_source="inception";
    classifier: a second InceptionV3Features, the character classifier whose logits label_counts scores (other weights than the
    FID network's, usually preprocess="pillow").
    lpips: an rcdms_amd.lpips.LpipsNet, the network behind metrics=("lpips",)."""

    def __init__(self, prior_pipe, stage2_pipe, image_encoder, clip_processor=None, frame_transform=None, inception=None,
                 classifier=None, lpips=None):
        self.prior_pipe, self.stage2_pipe, self.image_encoder = prior_pipe, stage2_pipe, image_encoder
        self.inception, self.classifier, self.lpips = inception, classifier, lpips
        if clip_processor is None:
            from .image import ClipImageProcessor
            size = int(image_encoder.config.image_size)
            clip_processor = ClipImageProcessor(size=size, crop_size=size)
        if frame_transform is None and stage2_pipe is not None:
            from .image import FrameTransform
            side = stage2_pipe.unet.config.sample_size * stage2_pipe.vae_scale_factor
            frame_transform = FrameTransform(side, side)
        self.clip_processor, self.frame_transform = clip_processor, frame_transform
        self._black_white = None

    @property
    def device(self):
        return self.prior_pipe.device

    def _pixels(self, frames):
        return self.clip_processor(images=frames, return_tensors="pt").pixel_values

    def black_white_embeds(self, like):
        """(black, white): `image_embeds` (E,) of the all-black and the all-white image (stage1…:160-163), encoded once per
        runner — the drivers encode them again for every story.  like: uint8 frames (n, H, W, 3) giving size and device."""
        if self._black_white is None:
            bw = torch.zeros(2, *like.shape[1:], dtype=torch.uint8, device=like.device)
            bw[1] = 255
            e = self.image_encoder(self._pixels(bw)).image_embeds
            self._black_white = (e[0].clone(), e[1].clone())
        return self._black_white

    def stage1_inputs(self, target, black, white, mode, done=None):
        """(imgs_proj_embeds1, mask_label), each (S, 5, 1, E).  done None: the mode's own rows (stage1…:164-178) —
        "continue": [frame 0, black x 4] under the mask [white, black x 4]; "visualization": black throughout.  done
        (S, i, E), i >= 1: pass i of the autoregressive loop (:190-224) — the i embeddings generated so far, then black, under
        a mask whose first i entries are white."""
        S, E = target.shape[0], target.shape[-1]
        proj = black.expand(S, FRAMES, E).clone()
        label = black.expand(S, FRAMES, E).clone()
        if done is not None:
            i = done.shape[1]
            proj[:, :i] = done
            label[:, :i] = white
        elif mode == "continue":
            proj[:, 0] = target[:, 0]
            label[:, 0] = white
        return proj.unsqueeze(2), label.unsqueeze(2)

    @torch.no_grad()
    def __call__(self, frames, texts, mode="continue", autoreg=False, num_inference_steps=50, prior_steps=25,
                 guidance_scale=7.5, prior_guidance_scale=4.0, generator=None, prior_generator=None, output_type="tensor",
                 save_dir=None, indices=None, stage2=None, fix_context_order=False, guidance_rescale=0.0, eta=0.0, metrics=(),
                 stage2_autoreg=False, frames_dir=None, grid_dir=None, feature_stats=None, feature_banks=None,
                 feature_source="clip", labels=None, label_counts=None, label_frames=None, logit_bank=None):
        """frames: uint8 (S, 5, Hs, Ws, 3) RGB, host or device; texts: S lists of five captions (lower-cased here, as the
        drivers do).  stage2: run stage 2 (default: in "continue" mode when the runner has a stage-2 pipeline).  save_dir /
        indices: also write each story's stage-1 embeddings as `{index}_{j}.npy` / `{index}.npy` (indices default 0..S-1).
        guidance_rescale / eta: stage 2's sampling arguments (RCDMsPipeline.__call__); the stage-1 prior has neither.
        metrics: any of "ssim", "psnr", "clip_i", "lpips" — per-frame figures of the generated frames against the five given frames
        resized to the stage-2 size with Pillow's bilinear filter (the driver's vis_augment, stage2…:390-396), in the result's
        fields of those names, computed on the device (rcdms_amd.metrics; "clip_i" is one more vision forward; "lpips" runs the
        runner's `lpips` network, rcdms_amd.lpips.LpipsNet, on the same resized targets "ssim" / "psnr" use — without one it is a
        ValueError before anything is launched).  They need a stage-2 run with output_type="uint8".  metrics=(): nothing more
        is launched.
        feature_stats: (generated, reference), two rcdms_amd.frechet.FeatureStats of the embedding width: the CLIP embeddings of
        the 5 S generated frames are added to `generated` (the forward "clip_i" runs, done once when both are asked for) and
        target_embeds to `reference`, for a set-level Fréchet distance (frechet_distance; a CLIP-FD) over as many calls as the
        caller likes.  Its requirements are those of "clip_i".  None: nothing more is launched.
        feature_banks: (generated, reference), two rcdms_amd.kid.FeatureBank of the embedding width: the same rows, kept rather
        than summed, for a kernel distance (kernel_distance; a CLIP-KID).  The same forward, the same requirements.  None: nothing
        more is launched.
        feature_source: where the rows of feature_stats / feature_banks come from.  "clip" (default): the CLIP embeddings, as
        above.  "inception": the runner's `inception` extractor — `generated` receives inception(the 5 S generated uint8
        frames), `reference` inception(the five given uint8 frames of every story), 2048 wide: the inputs of an Inception FID /
        KID.  The CLIP forward over the generated frames then runs only when "clip_i" is asked for as well.  Without an extractor,
        or with an output type that leaves no uint8 frames, "inception" is a ValueError before anything is launched.
        label_counts: an rcdms_amd.scores.LabelCounts: the runner's `classifier` runs on the generated uint8 frames and its logits
        are scored against `labels`, uint8 (S, 5, C) character labels (non-zero: present), C the classifier's num_classes and
        the counts' — the sufficient statistics of Char-F1 / Frm-Acc over as many calls as the caller likes, no read-back.
        label_frames: the frame indices scored, default all five (continuation papers score (1, 2, 3, 4): frame 0 is given).
        logit_bank: an rcdms_amd.kid.FeatureBank of width inception.num_classes that keeps the logits of the generated frames
        (for rcdms_amd.scores.inception_score), from the one forward feature_source="inception" runs on them — required —, which
        then also returns its logits: no second forward.  Both need a stage-2 run that leaves uint8 frames; a missing
        extractor, missing labels or a width mismatch is a ValueError before anything is launched.  None: nothing more is
        launched.
        stage2_autoreg: the stage-2 driver's --autoreg loop (stage2…:304-362) for the S stories, independent of `autoreg`
        (stage 1's loop): five stage-2 calls at batch S, pass i keeping frame i of every story —
          pass 0: the call of stage2_autoreg=False (given frame 0 seen, image_embeds_1 its hidden state, proj_embeds_0
                  embeds[1:]);
          pass i >= 1: the generated frames 0..i-1 seen — frame 0 too: the given one is replaced (:306-311) —, as
                  source_from_bytes of the bytes kept, no file in between; image_embeds_1 the vision tower's hidden states
                  of those i frames (the reference's call omits both embeddings and cannot run: they follow the frames in
                  source_img here, so that the fine stack sees what the VAE sees; each kept frame is encoded once);
                  proj_embeds_0 embeds[i:].
        Every pass takes this call's guidance_scale, num_inference_steps, fix_context_order, guidance_rescale and eta, and
        the same `generator` object(s): with one generator per story, story s's five passes draw from it one after the other
        (posterior noise, initial latents, per-step noise; then the next pass) as the driver's five calls do; one generator
        for S > 1 stories serves them pass-major — all stories of pass 0, then of pass 1 … — which no sequence of
        single-story runs reproduces.  `videos` holds frame i of pass i in the layout of output_type ("tensor", "uint8" or
        "png"), `frames_u8` the kept bytes; metrics are computed from those bytes whatever the output_type.
        frames_dir / grid_dir (any stage-2 run with one of those three output types): the driver's `{index}_{i}.png` per
        generated frame and `{index}.png`, the generated frames over the resized targets (write_story_pngs)."""
        metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
        for m in metrics:
            if m not in METRICS:
                raise ValueError(f"metric {m!r}: any of {METRICS}")
        if "lpips" in metrics and self.lpips is None:
            raise ValueError('metrics=("lpips",) needs a network: build the runner with lpips=LpipsNet(...)')
        if mode not in ("continue", "visualization"):
            raise ValueError("check mode")                                      # stage1…:180
        if feature_source not in FEATURE_SOURCES:
            raise ValueError(f"feature_source {feature_source!r}: one of {FEATURE_SOURCES}")
        if feature_source == "inception":
            if self.inception is None:
                raise ValueError('feature_source="inception" needs an extractor: build the runner with inception=InceptionV3Features(...)')
            if output_type != "uint8" and not stage2_autoreg:
                raise ValueError(f'feature_source="inception" reads uint8 frames: pass output_type="uint8", not {output_type!r}')
        if stage2 is None:
            stage2 = mode == "continue" and self.stage2_pipe is not None
        if stage2 and mode == "visualization":
            raise ValueError('stage 2 in mode "visualization": the reference leaves image_embeds_1 / proj_embeds_0 undefined '
                             "there and fails at stage2_batchtest_rcdms_model.py:367 — run mode=\"continue\", or stage2=False")
        if stage2 and self.stage2_pipe is None:
            raise ValueError("stage 2 asked for, but the runner was built without a stage-2 pipeline")
        for name, pair, kind in (("feature_stats", feature_stats, "FeatureStats"), ("feature_banks", feature_banks, "FeatureBank")):
            if pair is None:
                continue
            if len(pair) != 2:
                raise ValueError(f"{name} is a pair (generated, reference) of {kind}")
            if not stage2:
                raise ValueError(f"{name} collect the embeddings of the frames stage 2 generates: this call runs no stage 2")
            if output_type != "uint8" and not stage2_autoreg:
                raise ValueError(f"{name} are taken from uint8 frames: pass output_type=\"uint8\", not {output_type!r}")
        for name, given in (("label_counts", label_counts), ("logit_bank", logit_bank)):
            if given is None:
                continue
            if not stage2:
                raise ValueError(f"{name} takes the logits of the frames stage 2 generates: this call runs no stage 2")
            if output_type != "uint8" and not stage2_autoreg:
                raise ValueError(f"{name} is filled from uint8 frames: pass output_type=\"uint8\", not {output_type!r}")
        labels, label_frames = self._check_labels(frames, labels, label_counts, label_frames)
        if logit_bank is not None:
            if self.inception is None or feature_source != "inception":
                raise ValueError('logit_bank keeps the logits of the forward feature_source="inception" runs: build the runner with '
                                 'inception=InceptionV3Features(...) and pass feature_source="inception"')
            if logit_bank.d != self.inception.num_classes:
                raise ValueError(f"logit_bank is {logit_bank.d} wide, the extractor has {self.inception.num_classes} classes")
        if metrics and not stage2:
            raise ValueError(f"metrics {metrics} compare the frames stage 2 generates with their targets: this call runs no stage 2")
        if stage2_autoreg and not stage2:
            raise ValueError("stage2_autoreg=True repeats stage 2 five times: this call runs no stage 2")
        if stage2_autoreg and output_type not in AUTOREG_OUTPUTS:
            raise ValueError(f"stage2_autoreg=True hands uint8 frames from pass to pass: output_type is one of {AUTOREG_OUTPUTS}, "
                             f"not {output_type!r}")
        files_asked = frames_dir is not None or grid_dir is not None
        if files_asked and not stage2:
            raise ValueError("frames_dir / grid_dir hold the frames stage 2 generates: this call runs no stage 2")
        if files_asked and output_type not in AUTOREG_OUTPUTS:
            raise ValueError(f"frames_dir / grid_dir are written from uint8 frames: output_type is one of {AUTOREG_OUTPUTS}, "
                             f"not {output_type!r}")
        if metrics and output_type != "uint8" and not stage2_autoreg:
            raise ValueError(f"metrics {metrics} are computed on uint8 frames: pass output_type=\"uint8\", not {output_type!r}")
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[1] != FRAMES or frames.shape[-1] != 3:
            raise ValueError(f"frames are uint8 (S, {FRAMES}, H, W, 3), got {frames.dtype} {tuple(frames.shape)}")
        S = frames.shape[0]
        if story_count(texts) != S:
            raise ValueError(f"`texts` must be {S} lists of {FRAMES} captions, one list per story of `frames`")
        indices = list(range(S)) if indices is None else list(indices)
        if len(indices) != S:
            raise ValueError(f"{len(indices)} indices for {S} stories")
        texts = [[c.lower() for c in story] for story in texts]
        frames = frames.to(self.device)

        # one vision forward over the 5 * S target frames: targets, stage 1's source_clip[0], stage 2's image_embeds_1
        vis = self.image_encoder(self._pixels(frames.reshape(S * FRAMES, *frames.shape[2:])))
        target = vis.image_embeds.reshape(S, FRAMES, -1)
        black, white = self.black_white_embeds(frames[0])

        def prior(proj, label):
            return self.prior_pipe(prompt=texts, imgs_proj_embeds1=proj, mask_label=label, video_length=FRAMES,
                                   guidance_scale=prior_guidance_scale, generator=prior_generator,
                                   num_inference_steps=prior_steps).image_embeds

        if autoreg:
            # five passes (stage1…:186-242): pass i conditions on the rows kept from passes 0..i-1 and keeps its row i
            kept = []
            for i in range(FRAMES):
                out = prior(*self.stage1_inputs(target, black, white, mode, torch.stack(kept, dim=1) if kept else None))
                kept.append(out[:, i].to(target.dtype))
            embeds = torch.stack(kept, dim=1)
        else:
            embeds = prior(*self.stage1_inputs(target, black, white, mode))
        embeds = embeds.float()
        cosine = torch.nn.functional.cosine_similarity(embeds, target.float(), dim=-1)
        if save_dir is not None:
            for s, index in enumerate(indices):
                write_stage1_embeds(save_dir, index, embeds[s])
        videos = frames_u8 = None
        if stage2:
            pipe, ft = self.stage2_pipe, self.frame_transform
            H, W = ft.height, ft.width
            h, w = H // pipe.vae_scale_factor, W // pipe.vae_scale_factor
            source = torch.full((S, FRAMES, 3, H, W), -1.0, dtype=torch.float32, device=self.device)   # mask_augment(black)
            source[:, 0] = ft(frames[:, 0])
            label = torch.zeros(S, FRAMES, h, w, dtype=torch.float32, device=self.device)
            label[:, 0] = 1.0
            hidden = vis.last_hidden_state.reshape(S, FRAMES, *vis.last_hidden_state.shape[1:])
            kw = dict(prompt=texts, video_length=FRAMES, height=H, width=W, guidance_scale=guidance_scale, generator=generator,
                      num_inference_steps=num_inference_steps, fix_context_order=fix_context_order,
                      guidance_rescale=guidance_rescale, eta=eta)
            img1, proj0 = [hidden[s, :1] for s in range(S)], [embeds[s, 1:].unsqueeze(1) for s in range(S)]
            if stage2_autoreg:
                videos, frames_u8 = self._stage2_autoreg(source, label, img1, embeds, output_type, kw)
            elif files_asked:
                videos, frames_u8 = self._stage2_bytes(source, label, img1, proj0, output_type, kw)
            else:
                videos = pipe(source_img=source, image_embeds_1=img1, proj_embeds_0=proj0, mask_label=label,
                              output_type=output_type, **kw).videos
            files = None
            if frames_u8 is not None and output_type == "png":
                from .image import encode_png
                flat = encode_png(frames_u8.reshape(S * FRAMES, *frames_u8.shape[2:]))
                videos = files = [flat[s * FRAMES:(s + 1) * FRAMES] for s in range(S)]
            if files_asked:
                write_story_pngs(frames_dir, grid_dir, indices, frames_u8,
                                 self.target_frames(frames) if grid_dir is not None else None, files)
        figures = {}
        if metrics or feature_stats is not None or feature_banks is not None or label_counts is not None or logit_bank is not None:
            figures = self.story_metrics(frames_u8 if stage2_autoreg else videos, frames, target, metrics, feature_stats,
                                         feature_banks, feature_source, labels, label_counts, label_frames, logit_bank)
        return StoryResult(videos=videos, image_embeds=embeds, target_embeds=target, cosine=cosine, **figures,
                           frames_u8=frames_u8 if stage2_autoreg else None)

    def _check_labels(self, frames, labels, label_counts, label_frames):
        """The label arguments of a call, checked on the host -> (labels as a uint8 tensor or None, label_frames as a list or None)."""
        if label_counts is None:
            if labels is not None or label_frames is not None:
                raise ValueError("labels / label_frames are scored into label_counts: pass a LabelCounts")
            return None, None
        if self.classifier is None:
            raise ValueError("label_counts needs a classifier: build the runner with classifier=InceptionV3Features(...)")
        if labels is None:
            raise ValueError("label_counts scores the classifier's logits against `labels`: uint8 (S, 5, C)")
        labels = torch.as_tensor(labels)
        C = self.classifier.num_classes
        if labels.dtype != torch.uint8 or labels.dim() != 3 or tuple(labels.shape[:2]) != (np.shape(frames)[0], FRAMES):
            raise ValueError(f"labels are uint8 (S, {FRAMES}, C) for the S stories of `frames`, got {labels.dtype} {tuple(labels.shape)}")
        if labels.shape[2] != C or label_counts.num_classes != C:
            raise ValueError(f"the classifier has {C} classes, labels {labels.shape[2]} and label_counts {label_counts.num_classes}")
        if label_frames is not None:
            label_frames = [int(i) for i in label_frames]
            if not label_frames or len(set(label_frames)) != len(label_frames) or not all(0 <= i < FRAMES for i in label_frames):
                raise ValueError(f"label_frames are distinct frame indices in 0..{FRAMES - 1}, got {label_frames}")
        return labels, label_frames

    def _stage2_bytes(self, source, label, img1, proj0, output_type, kw):
        """One stage-2 call whose frames are also wanted as bytes -> (videos, device uint8 (S, 5, H, W, 3)).  "tensor": the
        float frames and the bytes of the same decode; "uint8" / "png": the bytes (the caller encodes the files)."""
        if output_type == "tensor":
            out = self.stage2_pipe(source_img=source, image_embeds_1=img1, proj_embeds_0=proj0, mask_label=label,
                                   output_type="tensor", return_uint8=True, **kw)
            return out.videos, out.frames_u8
        u8 = self.stage2_pipe(source_img=source, image_embeds_1=img1, proj_embeds_0=proj0, mask_label=label,
                              output_type="uint8", **kw).videos
        return u8, u8

    def _stage2_autoreg(self, source, label, img1, embeds, output_type, kw):
        """The five passes.  source / label / img1: pass 0's, i.e. the plain call's; embeds (S, 5, E).  -> (videos in the
        layout of "tensor" or "uint8", the kept bytes (S, 5, H, W, 3)); everything handed on stays on the device."""
        S = source.shape[0]
        source, label = source.clone(), label.clone()
        kept_u8, kept_video, seen_hidden = [], [], []
        for i in range(FRAMES):
            if i >= 1:
                new = kept_u8[i - 1]                                                # (S, H, W, 3), kept by the pass before
                source[:, i - 1] = source_from_bytes(new)                           # pass 1: replaces the given frame 0
                label[:, i - 1] = 1.0
                seen_hidden.append(self.image_encoder(self._pixels(new)).last_hidden_state)   # (S, tokens, width), once per frame
                img1 = [torch.stack([hs[s] for hs in seen_hidden]) for s in range(S)]
            proj0 = [embeds[s, max(i, 1):].unsqueeze(1) for s in range(S)]
            videos, u8 = self._stage2_bytes(source, label, img1, proj0, output_type, kw)
            kept_u8.append(u8[:, i].contiguous())
            if output_type == "tensor":
                kept_video.append(videos[:, :, i])
        frames_u8 = torch.stack(kept_u8, dim=1)
        return (torch.stack(kept_video, dim=2) if output_type == "tensor" else frames_u8), frames_u8

    def target_frames(self, frames):
        """The five given frames of every story at the stage-2 size, uint8 (S, 5, H, W, 3): Pillow's bilinear resize as bytes,
        one launch for all 5 S frames."""
        from .image import resampler, to_device_frames
        S = frames.shape[0]
        flat, = to_device_frames(frames.reshape(S * FRAMES, *frames.shape[2:]), self.device)
        ft = self.frame_transform
        r = resampler(flat.shape[1], flat.shape[2], ft.height, ft.width, ft.resample, None, flat.device)
        return r.to_uint8(flat, ft.flip_channels).view(S, FRAMES, ft.height, ft.width, 3)

    def story_metrics(self, videos, frames, target_embeds, metrics, feature_stats=None, feature_banks=None, feature_source="clip",
                      labels=None, label_counts=None, label_frames=None, logit_bank=None):
        """videos: uint8 (S, 5, H, W, 3) as stage 2 returns them; frames: the given uint8 (S, 5, Hs, Ws, 3) on the device.
        -> {name: (S, 5) tensor} for the names in `metrics`.  feature_stats: (generated, reference) FeatureStats that take the
        embeddings of `videos` and target_embeds; feature_banks: (generated, reference) FeatureBanks that keep the same rows.
        feature_source="inception": both pairs receive the runner's Inception features of `videos` and of `frames` instead.
        label_counts / labels / label_frames / logit_bank: as in __call__ (checked there)."""
        from .metrics import frame_metrics
        if feature_source not in FEATURE_SOURCES:
            raise ValueError(f"feature_source {feature_source!r}: one of {FEATURE_SOURCES}")
        wants_rows = feature_stats is not None or feature_banks is not None
        inception = feature_source == "inception"
        if inception and self.inception is None:
            raise ValueError('feature_source="inception" needs an extractor: build the runner with inception=InceptionV3Features(...)')
        if inception and wants_rows and videos.dtype != torch.uint8:
            raise ValueError(f'feature_source="inception" reads uint8 frames, got {videos.dtype}')
        S = videos.shape[0]
        out = {}
        if "lpips" in metrics and self.lpips is None:
            raise ValueError('metrics=("lpips",) needs a network: build the runner with lpips=LpipsNet(...)')
        targets = self.target_frames(frames) if any(m in metrics for m in ("ssim", "psnr", "lpips")) else None
        if "lpips" in metrics:
            out["lpips"] = self.lpips(videos, targets)
        if "ssim" in metrics or "psnr" in metrics:
            fm = frame_metrics(videos, targets)
            if "ssim" in metrics:
                out["ssim"] = fm.ssim.view(S, FRAMES)
            if "psnr" in metrics:
                out["psnr"] = fm.psnr.view(S, FRAMES)
        if "clip_i" in metrics or (wants_rows and not inception):
            e = self.image_encoder(self._pixels(videos.reshape(S * FRAMES, *videos.shape[2:]))).image_embeds
        if logit_bank is not None:
            if not inception or videos.dtype != torch.uint8:
                raise ValueError('logit_bank is filled by the forward of feature_source="inception" over uint8 frames')
            gen_rows, gen_logits = self.inception(videos.reshape(S * FRAMES, *videos.shape[2:]), return_logits=True)
            logit_bank.append(gen_logits)
            if wants_rows:
                ref_rows = self.inception(frames.reshape(S * FRAMES, *frames.shape[2:]))
        elif wants_rows and inception:
            gen_rows = self.inception(videos.reshape(S * FRAMES, *videos.shape[2:]))
            ref_rows = self.inception(frames.reshape(S * FRAMES, *frames.shape[2:]))
        elif wants_rows:
            gen_rows, ref_rows = e.reshape(S * FRAMES, -1), target_embeds.reshape(S * FRAMES, -1)
        if feature_stats is not None:
            generated, reference = feature_stats
            generated.update(gen_rows)
            reference.update(ref_rows)
        if feature_banks is not None:
            generated, reference = feature_banks
            generated.append(gen_rows)
            reference.append(ref_rows)
        if label_counts is not None:
            if self.classifier is None or labels is None or videos.dtype != torch.uint8:
                raise ValueError("label_counts needs the runner's classifier, `labels` and uint8 frames")
            _, logits = self.classifier(videos.reshape(S * FRAMES, *videos.shape[2:]), return_logits=True)
            logits, lab = logits.view(S, FRAMES, -1), torch.as_tensor(labels).to(logits.device)
            if label_frames is not None:
                logits, lab = logits[:, list(label_frames)], lab[:, list(label_frames)]
            label_counts.update(logits, lab)
        if "clip_i" in metrics:
            out["clip_i"] = torch.nn.functional.cosine_similarity(e.reshape(S, FRAMES, -1).float(), target_embeds.float(), dim=-1)
        return out
