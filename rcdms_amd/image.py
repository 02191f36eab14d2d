"""uint8 frames in, uint8 frames out: the image front and back end of the story pipeline on the HIP path.

Front end — what stage2_batchtest_rcdms_model.py:172-196,255-276 (and mydatasets/*.py) do on the host with PIL,
torchvision and transformers before the first kernel runs:
  ClipImageProcessor   `CLIPImageProcessor()`: PIL bicubic resize of the shortest edge to 224, centre crop 224, * 1/255,
                       CLIP mean / std  ->  the `pixel_values` of CLIPVisionEncoder
  FrameTransform       `ToPILImage -> Resize([H, W]) -> ToTensor -> Normalize(0.5, 0.5)`: PIL bilinear resize, [-1, 1]
                       ->  the input of AutoencoderKL.encode
Both are one rcdm_image_resample launch per batch of equally sized frames.  Pillow's 8-bit resample is integer
arithmetic on coefficient tables of 22 fractional bits; `resample_tables` builds those tables on the host in float64
exactly as Pillow does and the kernel does the integer multiply-accumulate, so the resized bytes equal Pillow's bit for bit.
Back end — RCDMs_pipeline.py:274-287 and the driver's tensor2list: `frames_to_uint8` is (x / 2 + 0.5).clamp(0, 1) * 255
truncated, from the VAE decoder's f16 rows or an fp32 NCHW tensor straight to uint8 HWC (rcdm_frames_to_u8).
Files — the driver's PIL.Image.save calls (:378-401): `encode_png` / `save_png` / `PngEncoder` turn device uint8 frames into
complete PNG files on the device (rcdm_png_encode: adaptive filters, literal-only Huffman deflate), one download per call.
Files, reading — the drivers' cv2.imdecode over the test set (:41-46, :446-450) and Image.open(...).convert("RGB") (:256-260,
:304-343): `decode_png` / `load_png` / `PngDecoder` walk the container on the host (chunk headers only), upload the files as
one byte buffer and leave the frames on the device as uint8 HWC, RGB or — cv2's order, which the drivers hand on unflipped —
BGR (rcdm_png_decode: inflate, Adler-32, the five filters and the colour conversion on the device, one wavefront per file).

No CPU path: a call without a GPU raises (only `resample_tables` and the geometry helpers are host code)."""
import ctypes
import math
import struct
import types
import zlib

import numpy as np
import torch

from . import hip

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22
MAX_TAPS = 40
_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
_PIL_FILTER = {2: "bilinear", 3: "bicubic"}          # PIL.Image.Resampling values the drivers pass


def _filter_name(f):
    f = _PIL_FILTER.get(int(f), f) if not isinstance(f, str) else f.lower()
    if f not in _SUPPORT:
        raise ValueError(f"resample filter {f!r}: bilinear or bicubic")
    return f


def _weights(x, filt):
    x = np.abs(x)
    if filt == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_tables(in_size, out_size, filter, box=None, window=None):
    """Pillow's coefficient tables of one axis (precompute_coeffs + normalize_coeffs_8bpc), in numpy float64.
    box = (in0, in1): the source interval that maps onto the out_size outputs (default: the whole axis); window =
    (first, count): only these output indices are tabulated (a crop behind the resize).  An axis Pillow's resize skips
    (size kept, no box) gives the identity table.
    -> SimpleNamespace(k int32 [count][taps], bounds int32 [count][2] = (first source index, taps used), taps)."""
    in_size, out_size = int(in_size), int(out_size)
    filt = _filter_name(filter)
    first, count = (0, out_size) if window is None else (int(window[0]), int(window[1]))
    if in_size <= 0 or out_size <= 0 or first < 0 or count <= 0 or first + count > out_size:
        raise ValueError(f"resample_tables({in_size}, {out_size}, window={window})")
    in0, in1 = (0.0, float(in_size)) if box is None else (float(box[0]), float(box[1]))
    if not (0.0 <= in0 < in1 <= in_size):
        raise ValueError(f"box {box} outside the axis of {in_size}")
    if in_size == out_size and in0 == 0.0 and in1 == in_size:
        k = np.full((count, 1), 1 << PRECISION_BITS, dtype=np.int32)
        bounds = np.stack([np.arange(first, first + count), np.ones(count, dtype=np.int64)], axis=1).astype(np.int32)
        return types.SimpleNamespace(k=k, bounds=bounds, taps=1)
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = _SUPPORT[filt] * fs
    taps = int(math.ceil(support)) * 2 + 1
    xx = np.arange(first, first + count, dtype=np.float64)
    center = in0 + (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)
    n = np.minimum(np.trunc(center + support + 0.5), float(in_size)) - xmin
    i = np.arange(taps, dtype=np.float64)[None, :]
    live = i < n[:, None]
    w = np.where(live, _weights((i + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs), filt), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                  # summed left to right, as the C loop does (np.sum pairs)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = w * float(1 << PRECISION_BITS)
    k = np.where(live, np.trunc(np.where(q < 0, q - 0.5, q + 0.5)), 0.0).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return types.SimpleNamespace(k=np.ascontiguousarray(k), bounds=np.ascontiguousarray(bounds), taps=taps)


def tile_rows(bounds, tile=hip.IMAGE_TILE):
    """Largest source-row span of one `tile`-row output tile (rcdm_resample_desc.tile_rows)."""
    span = 1
    for t in range(0, len(bounds), tile):
        b = bounds[t:t + tile].astype(np.int64)
        span = max(span, int((b[:, 0] + b[:, 1]).max() - b[:, 0].min()))
    return span


def shortest_edge_size(h, w, size):
    """transformers' get_resize_output_image_size(default_to_square=False): (new_h, new_w)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def clip_geometry(h, w, size, crop):
    """-> (resized_h, resized_w, top, left) of the shortest-edge resize and the centre crop behind it."""
    rh, rw = shortest_edge_size(h, w, size)
    if rh < crop or rw < crop:
        raise ValueError(f"a {h}x{w} image resized to {rh}x{rw} is smaller than the {crop}x{crop} crop")
    return rh, rw, (rh - crop) // 2, (rw - crop) // 2


_TABLE_CACHE = {}


def _device_tables(key, device):
    """key = (in_size, out_size, filter, box, window): the axis tables resident on `device`, built once per shape."""
    dev = torch.device(device)
    hit = _TABLE_CACHE.get((key, dev))
    if hit is None:
        t = resample_tables(*key)
        if t.taps > MAX_TAPS:
            raise hip.RcdmError(f"resample {key[0]} -> {key[1]} ({key[2]}) needs {t.taps} taps; rcdm_image_resample takes <= {MAX_TAPS}")
        hit = types.SimpleNamespace(k=torch.from_numpy(t.k).to(dev), bounds=torch.from_numpy(t.bounds).to(dev), taps=t.taps,
                                    tile_rows=tile_rows(t.bounds), count=len(t.bounds))
        _TABLE_CACHE[(key, dev)] = hit
    return hit


def _default_device():
    if not torch.cuda.is_available():
        raise hip.RcdmError("rcdms_amd.image runs on the HIP path only: no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _one_hwc(im):
    if isinstance(im, torch.Tensor):
        return im
    a = np.asarray(im)                                   # numpy array or PIL image
    if not a.flags.writeable:                            # a PIL image's buffer: torch wants memory it may write
        a = a.copy()
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, axis=2)
    return torch.from_numpy(np.ascontiguousarray(a))


def to_device_frames(images, device=None):
    """numpy uint8 HWC array(s), PIL image(s) or uint8 tensors -> list of device uint8 tensors (n, H, W, 3), equal sizes
    batched together in order.  A device tensor is used where it lies when its pixels are dense (stride 3 between pixels,
    1 between channels): any row pitch and image stride — a frame sliced out of a strip — goes to the kernel as it is."""
    device = _default_device() if device is None else torch.device(device)
    if isinstance(images, (list, tuple)):
        items = [_one_hwc(im) for im in images]
    else:
        items = [_one_hwc(images)]
    groups = []
    for t in items:
        if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise ValueError(f"frames are uint8 (H, W, 3) or (n, H, W, 3), got {t.dtype} {tuple(t.shape)}")
        t = t if t.dim() == 4 else t.unsqueeze(0)
        if groups and isinstance(groups[-1], list) and groups[-1][0].shape[1:] == t.shape[1:] and not t.is_cuda:
            groups[-1].append(t)
        elif t.is_cuda:
            groups.append(t)
        else:
            groups.append([t])
    out = []
    for g in groups:
        t = torch.cat(g).to(device, non_blocking=False) if isinstance(g, list) else g.to(device)
        if t.stride(3) != 1 or t.stride(2) != 3 or t.stride(1) < 3 * t.shape[2] or (t.shape[0] > 1 and t.stride(0) < 0):
            t = t.contiguous()
        out.append(t)
    return out


class Resampler:
    """One resample geometry (in_h x in_w -> resize -> window) on one device: the four cached tables and the descriptor."""

    def __init__(self, in_h, in_w, out_h, out_w, filter, window=None, device=None):
        self.device = _default_device() if device is None else torch.device(device)
        filt = _filter_name(filter)
        top, left, wh, ww = (0, 0, out_h, out_w) if window is None else window
        self.ty = _device_tables((in_h, out_h, filt, None, (top, wh)), self.device)
        self.tx = _device_tables((in_w, out_w, filt, None, (left, ww)), self.device)
        self.in_h, self.in_w, self.out_h, self.out_w = int(in_h), int(in_w), int(wh), int(ww)

    def desc(self, src, mode, flip=False, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dst_pitch=0, dst_stride=0, ld=0, c_pad=0):
        n, h, w, _ = src.shape
        assert (h, w) == (self.in_h, self.in_w) and src.dtype == torch.uint8 and src.is_cuda
        d = hip.ResampleDesc()
        d.src_pitch, d.src_stride = src.stride(1), src.stride(0) if n > 1 else 0
        d.dst_pitch, d.dst_stride = int(dst_pitch), int(dst_stride)
        d.n, d.channels = n, 3
        d.in_h, d.in_w, d.out_h, d.out_w = h, w, self.out_h, self.out_w
        d.taps_x, d.taps_y, d.tile_rows = self.tx.taps, self.ty.taps, self.ty.tile_rows
        d.flip_channels, d.mode, d.ld, d.c_pad = int(bool(flip)), mode, int(ld), int(c_pad)
        d.mean[:], d.std[:] = [float(v) for v in mean], [float(v) for v in std]
        return d

    def launch(self, d, src, dst_ptr):
        hip.image_resample(d, src.data_ptr(), self.tx.k.data_ptr(), self.tx.bounds.data_ptr(), self.ty.k.data_ptr(),
                           self.ty.bounds.data_ptr(), dst_ptr)

    def to_uint8(self, src, flip=False, out=None):
        """-> uint8 (n, out_h, out_w, 3); `out`: a uint8 device tensor of that shape, any row pitch / image stride."""
        n = src.shape[0]
        if out is None:
            out = torch.empty(n, self.out_h, self.out_w, 3, dtype=torch.uint8, device=self.device)
        assert tuple(out.shape) == (n, self.out_h, self.out_w, 3) and out.stride(3) == 1 and out.stride(2) == 3
        self.launch(self.desc(src, hip.IMAGE_U8, flip, dst_pitch=out.stride(1), dst_stride=out.stride(0) if n > 1 else 0), src,
                    out.data_ptr())
        return out

    def to_nchw(self, src, mean, std, flip=False):
        """-> fp32 (n, 3, out_h, out_w): (u8 * (1/255) - mean[c]) * (1 / std[c])."""
        out = torch.empty(src.shape[0], 3, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
        self.launch(self.desc(src, hip.IMAGE_F32_NCHW, flip, mean, std), src, out.data_ptr())
        return out

    def to_rows(self, src, mean, std, dst_ptr, ld, c_pad, flip=False):
        """f16 pixel rows [n * out_h * out_w][ld] at dst_ptr: the value of to_nchw rounded to f16, channels 3..c_pad zero."""
        self.launch(self.desc(src, hip.IMAGE_F16_ROWS, flip, mean, std, ld=ld, c_pad=c_pad), src, dst_ptr)


_RESAMPLERS = {}


def resampler(in_h, in_w, out_h, out_w, filter, window=None, device=None):
    device = _default_device() if device is None else torch.device(device)
    key = (in_h, in_w, out_h, out_w, _filter_name(filter), window, device)
    r = _RESAMPLERS.get(key)
    if r is None:
        r = _RESAMPLERS[key] = Resampler(in_h, in_w, out_h, out_w, filter, window, device)
    return r


class BatchFeature(dict):
    """What the processor returns: `.pixel_values` and `["pixel_values"]`, as transformers' class of this name."""
    __getattr__ = dict.__getitem__


class ClipImageProcessor:
    """transformers' CLIPImageProcessor as the stage-2 driver uses it, on the HIP path:
    `proc(images=frames, return_tensors="pt").pixel_values` -> device fp32 (B, 3, crop, crop).  frames: numpy uint8 HWC
    array(s), PIL image(s) or device uint8 tensors.  The driver hands it cv2's BGR arrays unflipped, so the CLIP mean / std
    meet the channels in that order: flip_channels=False keeps that quirk, True swaps channels 0 and 2 first."""

    def __init__(self, size=224, crop_size=224, resample="bicubic", image_mean=CLIP_MEAN, image_std=CLIP_STD,
                 flip_channels=False, device=None):
        size = size["shortest_edge"] if isinstance(size, dict) else size
        crop_size = crop_size["height"] if isinstance(crop_size, dict) else crop_size
        self.size, self.crop_size, self.resample = int(size), int(crop_size), _filter_name(resample)
        self.image_mean, self.image_std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
        self.flip_channels, self.device = bool(flip_channels), device

    def _resampler(self, h, w, device):
        rh, rw, top, left = clip_geometry(h, w, self.size, self.crop_size)
        return resampler(h, w, rh, rw, self.resample, (top, left, self.crop_size, self.crop_size), device)

    def cropped_uint8(self, images):
        """The resized and cropped bytes (B, crop, crop, 3) — what Pillow produces before the rescale."""
        outs = [self._resampler(t.shape[1], t.shape[2], t.device).to_uint8(t, self.flip_channels)
                for t in to_device_frames(images, self.device)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def preprocess(self, images, return_tensors="pt", **_):
        if return_tensors not in ("pt", None):
            raise ValueError("return_tensors='pt': the pixel values stay on the device")
        outs = [self._resampler(t.shape[1], t.shape[2], t.device).to_nchw(t, self.image_mean, self.image_std, self.flip_channels)
                for t in to_device_frames(images, self.device)]
        return BatchFeature(pixel_values=outs[0] if len(outs) == 1 else torch.cat(outs))

    def __call__(self, images=None, return_tensors="pt", **kw):
        return self.preprocess(images, return_tensors=return_tensors, **kw)


class FrameTransform:
    """The driver's img_augment (ToPILImage -> Resize([height, width]) -> ToTensor -> Normalize(0.5, 0.5)):
    `ft(frames)` -> device fp32 (n, 3, height, width) in [-1, 1].  `ft(frames, rows=True, out=rows)` writes the same
    values rounded to f16 as channels-last pixel rows into `out` (a plan.Rows: ptr, ld, C — VaeEncodeProgram.x_in), pad
    channels zeroed, and returns `out`."""
    MEAN = STD = (0.5, 0.5, 0.5)

    def __init__(self, height, width, resample="bilinear", flip_channels=False, device=None):
        self.height, self.width, self.resample = int(height), int(width), _filter_name(resample)
        self.flip_channels, self.device = bool(flip_channels), device

    def __call__(self, frames, rows=False, out=None):
        groups = to_device_frames(frames, self.device)
        if rows:
            if out is None or len(groups) != 1:
                raise ValueError("rows=True writes one batch of equally sized frames into `out` (a plan.Rows)")
            t = groups[0]
            if out.M != t.shape[0] * self.height * self.width or out.C % 8 or out.C < 8:
                raise ValueError(f"`out` holds {out.M} rows of {out.C} channels; {t.shape[0]} frames of {self.height}x{self.width} "
                                 "need one row per pixel and a channel count that is a multiple of 8")
            resampler(t.shape[1], t.shape[2], self.height, self.width, self.resample, None, t.device).to_rows(
                t, self.MEAN, self.STD, out.ptr, out.ld, out.C, self.flip_channels)
            return out
        outs = [resampler(t.shape[1], t.shape[2], self.height, self.width, self.resample, None, t.device).to_nchw(
            t, self.MEAN, self.STD, self.flip_channels) for t in groups]
        return outs[0] if len(outs) == 1 else torch.cat(outs)


def frames_to_uint8(x, out=None):
    """uint8 frames of decoder output: trunc(clamp(x / 2 + 0.5, 0, 1) * 255), NaN -> 0.
    x: a device fp32 tensor (n, 3, H, W) — or (b, 3, f, H, W), frames then come out as (b, f, H, W, 3) — or
    (rows, n, H, W) with rows a plan.Rows of f16 channels-last pixels (VaeDecodeProgram.out_rows).
    out: a device uint8 tensor (n, H, W, 3) with dense pixels and any row pitch / image stride (e.g. the cells of one row
    of a grid image); default a new dense one."""
    lib_kind, lead = None, None
    if isinstance(x, tuple):
        rows, n, H, W = x
        src_ptr, ld, lib_kind, device = rows.ptr, rows.ld, hip.FRAMES_F16_ROWS, rows.buf.t.device
        if rows.M != n * H * W or rows.C < 3:
            raise ValueError(f"{rows.M} rows of {rows.C} channels are not {n} frames of {H}x{W} pixels")
        keep = None
    else:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise hip.RcdmError("frames_to_uint8 runs on the HIP path only: x must be a device tensor")
        if x.dim() == 5:
            lead = (x.shape[0], x.shape[2])
            x = x.permute(0, 2, 1, 3, 4).reshape(-1, x.shape[1], *x.shape[3:])
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"x {tuple(x.shape)}: expected (n, 3, H, W) or (b, 3, f, H, W)")
        keep = x.detach().to(torch.float32).contiguous()
        n, _, H, W = keep.shape
        src_ptr, ld, lib_kind, device = keep.data_ptr(), 0, hip.FRAMES_F32_NCHW, keep.device
    if out is None:
        out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=device)
    if (out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or out.stride(3) != 1 or out.stride(2) != 3 or
            out.stride(1) < 3 * W or not out.is_cuda):
        raise ValueError(f"out must be device uint8 ({n}, {H}, {W}, 3) with dense pixels")
    d = hip.FramesU8Desc(out.stride(1), out.stride(0) if n > 1 else 0, n, H, W, 3, lib_kind, ld)
    hip.frames_to_u8(d, src_ptr, out.data_ptr())
    if keep is not None:
        keep.record_stream(torch.cuda.current_stream(device))
    return out.view(*lead, H, W, 3) if lead is not None and out.is_contiguous() else out


# ------------------------------------------------------------------------------------------------
# PNG files of uint8 frames (rcdm_png_encode): what the driver's PIL.Image.save calls write, encoded on the device
PNG_FILTERS = {"adaptive": hip.PNG_ADAPTIVE, "none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}


def _png_filter(f):
    v = PNG_FILTERS.get(f.lower()) if isinstance(f, str) else (int(f) if isinstance(f, int) and not isinstance(f, bool) else None)
    if v is None or not -1 <= v <= 4:
        raise ValueError(f"png filter {f!r}: one of {sorted(PNG_FILTERS)} or -1..4")
    return v


def _png_frames(frames):
    """-> the (n, h, w, 3) device uint8 view the kernel reads (dense pixels, any row pitch / image stride)."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"PNG frames are a device uint8 tensor, got {type(frames).__name__}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"PNG frames are uint8, got {frames.dtype}: convert with frames_to_uint8 first")
    if frames.dim() not in (3, 4) or frames.shape[-1] != 3 or 0 in frames.shape:
        raise ValueError(f"PNG frames are (h, w, 3) or (n, h, w, 3), got {tuple(frames.shape)}")
    if not frames.is_cuda:
        raise hip.RcdmError("encode_png runs on the HIP path only: frames must be a device tensor (there is no CPU encoder here)")
    t = frames if frames.dim() == 4 else frames.unsqueeze(0)
    n, h, w, _ = t.shape                                 # the stride of a dimension of size 1 addresses nothing: any value goes
    if t.stride(3) != 1 or (w > 1 and t.stride(2) != 3) or (h > 1 and t.stride(1) < 3 * w) or (n > 1 and t.stride(0) < 0):
        t = t.contiguous()
    return t


def _png_device(device):
    """`device` with its index spelled out ("cuda" -> the current device), so that it compares equal to a tensor's."""
    if device is None:
        return _default_device()
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class PngEncoder:
    """n images of h x w on one device: the descriptor's geometry, the workspace, the output streams (+ their sizes behind
    them, so one download brings both) and a pinned host buffer of the same size, kept for every call of this shape.
    match=True: rcdm_png_encode_match (matches at the PNG row distances, per-block fallback to the literal form)."""

    def __init__(self, h, w, n=1, device=None, match=False):
        self.device = _png_device(device)
        self.h, self.w, self.n, self.match = int(h), int(w), int(n), bool(match)
        d = self._desc(3 * self.w, 0, 0, hip.PNG_ADAPTIVE)
        self.bound = hip.png_bound(d)
        if self.bound == 0:
            raise hip.RcdmError(f"rcdm_png_encode takes 1..65535 images with sides 1..8192, got {self.n} of {self.h}x{self.w}")
        self.stride = (self.bound + 15) & ~15
        self.workspace = torch.empty((hip.png_match_workspace_bytes if self.match else hip.png_workspace_bytes)(d), dtype=torch.uint8,
                                     device=self.device)
        self.out = torch.empty(self.n * self.stride + 8 * self.n, dtype=torch.uint8, device=self.device)
        self.host = torch.empty(self.out.shape, dtype=torch.uint8, pin_memory=True)

    def _desc(self, pitch, src_stride, dst_stride, filt):
        return hip.PngDesc(pitch, src_stride, dst_stride, self.n, self.h, self.w, 3, filt)

    def launch(self, frames, filter="adaptive", dst=None, dst_stride=None, sizes=None):
        """The launch sequence alone (graph-capturable): files at dst + i * dst_stride, sizes[i] (uint64) on the device.
        Default destination: this encoder's own buffer."""
        t = _png_frames(frames)
        if tuple(t.shape) != (self.n, self.h, self.w, 3) or t.device != self.device:
            raise ValueError(f"this encoder takes ({self.n}, {self.h}, {self.w}, 3) on {self.device}, got {tuple(t.shape)} on {t.device}")
        dst_ptr = self.out.data_ptr() if dst is None else dst
        stride = self.stride if dst_stride is None else int(dst_stride)
        sizes_ptr = self.out.data_ptr() + self.n * self.stride if sizes is None else sizes
        d = self._desc(t.stride(1) if self.h > 1 else 3 * self.w, t.stride(0) if self.n > 1 else 0, stride if self.n > 1 else 0,
                       _png_filter(filter))
        (hip.png_encode_match if self.match else hip.png_encode)(d, t.data_ptr(), self.workspace.data_ptr(), dst_ptr, sizes_ptr)
        return t

    def encode(self, frames, filter="adaptive"):
        """-> list of n `bytes`: one launch sequence, one download, a slice per file."""
        keep = self.launch(frames, filter)
        self.host.copy_(self.out, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        del keep
        raw = self.host.numpy()
        sizes = raw[self.n * self.stride:].view(np.uint64)
        out = []
        for i in range(self.n):
            size = int(sizes[i])
            if not 57 <= size <= self.bound:
                raise hip.RcdmError(f"rcdm_png_encode reported {size} bytes for image {i} (bound {self.bound})")
            out.append(raw[i * self.stride:i * self.stride + size].tobytes())
        return out


_PNG_ENCODERS = {}


def png_encoder(h, w, n=1, device=None, match=False):
    device = _png_device(device)
    key = (int(h), int(w), int(n), device, bool(match))
    e = _PNG_ENCODERS.get(key)
    if e is None:
        e = _PNG_ENCODERS[key] = PngEncoder(h, w, n, device, match)
    return e


def encode_png(frames, filter="adaptive", match=False):
    """Device uint8 frames (n, h, w, 3) or (h, w, 3), dense pixels with any row pitch / image stride -> list of PNG files as
    `bytes`.  Literal-only deflate (see include/rcdm.h, "PNG"): about Pillow's default size on noisy decoder output, far
    larger than Pillow's on flat images.  filter: "adaptive" (per row) or one of none / sub / up / average / paeth.
    match=True: the match mode (rcdm_png_encode_match) — the same pixels, no block larger, flat frames several times smaller."""
    _png_filter(filter)
    t = _png_frames(frames)
    return png_encoder(t.shape[1], t.shape[2], t.shape[0], t.device, match).encode(t, filter)


def save_png(paths, frames, filter="adaptive", match=False):
    """Write frames[i] to paths[i] (a single path for a single (h, w, 3) frame)."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    files = encode_png(frames, filter, match)
    if len(files) != len(paths):
        raise ValueError(f"{len(paths)} paths for {len(files)} frames")
    for p, b in zip(paths, files):
        with open(p, "wb") as f:
            f.write(b)


# ------------------------------------------------------------------------------------------------
# PNG files -> uint8 frames on the device (rcdm_png_decode): the container is walked here, the bulk is the device's
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_ORDERS = {"rgb": hip.PNG_RGB, "bgr": hip.PNG_BGR}
_PNG_BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_PNG_MAX_SIDE = 8192


def png_walk(data, index=0, check_crc=False):
    """The chunk headers of one file (8 bytes per chunk; the payloads are not touched unless check_crc) ->
    SimpleNamespace(w, h, color_type, idats [(payload offset, bytes)], plte (offset, entries)).  Ancillary chunks are
    skipped, tRNS included (what Image.convert("RGB") and cv2.IMREAD_COLOR make of them).  NotImplementedError, naming the
    file index, for what rcdm_png_decode does not read: a bit depth other than 8, Adam7, a side above 8192, a missing IHDR /
    IDAT / PLTE; ValueError for what is not a PNG container at all (signature, a chunk that runs past the end, a CRC)."""
    data = memoryview(data)
    if len(data) < 8 or bytes(data[:8]) != PNG_SIGNATURE:
        raise ValueError(f"file {index}: not a PNG signature")
    out = types.SimpleNamespace(w=None, h=None, color_type=None, idats=[], plte=None)
    off = 8
    while off + 12 <= len(data):
        n, = struct.unpack(">I", data[off:off + 4])
        kind = bytes(data[off + 4:off + 8])
        if off + 12 + n > len(data):
            raise ValueError(f"file {index}: a {kind!r} chunk of {n} bytes runs past the end of the file")
        if check_crc:
            stored, = struct.unpack(">I", data[off + 8 + n:off + 12 + n])
            if stored != zlib.crc32(data[off + 4:off + 8 + n]) & 0xFFFFFFFF:
                raise ValueError(f"file {index}: CRC of the {kind!r} chunk at byte {off}")
        if kind == b"IHDR":
            if n != 13:
                raise ValueError(f"file {index}: an IHDR of {n} bytes")
            w, h, depth, ct, comp, filt, interlace = struct.unpack(">IIBBBBB", data[off + 8:off + 21])
            if depth != 8 or ct not in _PNG_BPP:
                raise NotImplementedError(f"file {index}: bit depth {depth}, colour type {ct}: rcdm_png_decode reads 8-bit grey, "
                                          "RGB, palette, grey + alpha and RGBA")
            if interlace:
                raise NotImplementedError(f"file {index}: Adam7 interlacing is not read")
            if comp or filt:
                raise NotImplementedError(f"file {index}: compression method {comp}, filter method {filt}")
            if not (1 <= w <= _PNG_MAX_SIDE and 1 <= h <= _PNG_MAX_SIDE):
                raise NotImplementedError(f"file {index}: {h}x{w}: sides are 1..{_PNG_MAX_SIDE}")
            out.w, out.h, out.color_type = w, h, ct
        elif kind == b"PLTE":
            out.plte = (off + 8, min(n // 3, 256))
        elif kind == b"IDAT":
            out.idats.append((off + 8, n))
        elif kind == b"IEND":                            # a missing IEND is let pass, as Pillow and cv2 do
            break
        off += 12 + n
    if out.w is None:
        raise NotImplementedError(f"file {index}: no IHDR chunk")
    if not out.idats or sum(n for _, n in out.idats) == 0:
        raise NotImplementedError(f"file {index}: no IDAT data")
    if out.color_type == 3 and out.plte is None:
        raise NotImplementedError(f"file {index}: colour type 3 without a PLTE chunk")
    return out


def _png_files(files):
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    files = list(files)
    if not files or not all(isinstance(f, (bytes, bytearray, memoryview)) for f in files):
        raise TypeError("PNG files are one bytes object or a non-empty sequence of them")
    if len(files) > 65535:
        raise ValueError(f"rcdm_png_decode takes 1..65535 files per call, got {len(files)}")
    return files


def png_decode_plan(files, check_crc=False, pitch=None, gap=0):
    """Host side of one rcdm_png_decode call: walks every file and lays out the buffers ->
    SimpleNamespace(n, n_idat, records (hip.PngFile * n), idats (hip.PngIdat * n_idat), src uint8 numpy (the files, each at
    a 16-byte boundary), dst_bytes, workspace_bytes, shapes [(h, w)]).  pitch(w) -> bytes between output rows (default
    dense, 3 w); gap: bytes left free in front of every image (both for tests that guard the output)."""
    files = _png_files(files)
    walks = [png_walk(f, i, check_crc) for i, f in enumerate(files)]
    n, n_idat = len(files), sum(len(wk.idats) for wk in walks)
    records, idats = (hip.PngFile * n)(), (hip.PngIdat * n_idat)()
    src_at, dst_at, ws_at, idat_at = 0, 0, 0, 0
    for i, (f, wk) in enumerate(zip(files, walks)):
        r = records[i]
        r.src_offset, r.src_bytes = src_at, len(f)
        src_at += (len(f) + 15) & ~15
        r.w, r.h, r.color_type = wk.w, wk.h, wk.color_type
        r.dst_pitch = 3 * wk.w if pitch is None else int(pitch(wk.w))
        dst_at += gap
        r.dst_offset = dst_at
        dst_at += r.dst_pitch * wk.h
        r.idat_first, r.idat_count = idat_at, len(wk.idats)
        for off, nb in wk.idats:
            idats[idat_at].offset, idats[idat_at].bytes = off, nb
            idat_at += 1
        r.zlib_bytes = sum(nb for _, nb in wk.idats)
        r.ws_offset = ws_at
        ws_at += hip.png_file_workspace(r.zlib_bytes, wk.h * (1 + _PNG_BPP[wk.color_type] * wk.w))
        r.plte_offset, r.plte_entries = wk.plte if wk.plte is not None and wk.color_type == 3 else (0, 0)
    src = np.zeros(src_at, dtype=np.uint8)
    for r, f in zip(records, files):
        src[r.src_offset:r.src_offset + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return types.SimpleNamespace(n=n, n_idat=n_idat, records=records, idats=idats, src=src, dst_bytes=dst_at + gap, workspace_bytes=ws_at,
                                 shapes=[(wk.h, wk.w) for wk in walks])


class PngDecoder:
    """rcdm_png_decode on one device: `decode(files)` is one upload of the file bytes, one of the tables, one launch
    sequence (inflate, unfilter + convert; `launch` alone is graph-capturable) and one download of n status words."""

    def __init__(self, device=None):
        self.device = _png_device(device)
        if self.device.type != "cuda":
            raise hip.RcdmError("decode_png runs on the HIP path only: there is no CPU decoder here")

    def upload(self, plan):
        """-> (src, tables) on the device; tables: the records, then the IDAT table (both 8-byte aligned)."""
        rec = np.frombuffer(bytes(plan.records), dtype=np.uint8)
        tab = np.concatenate([rec, np.frombuffer(bytes(plan.idats), dtype=np.uint8)])
        assert ctypes.sizeof(hip.PngFile) % 8 == 0
        return torch.from_numpy(plan.src).to(self.device), torch.from_numpy(tab).to(self.device)

    def launch(self, plan, src, tables, workspace, dst, status, order="rgb"):
        """The two launches on the current stream.  workspace / dst: device uint8 tensors of at least plan.workspace_bytes /
        plan.dst_bytes; status: device int32 [n]."""
        if order not in PNG_ORDERS:
            raise ValueError(f"order {order!r}: rgb or bgr")
        if workspace.numel() < plan.workspace_bytes or dst.numel() < plan.dst_bytes or status.numel() < plan.n:
            raise ValueError("workspace, dst or status is smaller than the plan asks for")
        hip.png_decode(tables.data_ptr(), tables.data_ptr() + plan.n * ctypes.sizeof(hip.PngFile), plan.n, plan.n_idat, PNG_ORDERS[order],
                       src.data_ptr(), workspace.data_ptr(), dst.data_ptr(), status.data_ptr())

    def decode(self, files, order="rgb", check_crc=False):
        """-> list of n device uint8 (h, w, 3) tensors: views of ONE buffer with dense rows, in order (`PngDecoder.batch` views
        a run of equal sizes as (n, h, w, 3) without a copy)."""
        plan = png_decode_plan(files, check_crc)
        if hip.png_decode_workspace_bytes(plan.records, plan.n) != plan.workspace_bytes:
            raise hip.RcdmError("rcdm_png_decode_workspace_bytes disagrees with the host's layout")
        src, tables = self.upload(plan)
        workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=self.device)
        dst = torch.empty(plan.dst_bytes, dtype=torch.uint8, device=self.device)
        status = torch.empty(plan.n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self.launch(plan, src, tables, workspace, dst, status, order)
        bad = status.cpu().numpy()                        # the one download; it also orders the buffers' release
        for i in np.flatnonzero(bad):
            raise hip.RcdmError(f"rcdm_png_decode: file {int(i)}: {hip.PNG_STATUS.get(int(bad[i]), int(bad[i]))}")
        out, at = [], 0
        for h, w in plan.shapes:
            out.append(dst[at:at + h * w * 3].view(h, w, 3))
            at += h * w * 3
        return out

    @staticmethod
    def batch(frames):
        """Equally sized frames of one decode call as the (n, h, w, 3) view of their shared buffer (no copy)."""
        h, w, _ = frames[0].shape
        if any(tuple(f.shape) != (h, w, 3) for f in frames):
            raise ValueError("the frames differ in size")
        return frames[0].as_strided((len(frames), h, w, 3), (h * w * 3, w * 3, 3, 1))


_PNG_DECODERS = {}


def png_decoder(device=None):
    device = _png_device(device)
    d = _PNG_DECODERS.get(device)
    if d is None:
        d = _PNG_DECODERS[device] = PngDecoder(device)
    return d


def decode_png(files, order="rgb", check_crc=False, device=None):
    """PNG files (one `bytes` or a sequence) -> list of device uint8 (h, w, 3) frames, views of one buffer with dense rows.
    order="bgr": cv2.imdecode's channel order, which the drivers hand unflipped to everything downstream.  check_crc: verify
    every chunk's CRC-32 on the host first (zlib.crc32); the Adler-32 of the pixel stream is always checked on the device.
    A file the device refuses raises hip.RcdmError naming the file index and the RCDM_PNG_E* code; one out of scope (bit
    depth, Adam7, missing chunks) NotImplementedError.  There is no CPU path: without a GPU it raises."""
    files = _png_files(files)
    return png_decoder(device).decode(files, order, check_crc)


def load_png(paths, order="rgb", check_crc=False, device=None):
    """decode_png of the files at `paths` (a single path gives a list of one frame)."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    files = []
    for p in paths:
        with open(p, "rb") as f:
            files.append(f.read())
    return decode_png(files, order, check_crc, device)
