"""Numpy restatement of the 8-bit image paths (the reference's PIL / torchvision / transformers preprocessing and its
uint8 truncation), written as plain loops from the published arithmetic of Pillow's ImagingResample, independently of
rcdms_amd/image.py's vectorised tables:

  coeffs            per-axis coefficient rows in double (precompute_coeffs) and their 22-bit integers (normalize_coeffs_8bpc)
  resize            Image.resize for uint8 HWC arrays: horizontal pass first, rounded to uint8, vertical pass over it; a pass
                    is skipped when its axis keeps its size and no box is given
  clip_geometry     transformers' shortest-edge size + centre-crop offsets
  clip_pixel_values CLIPImageProcessor on uint8 arrays: the cropped bytes and (u8 / 255 - mean) / std in float64
  frames_u8         (x / 2 + 0.5).clamp(0, 1) * 255 truncated, in fp32, as the pipeline + driver compute it

tests/test_image_host.py pins this file to Pillow itself (live, when it imports) and to the goldens minted from it."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0}
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTER = {"bilinear": _bilinear, "bicubic": _bicubic}


def coeffs(in_size, out_size, filt, box=None):
    """-> (k int32 [out_size][taps], bounds int32 [out_size][2] = (first, count), taps) for one axis."""
    in0, in1 = (0.0, float(in_size)) if box is None else (float(box[0]), float(box[1]))
    f = FILTER[filt]
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filt] * filterscale
    taps = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, taps), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds, taps


def _pass(img, k, bounds, axis):
    """One pass along `axis` (0 rows, 1 columns) of a uint8 HWC array."""
    src = img.astype(np.int64)
    shape = list(img.shape)
    shape[axis] = k.shape[0]
    out = np.empty(shape, dtype=np.uint8)
    for o in range(k.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = 1 << (PRECISION_BITS - 1)
        if axis == 1:
            acc = acc + (src[:, lo:lo + n, :] * k[o, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        else:
            acc = acc + (src[lo:lo + n] * k[o, :n].astype(np.int64)[:, None, None]).sum(axis=0)
        assert np.abs(acc).max() < 2 ** 31                       # Pillow accumulates in a C int
        v = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        if axis == 1:
            out[:, o, :] = v
        else:
            out[o] = v
    return out


def resize(img, size, filt, box=None):
    """PIL.Image.fromarray(img).resize(size, filt, box): img uint8 (H, W, C), size (width, height), box (x0, y0, x1, y1)."""
    h, w = img.shape[:2]
    ow, oh = size
    bx = None if box is None else (box[0], box[2])
    by = None if box is None else (box[1], box[3])
    out = img
    if ow != w or (bx is not None and (bx[0] != 0 or bx[1] != w)):
        k, b, _ = coeffs(w, ow, filt, bx)
        out = _pass(out, k, b, 1)
    if oh != h or (by is not None and (by[0] != 0 or by[1] != h)):
        k, b, _ = coeffs(h, oh, filt, by)
        out = _pass(out, k, b, 0)
    return np.ascontiguousarray(out)


def clip_geometry(h, w, size, crop):
    """-> (resized_h, resized_w, top, left): shortest edge to `size` keeping the aspect ratio (the long side truncated),
    then a centred crop x crop window."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    rh, rw = (new_long, new_short) if w <= h else (new_short, new_long)
    return rh, rw, (rh - crop) // 2, (rw - crop) // 2


def clip_pixel_values(img, size=224, crop=224, filt="bicubic", mean=CLIP_MEAN, std=CLIP_STD):
    """-> (cropped uint8 (crop, crop, 3), float64 (3, crop, crop))."""
    rh, rw, top, left = clip_geometry(img.shape[0], img.shape[1], size, crop)
    u8 = np.ascontiguousarray(resize(img, (rw, rh), filt)[top:top + crop, left:left + crop])
    return u8, normalize(u8, mean, std)


def normalize(u8, mean, std):
    """(u8 / 255 - mean) / std in float64, HWC -> CHW."""
    x = u8.astype(np.float64) / 255.0
    x = (x - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


def normalize_f32(u8, mean, std):
    """The kernel's own fp32 sequence, (u8 * (1/255) - mean) * (1/std) with every step and both constants rounded to fp32
    (HWC -> CHW): what modes RCDM_IMAGE_F32_NCHW / _F16_ROWS store, bit for bit."""
    f = np.float32
    x = u8.astype(f) * (f(1) / f(255))
    x = (x - np.asarray(mean, dtype=f)) * (f(1) / np.asarray(std, dtype=f))
    assert x.dtype == f
    return np.ascontiguousarray(np.moveaxis(x, -1, -3))


def frames_u8(x):
    """x fp32 array in about [-1, 1] -> uint8, the pipeline's (x / 2 + 0.5).clamp(0, 1) then the driver's (* 255).astype(uint8)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        y = np.clip(x / np.float32(2) + np.float32(0.5), np.float32(0), np.float32(1)) * np.float32(255)
        return np.where(np.isnan(y), np.float32(0), y).astype(np.uint8)


def test_image(h, w, seed):
    """Seeded noise with a saturated quadrant (0 / 255 checkerboard blocks): bicubic overshoot reaches the clip on both sides."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    qh, qw = h // 2, w // 2
    yy, xx = np.mgrid[0:qh, 0:qw]
    img[:qh, :qw] = (((yy // 3 + xx // 3) & 1) * 255).astype(np.uint8)[:, :, None]
    return img


test_image.__test__ = False
