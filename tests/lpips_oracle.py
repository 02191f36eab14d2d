"""The oracle of the LPIPS path (rcdms_amd/lpips.py, csrc/lpips.hip), restated from Zhang et al. 2018 and the published forward
of the lpips package (v0.1: ScalingLayer, tower taps, normalize_tensor with the epsilon after the root, non-negative 1 x 1 lin
layers, spatial mean, sum over the taps).  Nothing here is pinned against the package itself.

  head_f64        the distance of one tap from the definition, in float64 on the f16 features
  head_model      the numpy model of csrc/lpips_core.h: the same fp32 operations in the same order, then the float64 tile tree
                  and the fixed sum over the tile partials — the bits the device and tools/lpips_host.cpp must give
  head_bound      the a-priori bound on |head_model - head_f64|, derived below from the operation counts
  input_rows      the rows rcdm_lpips_input_rows writes, from exact rational arithmetic (one fma rounding, one f16 rounding)
  tower           the fp32 towers through torch.nn.functional on the CPU in their natural form (AlexNet's stem as the direct
                  11 x 11 stride-4 conv), and the f16 model: weights rounded once, every layer output rounded to f16
  synthetic_state_dict   seeded full-width weights, He-scaled so that the activations stay O(1) to the last tap

The bound.  u = 2^-24 (fp32), U = 2^-53 (float64), L = lanes(C), k = 8 + log2 L the depth of a channel sum (8 in a lane, log2 L
in the group tree; the first addition, to +0.0, is exact, the product adds one rounding, so a sum of non-negative terms carries a
relative error of at most k u).
  S = sum a_c^2:        |S^ - S| <= k u S
  na = sqrt(S) + eps:   the root halves the relative error and adds u, the addition adds u, and fp32(1e-10) differs from 1e-10
                        by less than u eps <= u na:           |na^ - na| <= (k / 2 + 3) u na =: dn na
  x_c = a_c / na:       |x^ - x| <= (dn + u) |x|, likewise y_c = b_c / nb
  d_c = x_c - y_c:      |d^ - d| <= (dn + u)(|x| + |y|) + u |d|
  t_c = lin_c (d d):    |t^ - t| <= lin_c (2 |d| |d^ - d| + 2 u d^2)            (the square and the product by lin, one u each)
  v = sum t_c:          |v^ - v| <= sum_c |t^ - t| + k u v
so  E_pixel = sum_c lin_c (2 |d| (dn + u)(|x| + |y|) + (4 + k) u d^2),  evaluated in float64 on the exact x, y, d, times 1.01
for the second-order terms, plus 64 C 2^-149 max(lin, 1) for results of single operations that fall below the fp32 normal range.
The pixel values are widened exactly; the float64 sums add at most chain(hw) U of the mean, the division one more.
  bound = mean(E_pixel) 1.01 + (chain(hw) + 1) U mean(v) + 64 C 2^-149 max(lin, 1)."""
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from rcdms_amd import lpips as L

U32, U64 = 2.0 ** -24, 2.0 ** -53
TILE, LANES, CHUNK = 64, 256, 8
EPS = 1e-10
EPS32 = np.float32(1e-10)


def lanes(c):
    n = 1
    while n * CHUNK < c:
        n <<= 1
    return n


def tiles(hw):
    return (hw + TILE - 1) // TILE


def chain(hw):
    return 6 + (tiles(hw) + LANES - 1) // LANES + 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------ the head
def pixel_values_f64(a, b, lin, eps_inside_root=False):
    """a, b: (..., C) f16 -> the per-pixel value in float64 from the definition."""
    a, b, lin = a.astype(np.float64), b.astype(np.float64), np.asarray(lin, np.float64)
    if eps_inside_root:
        na, nb = np.sqrt((a * a).sum(-1) + EPS), np.sqrt((b * b).sum(-1) + EPS)
    else:
        na, nb = np.sqrt((a * a).sum(-1)) + EPS, np.sqrt((b * b).sum(-1)) + EPS
    d = a / na[..., None] - b / nb[..., None]
    return (lin * d * d).sum(-1)


def head_f64(a, b, lin, **kw):
    """a, b: (P, hw, C) f16; lin (C,) -> (P,) float64: the mean over the pixels of sum_c lin_c (a_c / na - b_c / nb)^2."""
    return pixel_values_f64(a, b, lin, **kw).mean(-1)


def _tree(part):
    """part (..., n), n a power of two: part[t] += part[t + s], s = n / 2 .. 1 -> (...)."""
    part = part.copy()
    s = part.shape[-1] // 2
    while s > 0:
        part[..., :s] = part[..., :s] + part[..., s:2 * s]
        s //= 2
    return part[..., 0]


def _lanes_view(x, c):
    """(N, C) f16 -> (N, L, 8) float32, zeros for the lanes past the channels."""
    n, Ln = x.shape[0], lanes(c)
    out = np.zeros((n, Ln * CHUNK), np.float32)
    out[:, :c] = x.astype(np.float32)
    return out.reshape(n, Ln, CHUNK)


def pixel_values_model(a, b, lin):
    """a, b: (N, C) f16 -> (N,) float32 with lpips_core.h's operations in its order."""
    c = a.shape[1]
    fa, fb = _lanes_view(a, c), _lanes_view(b, c)
    w = np.zeros(fa.shape[1] * CHUNK, np.float32)
    w[:c] = np.asarray(lin, np.float32)
    w = w.reshape(1, -1, CHUNK)

    def sumsq(v):
        s = np.zeros(v.shape[:2], np.float32)
        for e in range(CHUNK):
            s = s + v[..., e] * v[..., e]
        return _tree(s)
    na = (np.sqrt(sumsq(fa)) + EPS32)[:, None]
    nb = (np.sqrt(sumsq(fb)) + EPS32)[:, None]
    s = np.zeros(fa.shape[:2], np.float32)
    for e in range(CHUNK):
        d = fa[..., e] / na - fb[..., e] / nb
        s = s + w[..., e] * (d * d)
    out = _tree(s)
    assert out.dtype == np.float32
    return out


def fixed_sum(values):
    """fr's fixed sum of a float64 vector: 256 strided partial sums in ascending order from +0.0, then the tree."""
    v = np.zeros(((len(values) + LANES - 1) // LANES) * LANES, np.float64)
    v[:len(values)] = values
    part = np.zeros(LANES, np.float64)
    for row in v.reshape(-1, LANES):
        part = part + row
    return _tree(part)


def head_model(a, b, lin):
    """a, b: (P, hw, C) f16 -> (P,) float64, the bits rcdm_lpips_head and tools/lpips_host.cpp give."""
    P, hw, c = a.shape
    out = np.zeros(P, np.float64)
    for p in range(P):
        v = np.zeros(tiles(hw) * TILE, np.float64)
        v[:hw] = pixel_values_model(a[p], b[p], lin).astype(np.float64)
        out[p] = fixed_sum(_tree(v.reshape(-1, TILE))) / np.float64(hw)
    return out


def head_bound(a, b, lin):
    """(P,) float64: the a-priori bound on |head_model - head_f64| (module docstring)."""
    P, hw, c = a.shape
    lin = np.asarray(lin, np.float64)
    k = 8 + int(np.log2(lanes(c)))
    dn = (k / 2.0 + 3.0) * U32
    fa, fb = a.astype(np.float64), b.astype(np.float64)
    na, nb = np.sqrt((fa * fa).sum(-1)) + EPS, np.sqrt((fb * fb).sum(-1)) + EPS
    x, y = fa / na[..., None], fb / nb[..., None]
    d = x - y
    e_pixel = (lin * (2.0 * np.abs(d) * (dn + U32) * (np.abs(x) + np.abs(y)) + (4.0 + k) * U32 * d * d)).sum(-1)
    tiny = 64.0 * c * 2.0 ** -149 * max(float(lin.max()), 1.0)
    return e_pixel.mean(-1) * 1.01 + (chain(hw) + 1) * U64 * (lin * d * d).sum(-1).mean(-1) + tiny


# ------------------------------------------------------------------------------------------------ the input rows
def _round_f32(q):
    """The fp32 nearest to the rational q, ties to even."""
    c = np.float32(float(q))
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.float32(cand).view(np.int32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return np.float32(best[1])


def input_table(mul, add):
    """(256, 3) f16: f16(fma(fp32(u8 / 255), mul[ch], add[ch])), the fma from exact rational arithmetic."""
    t = np.zeros((256, 3), np.float32)
    for u in range(256):
        x = Fraction(float(np.float32(u) / np.float32(255.0)))
        for ch in range(3):
            t[u, ch] = _round_f32(x * Fraction(float(np.float32(mul[ch]))) + Fraction(float(np.float32(add[ch]))))
    return t.astype(np.float16)


def alex_out_side(n):
    return (n - 7) // 4 + 1


def space_to_depth(x):
    """x (n, H, W, 3), any dtype -> (n, h_out + 2, w_out + 2, 48): Q[n][Y][X][(dy 4 + dx) 3 + ch] = x[n][4 Y + dy - 2][4 X + dx - 2][ch],
    zeros outside the image: the rows over which AlexNet's 11 x 11 stride-4 pad-2 stem is a 3 x 3 stride-1 conv."""
    n, H, W = x.shape[:3]
    qh, qw = alex_out_side(H) + 2, alex_out_side(W) + 2
    z = np.zeros((n, 4 * qh, 4 * qw, 3), x.dtype)
    rh, rw = min(H, 4 * qh - 2), min(W, 4 * qw - 2)
    z[:, 2:2 + rh, 2:2 + rw] = x[:, :rh, :rw]
    return np.ascontiguousarray(z.reshape(n, qh, 4, qw, 4, 3).transpose(0, 1, 3, 2, 4, 5)).reshape(n, qh, qw, 48)


def input_rows(frames, s2d, mul, add):
    """frames (n, H, W, 3) uint8 -> the f16 rows of rcdm_lpips_input_rows: (n, H, W, 8), channels 3 .. 7 zero (s2d = 1), or the
    space-to-depth rows (s2d = 4)."""
    table = input_table(mul, add)
    x = table[frames.astype(np.int64), np.arange(3)]                    # (n, H, W, 3) f16
    if s2d == 4:
        return space_to_depth(x)
    out = np.zeros(x.shape[:3] + (8,), np.float16)
    out[..., :3] = x
    return out


# ------------------------------------------------------------------------------------------------ the towers
def synthetic_state_dict(net, seed=0, prefix="lpips"):
    """Seeded full-width weights under the lpips package's keys (prefix="lpips") or torchvision's (prefix="features")."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, cin, cout, k, _, _, sl in L.CONVS[net]:
        base = f"net.slice{sl}.{i}" if prefix == "lpips" else f"features.{i}"
        sd[f"{base}.weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[f"{base}.bias"] = 0.1 * torch.rand(cout, generator=g)
    for t, c in enumerate(L.TAP_CHANNELS[net]):
        key = f"lin{t}.model.1.weight" if prefix == "lpips" else f"lins.{t}.model.1.weight"
        sd[key] = torch.rand(1, c, 1, 1, generator=g)
    return sd


def _get(sd, names):
    for k in names:
        if k in sd:
            return sd[k]
    raise KeyError(names[0])


def scaled_input(frames, shift=L.SHIFT, scale=L.SCALE):
    """frames (n, H, W, 3) uint8 -> fp32 NCHW, the package's ScalingLayer on 2 x / 255 - 1 in its natural form."""
    x = torch.from_numpy(frames).to(torch.float32).permute(0, 3, 1, 2) / 255.0 * 2.0 - 1.0
    return (x - torch.tensor(shift, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(scale, dtype=torch.float32).view(1, 3, 1, 1)


def tower(sd, net, x, f16=False):
    """x fp32 NCHW (scaled) -> the five post-ReLU taps, fp32 NCHW.  f16: weights rounded once to f16, every layer output
    rounded to f16 (x itself is the caller's: hand it the kernel's rows)."""
    r = (lambda t: t.to(torch.float16).to(torch.float32)) if f16 else (lambda t: t)
    taps = []
    for i, _, _, k, s, p, sl in L.CONVS[net]:
        if i in L.POOL_BEFORE[net]:
            pk, ps = L.POOL_BEFORE[net][i]
            x = F.max_pool2d(x, pk, ps)
        w = _get(sd, (f"net.slice{sl}.{i}.weight", f"features.{i}.weight")).to(torch.float32)
        b = _get(sd, (f"net.slice{sl}.{i}.bias", f"features.{i}.bias")).to(torch.float32)
        x = r(F.relu(F.conv2d(x, r(w), b, stride=s, padding=p)))
        if i in L.TAPS[net]:
            taps.append(x)
    return taps


def lins(sd):
    return [_get(sd, (f"lin{t}.model.1.weight", f"lins.{t}.model.1.weight")).to(torch.float32).reshape(-1).numpy() for t in range(5)]


def rows_of(t):
    """fp32 NCHW -> (N, h w, C) numpy."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).numpy()


def distance(sd, net, a, b):
    """a, b: (P, H, W, 3) uint8 -> (P, 5) float64: the fp32 tower and the float64 head on its (unrounded) taps."""
    ta, tb = tower(sd, net, scaled_input(a)), tower(sd, net, scaled_input(b))
    return np.stack([head_f64(rows_of(x), rows_of(y), w) for x, y, w in zip(ta, tb, lins(sd))], axis=1)


# ------------------------------------------------------------------------------------------------ test inputs
def features(P, hw, c, seed, magnitude=1.0, zero_fraction=0.5):
    """Post-ReLU-like f16 features (P, hw, c): half-normal values of the given magnitude, about half of them zero."""
    rng = np.random.RandomState(seed)
    v = np.abs(rng.standard_normal((P, hw, c))) * magnitude
    v[rng.random_sample(v.shape) < zero_fraction] = 0.0
    return v.astype(np.float16)


def lin_weights(c, seed):
    return np.random.RandomState(seed).random_sample(c).astype(np.float32)
