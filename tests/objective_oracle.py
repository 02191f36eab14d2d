"""A numpy model of the two kernels of the denoising objective (rcdms_amd/csrc/objective_core.h), for the CPU and GPU tests:

  rows     float32 operation by operation — numpy rounds every float32 product and sum on its own, as torch's separate
           kernels do — then round-to-nearest-even into float16.  `form="fma"` is the contracted expression
           fma(sa, x0, fl(s1m n)), evaluated exactly (a float64 sum rounded to odd, then to float32), the mistake the kernel's
           three roundings are held against.
  sums     the core's summation order in float64: a pixel's four channels ascending, the binary tree over 256 slots of a
           chunk, the chunks of a frame ascending from +0.0.
  exact    the same sums in Python rationals: float16 and float32 values are dyadic, so every term and the sum are exact
           fractions.

The a-priori bound.  With u = 2^-53, an element's term d^2 carries the rounding of d = double(eps) - double(n) twice and the
rounding of the product once, (1 + delta)^3, and then passes through at most D additions: 3 inside the pixel, 8 levels of the
tree, and chunks - 1 in the fold (the first chunk is added to +0.0, exactly).  Every term is non-negative, so
  |computed - exact| <= u (D + 3) sum(exact terms)
to first order in u; the second-order part is below 2^-90 of the sum at the sizes used here."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
CHUNK = 256
F16_NAN = 0x7E00
ROW_SHAPES = [(64, 64), (72, 64), (24, 16)]                  # (ld, c_pad)
BATCHES, FRAMES = (1, 3), (1, 5)
PLANES = [(1, 1), (3, 5), (16, 16), (17, 16)]                # (H, W): one pixel; odd; exactly one chunk; a chunk plus a tail
GEOMETRIES = [(B, F, H, W) for B in BATCHES for F in FRAMES for H, W in PLANES]
OFFS_SCALE = 0.1                                             # train_stage2.py's noise_offset is of this size
_CASES = {}


def chunks_per_frame(hw):
    return (hw + CHUNK - 1) // CHUNK


def addition_chain(hw):
    """D: the longest chain of additions between an element's term and the frame's sum."""
    return 3 + 8 + (chunks_per_frame(hw) - 1)


def bound(exact, hw):
    return U * (addition_chain(hw) + 3) * float(exact)


# ------------------------------------------------------------------------------------------------ rows
def target(noise, offs, offs_scale):
    """n = noise + (offs_scale * offs[b][c][f]): two float32 roundings; offs None: the noise itself."""
    if offs is None:
        return noise
    p = (np.float32(offs_scale) * offs.astype(np.float32)).astype(np.float32)
    return (noise + p[:, :, :, None, None]).astype(np.float32)


def fma_f32(a, b, c):
    """fl32(a b + c) with one rounding, for float32 arrays: the product is exact in float64; the float64 sum is rounded to odd
    (an inexact sum keeps a sticky last bit), which makes the second rounding to float32 the correct one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)                           # TwoSum: s + e is the exact sum
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def noised(x0, n, t, table, form="three"):
    """fp32 (B,4,f,H,W): (sa x0) + (s1m n) with t's table row per story; NaN where t is outside the table."""
    T = table.shape[0]
    out = np.empty_like(x0)
    for b in range(x0.shape[0]):
        if not 0 <= int(t[b]) < T:
            out[b] = np.nan
            continue
        sa, s1m = table[int(t[b])]
        y = (s1m * n[b]).astype(np.float32)
        if form == "fma":
            out[b] = fma_f32(np.full_like(x0[b], sa), x0[b], y)
        else:
            out[b] = ((sa * x0[b]).astype(np.float32) + y).astype(np.float32)
    return out


def ncfhw_to_rows(x):
    """(B,C,f,H,W) -> [(B f H W)][C]."""
    B, C = x.shape[:2]
    return np.ascontiguousarray(np.moveaxis(x, 1, -1)).reshape(-1, C)


def f16_bits(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(np.float16).view(np.uint16)


def rows(x0, noise, offs, offs_scale, t, table, mask, masked, c_pad, form="three"):
    """uint16 [(B f H W)][c_pad]: the f16 bits the kernel stores."""
    lat = noised(x0, target(noise, offs, offs_scale), t, table, form)
    out = np.zeros((x0.shape[0] * x0.shape[2] * x0.shape[3] * x0.shape[4], c_pad), np.uint16)
    out[:, 0:4] = f16_bits(ncfhw_to_rows(lat))
    bad = np.repeat(np.array([not 0 <= int(v) < table.shape[0] for v in t]), out.shape[0] // x0.shape[0])
    out[bad, 0:4] = F16_NAN
    out[:, 4:5] = f16_bits(ncfhw_to_rows(mask))
    out[:, 5:9] = f16_bits(ncfhw_to_rows(masked))
    return out


# ------------------------------------------------------------------------------------------------ sums
def _frames(eps_bits, n, variant):
    """(eps, n) as float64 [B][f][HW][channels]."""
    B, _, F, H, W = n.shape
    e = np.ascontiguousarray(eps_bits).view(np.float16).astype(np.float64).reshape(B, F, H * W, -1)
    if variant == "neighbour":
        e = np.roll(e, -1, axis=1)
    t = np.moveaxis(n.astype(np.float64), 1, -1).reshape(B, F, H * W, 4)
    return e, t


def sqerr(eps_bits, noise, offs, offs_scale, variant=None):
    """float64 [B][f] in the core's order.  eps_bits: uint16 [(B f H W)][>= 4] (>= 5 for variant "chan4").
    variants (the mistakes): "no_offs" the target without its offset, "chan4" a fifth channel in the sum, "neighbour" frame
    f read from the rows of frame f + 1."""
    n = target(noise, None if variant == "no_offs" else offs, offs_scale)
    e, t = _frames(eps_bits, n, variant)
    with np.errstate(invalid="ignore", over="ignore"):
        d = e[..., :4] - t
        p = d * d
        q = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
        if variant == "chan4":
            q = q + e[..., 4] * e[..., 4]
        B, F, HW = q.shape
        cpf = chunks_per_frame(HW)
        part = np.zeros((B, F, cpf * CHUNK))
        part[:, :, :HW] = q
        part = part.reshape(B, F, cpf, CHUNK)
        s = CHUNK // 2
        while s > 0:
            part[..., :s] = part[..., :s] + part[..., s:2 * s]
            s //= 2
        total = np.zeros((B, F))
        for j in range(cpf):
            total = total + part[:, :, j, 0]
    return total


def sqerr_exact(eps_bits, noise, offs, offs_scale):
    """[B][f] Fractions: the exact sum of (eps - n)^2 over the frame, n the float32 target."""
    n = target(noise, offs, offs_scale)
    e, t = _frames(eps_bits, n, None)
    B, F, HW, _ = t.shape
    out = [[Fraction(0)] * F for _ in range(B)]
    for b in range(B):
        for f in range(F):
            ev, tv = e[b, f, :, :4].reshape(-1).tolist(), t[b, f].reshape(-1).tolist()
            out[b][f] = sum(((Fraction(x) - Fraction(y)) ** 2 for x, y in zip(ev, tv)), Fraction(0))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------ inputs
def timesteps(B, T=1000, start=0):
    """B of the mixed timesteps 0, 1, 500, 999 (T - 1), from `start` on."""
    pool = [0, 1, T // 2, T - 1]
    return np.array([pool[(start + b) % 4] for b in range(B)], np.int64)


def _plant(rng, x0, noise, pos, shift, sa, s1m):
    """Put into x0[pos], noise[pos] a pair for which the contracted form rounds to another f16 than the three roundings;
    shift: the float32 offset term added to the noise at pos (0.0 without offs)."""
    n_cand = 1 << 20
    # the two forms differ by the rounding of sa x0: keep the other addend no larger than that product, so that the sum's
    # float16 boundaries are not much coarser than the difference
    spread = min(1.0, float(sa) / float(s1m))
    for _ in range(16):
        cx = (rng.standard_normal(n_cand) * 2.0).astype(np.float32)
        cn = (rng.standard_normal(n_cand) * spread - float(shift)).astype(np.float32)
        n = (cn + np.float32(shift)).astype(np.float32)
        y = (np.float32(s1m) * n).astype(np.float32)
        three = ((np.float32(sa) * cx).astype(np.float32) + y).astype(np.float32)
        fused = fma_f32(np.full_like(cx, sa), cx, y)
        hit = np.nonzero(f16_bits(three) != f16_bits(fused))[0]
        if hit.size:
            x0[pos], noise[pos] = cx[hit[0]], cn[hit[0]]
            return
    raise AssertionError("no float16-visible difference among the candidates")


def inputs(B, F, H, W, seed, table, t, offs_scale):
    """Random operands of one case; in every story with a valid timestep, channel 0 of the first pixel is fma-sensitive without
    the offset and channel 1 of the last pixel with it (tests/test_objective_host.py asserts both)."""
    rng = np.random.default_rng(seed)
    shape = (B, 4, F, H, W)
    g = {"x0": (rng.standard_normal(shape) * 1.5).astype(np.float32), "noise": rng.standard_normal(shape).astype(np.float32),
         "offs": rng.standard_normal((B, 4, F)).astype(np.float32),
         "mask": np.broadcast_to((rng.random((B, 1, F, 1, 1)) < 0.5).astype(np.float32), (B, 1, F, H, W)).copy(),
         "masked": rng.standard_normal(shape).astype(np.float32)}
    for b in range(B):
        if 0 <= int(t[b]) < table.shape[0]:
            sa, s1m = table[int(t[b])]
            _plant(rng, g["x0"], g["noise"], (b, 0, 0, 0, 0), 0.0, sa, s1m)
            shift = np.float32(offs_scale) * g["offs"][b, 1, F - 1]
            _plant(rng, g["x0"], g["noise"], (b, 1, F - 1, H - 1, W - 1), shift, sa, s1m)
    return g


def case(B, F, H, W, table):
    """The shared operands of geometry (B, f, H, W), built once and never written to: inputs() at the mixed timesteps (the
    geometry's number decides where in 0, 1, T / 2, T - 1 its first story starts), plus "t" and "eps" (8 columns)."""
    key = (B, F, H, W, table.tobytes())
    if key not in _CASES:
        k = GEOMETRIES.index((B, F, H, W)) if (B, F, H, W) in GEOMETRIES else 0
        t = timesteps(B, table.shape[0], start=k)
        g = inputs(B, F, H, W, 100 + k, table, t, OFFS_SCALE)
        g["t"] = t
        g["eps"] = eps_rows(B, F, H, W, 100 + k)
        for v in g.values():
            v.setflags(write=False)
        _CASES[key] = g
    return _CASES[key]


def eps_rows(B, F, H, W, seed, channels=8, integers=False):
    """uint16 [(B f H W)][channels]: random f16 predictions (integers: from -2 .. 2)."""
    rng = np.random.default_rng(seed + 1000)
    shape = (B * F * H * W, channels)
    v = rng.integers(-2, 3, shape).astype(np.float16) if integers else rng.standard_normal(shape).astype(np.float16)
    return v.view(np.uint16)
