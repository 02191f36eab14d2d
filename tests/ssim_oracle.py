"""Float64 restatement of scikit-image's structural_similarity(a, b, channel_axis=-1, data_range=255) in pure numpy, the
named fixtures of the frame-metrics tests and their error budget.  No scipy, no skimage, no torch: it runs wherever the
tests run.  tests/test_ssim_host.py holds it against scipy's filters (and against skimage where that imports).

  definition  per channel, with F the window mean over the window positions that lie inside the image ("valid" region: skimage
              filters with a border mode and then crops (win - 1) // 2 rows and columns, so the border mode never shows):
                ux = F(x), uy = F(y), vx = cn (F(x x) - ux ux), vy = cn (F(y y) - uy uy), vxy = cn (F(x y) - ux uy)
                S = (2 ux uy + C1) (2 vxy + C2) / ((ux ux + uy uy + C1) (vx + vy + C2)),  C1 = (0.01 255)^2, C2 = (0.03 255)^2
              cn = NP / (NP - 1), NP = win^2 (use_sample_covariance, the default) or 1.  Channel figure: the mean of S; the
              image figure: the mean of the three channel figures.
  windows     "uniform": 7 x 7 box (skimage's default win_size).  "gaussian": gaussian_weights=True, sigma = 1.5, truncate
              3.5 -> radius 5, 11 taps exp(-i^2 / (2 sigma^2)) normalised, applied separably (rows, then columns).
  BUDGET      |device - oracle| <= 1e-6 on every channel mean: what a six-decimal figure needs.  It separates designs: on
              the bright-flat fixture float32 moments (uxx - ux ux in fp32) are off by several 1e-6 (`naive_f32`), exact
              integer sums or float64 accumulation by less than 1e-12."""
import numpy as np

BUDGET = 1e-6
K1, K2, DATA_RANGE = 0.01, 0.03, 255.0
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
SIGMA, RADIUS = 1.5, 5                                   # int(3.5 * 1.5 + 0.5) = 5
WINDOWS = ("uniform", "gaussian")
WIN = {"uniform": 7, "gaussian": 2 * RADIUS + 1}
FIXTURE_SHAPE = (37, 53, 3)
BLACK_WHITE = C1 / (255.0 ** 2 + C1)                     # ux = 0, uy = 255, no variance: S = C1 C2 / ((255^2 + C1) C2)


def gaussian_window(dtype=np.float64):
    i = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return (w / w.sum()).astype(dtype)


def taps(window, dtype=np.float64):
    if window not in WIN:
        raise ValueError(f"window {window!r}: one of {WINDOWS}")
    return gaussian_window(dtype) if window == "gaussian" else np.full(7, 1.0 / 7.0, dtype=dtype)


def _filter(x, w):
    """Separable valid-region filter over axes 0 and 1 of x (H, W, ...), taps in index order, in x's dtype."""
    n = len(w)
    mh, mw = x.shape[0] - n + 1, x.shape[1] - n + 1
    rows = np.zeros((x.shape[0], mw) + x.shape[2:], dtype=x.dtype)
    for i in range(n):
        rows += w[i] * x[:, i:i + mw]
    out = np.zeros((mh, mw) + x.shape[2:], dtype=x.dtype)
    for i in range(n):
        out += w[i] * rows[i:i + mh]
    return out


def _check(a, b, window):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"uint8 (H, W, 3) pairs, got {a.dtype} {a.shape} and {b.dtype} {b.shape}")
    if min(a.shape[:2]) < WIN[window]:
        raise ValueError(f"{a.shape[0]}x{a.shape[1]} is smaller than the {WIN[window]}-wide window")
    return a, b


def ssim_map(a, b, window="uniform", sample_covariance=True, dtype=np.float64):
    """S over the valid region, (H - win + 1, W - win + 1, 3), every step in `dtype` (float64: the oracle)."""
    a, b = _check(a, b, window)
    w = taps(window, dtype)
    x, y = a.astype(dtype), b.astype(dtype)
    npx = dtype(WIN[window] ** 2)
    cn = npx / (npx - dtype(1)) if sample_covariance else dtype(1)
    ux, uy = _filter(x, w), _filter(y, w)
    uxx, uyy, uxy = _filter(x * x, w), _filter(y * y, w), _filter(x * y, w)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    c1, c2 = dtype(C1), dtype(C2)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_channels(a, b, window="uniform", sample_covariance=True):
    """(3,) float64: the channel means."""
    return ssim_map(a, b, window, sample_covariance).mean(axis=(0, 1), dtype=np.float64)


def ssim(a, b, window="uniform", sample_covariance=True):
    """What structural_similarity(..., channel_axis=-1) returns."""
    return float(ssim_channels(a, b, window, sample_covariance).mean())


def naive_f32(a, b, window="uniform", sample_covariance=True):
    """(3,) the straightforward float32 evaluation (float32 moments, uxx - ux ux in fp32), its mean taken in float64: the
    design the budget must catch."""
    return ssim_map(a, b, window, sample_covariance, dtype=np.float32).astype(np.float64).mean(axis=(0, 1))


def sse_sad(a, b):
    """((3,) int64 sum of squared differences, (3,) int64 sum of absolute differences) over the whole image."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return (d * d).sum(axis=(0, 1)), np.abs(d).sum(axis=(0, 1))


def psnr(a, b):
    sse, _ = sse_sad(a, b)
    mse = sse.sum() / float(np.asarray(a).size)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def fixtures(seed=20240519, shape=FIXTURE_SHAPE):
    """name -> (a, b), uint8 `shape`, all from `seed`."""
    h, w, c = shape
    rng = np.random.RandomState(seed)
    noise_a = rng.randint(0, 256, size=shape).astype(np.uint8)
    noise_b = rng.randint(0, 256, size=shape).astype(np.uint8)
    flat = np.full(shape, 250, dtype=np.uint8)
    dented = flat.copy()
    dented[::2, ::2] -= 1
    grad = ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 256).astype(np.int64)[:, :, None].repeat(c, axis=2)
    grad_noisy = np.clip(grad + rng.randint(-2, 3, size=shape), 0, 255).astype(np.uint8)
    check = (((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2) * 255).astype(np.uint8)[:, :, None].repeat(c, axis=2)
    return {
        "noise": (noise_a, noise_b),
        "identical": (noise_a, noise_a.copy()),
        "bright_flat": (flat, dented),
        "gradient": (grad.astype(np.uint8), grad_noisy),
        "checkerboard": (check, 255 - check),
        "black_white": (np.zeros(shape, dtype=np.uint8), np.full(shape, 255, dtype=np.uint8)),
    }


FIXTURES = ("noise", "identical", "bright_flat", "gradient", "checkerboard", "black_white")
# float64 values of this restatement (the three channels of these fixtures are equal), six significant digits and more
EXPECTED = {("identical", "uniform"): 1.0, ("identical", "gaussian"): 1.0,
            ("bright_flat", "uniform"): 0.996768108, ("bright_flat", "gaussian"): 0.996779291,
            ("black_white", "uniform"): BLACK_WHITE, ("black_white", "gaussian"): BLACK_WHITE}
