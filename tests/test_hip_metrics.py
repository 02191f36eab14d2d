"""GPU: rcdm_frame_metrics and rcdms_amd.metrics against the float64 restatement tests/ssim_oracle.py.

Sizes are the smallest at which the kernel can still go wrong: the 37 x 53 fixtures (more than one tile on both axes, ragged on
both), 7 x 7 with the box and 11 x 11 with the Gaussian (one map value), 6 x 9 refused, 64 x 64, five pairs of 128 x 128.
Layouts: dense, and the cells of a 2 x 3 grid of 53-pixel-wide cells (row pitch 3 * 3 * 53 bytes and more, bases at odd
byte offsets, `a` and `b` at different pitches).  Buffer discipline as tests/guard.py: the images lie in finite poison — the
bytes between 3 W and the pitch included —, the outputs between NaN / canary bands that are checked after the values.
Bounds: ssim_oracle.BUDGET (1e-6) on every channel mean; identical pairs exactly 1.0; sse and sad exact integers; two calls
on the same inputs return the same bits."""
import numpy as np
import pytest
import torch

from tests import guard
from tests import ssim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 64                     # elements of NaN / canary on either side of an output
MARGIN = 4096                 # bytes of poison in front of and behind an image buffer
FIX = O.fixtures()
H, W = O.FIXTURE_SHAPE[:2]
_ORACLE = {}


def oracle(key, a, b, window, sample):
    """Channel means of one pair, computed once per (key, window, sample) and shared by the tests."""
    k = (key, window, sample)
    if k not in _ORACLE:
        _ORACLE[k] = O.ssim_channels(a, b, window, sample)
    return _ORACLE[k]


def poison_u8(numel, salt):
    """Bytes of a fixed hash of the index: every value is a finite pixel, so an over-read changes the figure, never hides."""
    i = torch.arange(numel, dtype=torch.int64, device=DEV) + 7919 * salt
    h = (i * 2654435761) & 0xFFFFFFFF
    return ((h >> 11) & 0xFF).to(torch.uint8)


class Images:
    """n images (numpy uint8 (n, h, w, 3)) inside one poisoned byte buffer at `base` + i * stride, rows `pitch` apart."""

    def __init__(self, images, pitch, stride, base=0, salt=1):
        n, h, w, _ = images.shape
        assert pitch >= 3 * w
        extent = base + (n - 1) * stride + (h - 1) * pitch + 3 * w
        self.buf = poison_u8(MARGIN + extent + MARGIN, salt)
        self.view = self.buf.as_strided((n, h, w, 3), (stride, pitch, 3, 1), MARGIN + base)
        self.view.copy_(torch.from_numpy(images))
        self.snapshot = self.buf.clone()
        self.pitch, self.stride = pitch, stride

    def check(self):
        assert torch.equal(self.buf, self.snapshot), "a read-only image buffer changed"


class Outputs:
    def __init__(self, n):
        self.n = n
        self.f = torch.full((BAND + 3 * n + BAND,), float("nan"), dtype=torch.float64, device=DEV)
        self.i = [torch.full(((BAND + 3 * n + BAND) * 8,), guard.INT_FILL, dtype=torch.uint8, device=DEV).view(torch.int64) for _ in range(2)]
        self.fill = int(self.i[0][0])

    ssim = property(lambda s: s.f[BAND:BAND + 3 * s.n].view(s.n, 3))
    sse = property(lambda s: s.i[0][BAND:BAND + 3 * s.n].view(s.n, 3))
    sad = property(lambda s: s.i[1][BAND:BAND + 3 * s.n].view(s.n, 3))

    def check(self):
        f = self.f.view(torch.int64)
        nan = int(torch.full((1,), float("nan"), dtype=torch.float64).view(torch.int64)[0])
        assert bool((f[:BAND] == nan).all()) and bool((f[BAND + 3 * self.n:] == nan).all()), "wrote outside ssim[n][3]"
        for t, name in zip(self.i, ("sse", "sad")):
            assert bool((t[:BAND] == self.fill).all()) and bool((t[BAND + 3 * self.n:] == self.fill).all()), f"wrote outside {name}[n][3]"


def run(hip, a, b, window, sample=True, ws_extra=0):
    """One rcdm_frame_metrics call on two `Images` -> `Outputs`; the workspace is exactly the size the query names, between
    canaries."""
    n, h, w, _ = a.view.shape
    d = hip.MetricsDesc(a.pitch, a.stride if n > 1 else 0, b.pitch, b.stride if n > 1 else 0, n, h, w, 3,
                        hip.SSIM_GAUSS11 if window == "gaussian" else hip.SSIM_UNIFORM7, int(sample))
    need = hip.frame_metrics_workspace_bytes(d)
    assert need > 0 and need % 8 == 0
    ws = torch.full((BAND * 8 + need + BAND * 8,), guard.INT_FILL, dtype=torch.uint8, device=DEV)
    win = torch.full((BAND + 11 + BAND,), 3.0e4, dtype=torch.float64, device=DEV)
    win[BAND:BAND + 11] = torch.from_numpy(O.gaussian_window()).to(DEV)
    out = Outputs(n)
    hip.frame_metrics(d, a.view.data_ptr(), b.view.data_ptr(), win[BAND:].data_ptr(), out.ssim.data_ptr(), out.sse.data_ptr(),
                      out.sad.data_ptr(), ws[BAND * 8:].data_ptr(), need)
    torch.cuda.synchronize()
    assert bool((ws[:BAND * 8] == guard.INT_FILL).all()) and bool((ws[BAND * 8 + need:] == guard.INT_FILL).all()), "wrote outside the workspace"
    return out


def verify(out, pairs, keys, window, sample, what):
    """Values first, then the guards."""
    got = out.ssim.cpu().numpy()
    assert np.isfinite(got).all(), f"{what}: unwritten ssim"
    for i, ((a, b), key) in enumerate(zip(pairs, keys)):
        want = oracle(key, a, b, window, sample)
        err = np.abs(got[i] - want).max()
        print(f"{what} [{key}] {window} sample={sample}: ssim {got[i].mean():.9f}, |device - oracle| {err:.2e}")
        assert err <= O.BUDGET, (key, got[i].tolist(), want.tolist())
        if np.array_equal(a, b):
            assert (got[i] == 1.0).all(), (key, got[i].tolist())
        sse, sad = O.sse_sad(a, b)
        assert out.sse[i].tolist() == sse.tolist() and out.sad[i].tolist() == sad.tolist(), key
    out.check()


def stack(side):
    return np.stack([FIX[name][side] for name in O.FIXTURES])


@pytest.mark.parametrize("sample", [True, False])
@pytest.mark.parametrize("window", O.WINDOWS)
def test_fixtures_dense(hiplib, window, sample):
    from rcdms_amd import hip
    a, b = Images(stack(0), 3 * W, 3 * W * H, salt=1), Images(stack(1), 3 * W, 3 * W * H, salt=2)
    out = run(hip, a, b, window, sample)
    verify(out, [FIX[k] for k in O.FIXTURES], O.FIXTURES, window, sample, "dense")
    i = O.FIXTURES.index("black_white")
    assert np.abs(out.ssim[i].cpu().numpy() - O.BLACK_WHITE).max() <= O.BUDGET
    again = run(hip, a, b, window, sample)
    assert torch.equal(out.ssim.view(torch.int64), again.ssim.view(torch.int64)), "two calls on the same inputs differ in their bits"
    assert torch.equal(out.sse, again.sse) and torch.equal(out.sad, again.sad)
    a.check()
    b.check()


@pytest.mark.parametrize("window", O.WINDOWS)
def test_fixtures_as_grid_cells(hiplib, window):
    """The six fixtures as the cells of a 2 x 3 grid image: a row of cells is one call with n = 3 (stride 3 W, pitch 9 W), a
    single cell a call with n = 1.  `a`'s grid starts at an odd byte; `b`'s rows carry 7 more bytes of poison."""
    from rcdms_amd import hip
    pa, pb = 9 * W, 9 * W + 7
    rows = []
    for r in range(2):
        names = O.FIXTURES[3 * r:3 * r + 3]
        a = Images(np.stack([FIX[k][0] for k in names]), pa, 3 * W, base=1 + r * H * pa, salt=3 + r)
        b = Images(np.stack([FIX[k][1] for k in names]), pb, 3 * W, base=r * H * pb, salt=5 + r)
        assert {(a.view.data_ptr() + 3 * W * c) % 2 for c in range(3)} == {0, 1}      # 3 W is odd: cell bases of both parities
        out = run(hip, a, b, window)
        verify(out, [FIX[k] for k in names], names, window, True, f"grid row {r}")
        rows.append((a, b, names, out))
    # one cell alone, the middle one of the second row: base 3 W bytes into a row, an odd offset
    a, b, names, whole = rows[1]
    ca, cb = Images.__new__(Images), Images.__new__(Images)
    for cell, src in ((ca, a), (cb, b)):
        cell.buf, cell.snapshot, cell.pitch, cell.stride = src.buf, src.snapshot, src.pitch, 0
        cell.view = src.view[1:2]
    assert (ca.view.data_ptr() - a.view.data_ptr()) == 3 * W and (3 * W) % 2 == 1
    out = run(hip, ca, cb, window)
    verify(out, [FIX[names[1]]], [names[1]], window, True, "grid cell")
    assert torch.equal(out.ssim.view(torch.int64)[0], whole.ssim.view(torch.int64)[1]), "a cell alone and in its row differ"
    for a, b, _, _ in rows:
        a.check()
        b.check()


def random_pairs(n, h, w, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.randint(-40, 41, size=a.shape), 0, 255).astype(np.uint8)
    b[-1] = rng.randint(0, 256, size=(h, w, 3))
    return a, b


@pytest.mark.parametrize("n,h,w,window", [(2, 7, 7, "uniform"), (2, 11, 11, "gaussian"), (1, 64, 64, "uniform"), (1, 64, 64, "gaussian"),
                                          (5, 128, 128, "uniform"), (5, 128, 128, "gaussian"), (1, 11, 40, "gaussian"), (1, 30, 7, "uniform")])
def test_sizes(hiplib, n, h, w, window):
    """One map value (7 x 7 / 11 x 11), one map row or column, 64 x 64, five pairs of 128 x 128; padded rows throughout."""
    from rcdms_amd import hip
    an, bn = random_pairs(n, h, w, 100 * h + w)
    a = Images(an, 3 * w + 13, (3 * w + 13) * h + 5, base=3, salt=7)
    b = Images(bn, 3 * w, 3 * w * h, salt=8)
    out = run(hip, a, b, window)
    verify(out, list(zip(an, bn)), [(n, h, w, i) for i in range(n)], window, True, f"{n} x {h}x{w}")
    again = run(hip, a, b, window)
    assert torch.equal(out.ssim.view(torch.int64), again.ssim.view(torch.int64))
    a.check()
    b.check()


def test_images_below_the_window_are_refused(hiplib):
    from rcdms_amd import hip
    an, bn = random_pairs(1, 6, 9, 5)
    a, b = Images(an, 27, 0), Images(bn, 27, 0)
    for window in O.WINDOWS:
        d = hip.MetricsDesc(27, 0, 27, 0, 1, 6, 9, 3, hip.SSIM_GAUSS11 if window == "gaussian" else hip.SSIM_UNIFORM7, 1)
        assert hip.frame_metrics_workspace_bytes(d) == 0
        out = Outputs(1)
        ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
        with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
            hip.frame_metrics(d, a.view.data_ptr(), b.view.data_ptr(), ws.data_ptr(), out.ssim.data_ptr(), out.sse.data_ptr(),
                              out.sad.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.ssim).all()) and bool((out.sse == out.fill).all()), "a refused call wrote its outputs"
    # 7 x 10 takes the box and not the Gaussian
    d = hip.MetricsDesc(30, 0, 30, 0, 1, 7, 10, 3, hip.SSIM_GAUSS11, 1)
    assert hip.frame_metrics_workspace_bytes(d) == 0
    d.window = hip.SSIM_UNIFORM7
    assert hip.frame_metrics_workspace_bytes(d) == 9 * 8


# ---- the Python layer -----------------------------------------------------------------------------------------------------

def test_frame_metrics_fields(hiplib):
    from rcdms_amd import metrics as M
    a, b = torch.from_numpy(stack(0)).to(DEV), torch.from_numpy(stack(1)).to(DEV)
    for window in O.WINDOWS:
        fm = M.frame_metrics(a, b, window=window)
        assert tuple(fm.ssim.shape) == (6,) and tuple(fm.ssim_channels.shape) == (6, 3) and fm.ssim.dtype == torch.float64
        assert tuple(fm.mse.shape) == tuple(fm.psnr.shape) == tuple(fm.mae.shape) == (6,) and fm.ssim.is_cuda
        for i, k in enumerate(O.FIXTURES):
            want = oracle(k, *FIX[k], window, True)
            assert np.abs(fm.ssim_channels[i].cpu().numpy() - want).max() <= O.BUDGET
            assert abs(float(fm.ssim[i]) - want.mean()) <= O.BUDGET
            sse, sad = O.sse_sad(*FIX[k])
            assert float(fm.mse[i]) == sse.sum() / (3.0 * H * W) and float(fm.mae[i]) == sad.sum() / (3.0 * H * W)
            assert float(fm.psnr[i]) == pytest.approx(O.psnr(*FIX[k]), rel=1e-12)
        i = O.FIXTURES.index("identical")
        assert float(fm.ssim[i]) == 1.0 and float(fm.psnr[i]) == float("inf") and float(fm.mse[i]) == 0.0
        assert torch.equal(M.ssim(a, b, window=window), fm.ssim)
    assert torch.equal(M.psnr(a, b), M.frame_metrics(a, b).psnr)
    pop = M.frame_metrics(a[:1], b[:1], sample_covariance=False).ssim_channels[0].cpu().numpy()
    assert np.abs(pop - oracle("noise", *FIX["noise"], "uniform", False)).max() <= O.BUDGET


def test_frame_metrics_reads_grid_slices_where_they_lie(hiplib):
    from rcdms_amd import metrics as M
    grid_a = guard_grid(0, pad=0)
    grid_b = guard_grid(1, pad=7)
    want = M.frame_metrics(torch.from_numpy(stack(0)).to(DEV), torch.from_numpy(stack(1)).to(DEV)).ssim_channels
    for r in range(2):
        ca, cb = cells(grid_a, r), cells(grid_b, r)                    # (3, H, W, 3): stride 3 W, pitch of the grid
        assert ca.stride() == (3 * W, 9 * W, 3, 1) and cb.stride() == (3 * W, 9 * W + 7, 3, 1)
        assert M._view(ca).data_ptr() == ca.data_ptr() and M._view(cb).data_ptr() == cb.data_ptr(), "a grid row was copied"
        got = M.frame_metrics(ca, cb).ssim_channels
        assert torch.equal(got.view(torch.int64), want[3 * r:3 * r + 3].view(torch.int64))
        one = M.frame_metrics(ca[2], cb[2]).ssim_channels               # (H, W, 3): a single cell
        assert torch.equal(one.view(torch.int64), want[3 * r + 2:3 * r + 3].view(torch.int64))
    # rows x columns at once have no single image stride: the figures are the same, through a copy
    both = M.frame_metrics(torch.stack([cells(grid_a, 0), cells(grid_a, 1)]), torch.stack([cells(grid_b, 0), cells(grid_b, 1)]))
    assert tuple(both.ssim.shape) == (6,) and torch.equal(both.ssim_channels.view(torch.int64), want.view(torch.int64))
    all_a = grid_a.as_strided((2, 3, H, W, 3), (H * 9 * W, 3 * W, 9 * W, 3, 1))
    all_b = grid_b.as_strided((2, 3, H, W, 3), (H * (9 * W + 7), 3 * W, 9 * W + 7, 3, 1))
    assert torch.equal(M.frame_metrics(all_a, all_b).ssim_channels.view(torch.int64), want.view(torch.int64))


def guard_grid(side, pad):
    """The six fixtures' `side` as one 2 x 3 grid image, rows 9 W + pad bytes apart, pad bytes poisoned."""
    pitch = 9 * W + pad
    g = poison_u8(2 * H * pitch, 11 + side)
    v = g.as_strided((2, 3, H, W, 3), (H * pitch, 3 * W, pitch, 3, 1))
    v.copy_(torch.from_numpy(stack(side)).view(2, 3, H, W, 3))
    return g


def cells(grid, r):
    pitch = grid.numel() // (2 * H)
    return grid.as_strided((3, H, W, 3), (3 * W, pitch, 3, 1), r * H * pitch)


def test_frame_metrics_refuses_what_it_does_not_take(hiplib):
    from rcdms_amd import hip
    from rcdms_amd import metrics as M
    a = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(hip.RcdmError):
        M.frame_metrics(a.cpu(), a.cpu())
    with pytest.raises(hip.RcdmError):
        M.frame_metrics(a, a.cpu())
    with pytest.raises(ValueError):
        M.frame_metrics(a.float(), a.float())
    with pytest.raises(ValueError):
        M.frame_metrics(a, a[:, :15])
    with pytest.raises(ValueError):
        M.frame_metrics(a[..., :2], a[..., :2])
    with pytest.raises(hip.RcdmError, match="smaller than"):
        M.frame_metrics(a[:, :10], a[:, :10], window="gaussian")
    with pytest.raises(hip.RcdmError):
        M.frame_metrics(a[:, :6], a[:, :6])
