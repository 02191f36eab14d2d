"""CPU: the frame metrics without a device — the float64 restatement tests/ssim_oracle.py against scipy's filters (and against
scikit-image where it imports), its closed forms, the float32 model the budget must catch, the shared core
csrc/ssim_core.h compiled into tools/ssim_host.cpp and run over every fixture with both windows, and the argument checks of
rcdm_frame_metrics (nothing is launched: the pointers are never dereferenced)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import ssim_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
FIX = O.fixtures()
CASES = [(name, window) for name in O.FIXTURES for window in O.WINDOWS]


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


# ------------------------------------------------------------------------------------------------ the restatement
def test_fixtures_are_what_they_are_named():
    assert set(FIX) == set(O.FIXTURES)
    for name, (a, b) in FIX.items():
        assert a.shape == b.shape == O.FIXTURE_SHAPE and a.dtype == b.dtype == np.uint8, name
    a, b = FIX["bright_flat"]
    assert (a == 250).all() and int((a.astype(int) - b).sum()) == 3 * 19 * 27 and (b[1::2] == 250).all() and (b[:, 1::2] == 250).all()
    a, b = FIX["gradient"]
    assert a[5, 7, 0] == 12 and np.abs(a.astype(int) - b).max() == 2
    a, b = FIX["checkerboard"]
    assert set(np.unique(a)) == {0, 255} and (a.astype(int) + b == 255).all() and a[0, 0, 0] != a[0, 1, 0] != a[1, 1, 0]
    assert np.array_equal(FIX["identical"][0], FIX["identical"][1]) and not np.array_equal(*FIX["noise"])
    again = O.fixtures()
    assert all(np.array_equal(FIX[k][i], again[k][i]) for k in FIX for i in (0, 1)), "fixtures depend on more than the seed"


def test_gaussian_window_is_skimage_s():
    w = O.gaussian_window()
    assert len(w) == 11 and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert abs(w[4] / w[5] - np.exp(-1.0 / 4.5)) < 1e-15


@pytest.mark.parametrize("name,window", [c for c in CASES if c in O.EXPECTED])
def test_recorded_values_and_closed_forms(name, window):
    for sample in (True, False):
        got = O.ssim_channels(*FIX[name], window, sample)
        if name == "identical":
            assert (got == 1.0).all()
        elif name == "black_white":
            assert np.abs(got - O.C1 / (255.0 ** 2 + O.C1)).max() < 1e-15         # no variance: cov_norm drops out
    assert abs(O.ssim(*FIX[name], window) - O.EXPECTED[(name, window)]) < 5e-10
    assert abs(O.BLACK_WHITE - 0.00009999) < 1e-9


def test_sse_sad_and_psnr():
    sse, sad = O.sse_sad(*FIX["black_white"])
    assert sse.tolist() == [37 * 53 * 255 * 255] * 3 and sad.tolist() == [37 * 53 * 255] * 3
    assert O.psnr(*FIX["black_white"]) == 0.0 and O.psnr(*FIX["identical"]) == float("inf")
    sse, sad = O.sse_sad(*FIX["bright_flat"])
    assert sse.tolist() == sad.tolist() == [19 * 27] * 3


@pytest.mark.parametrize("window", O.WINDOWS)
def test_naive_float32_misses_the_budget(window):
    """The budget discriminates: float32 moments with uxx - ux ux in fp32 are off by more than it on the bright-flat pair."""
    want = O.ssim_channels(*FIX["bright_flat"], window)
    err = np.abs(O.naive_f32(*FIX["bright_flat"], window) - want).max()
    print(f"bright-flat, {window}: float32 model off by {err:.2e}")
    assert err > O.BUDGET


@pytest.mark.parametrize("name,window", CASES)
def test_oracle_equals_scipy_filters(name, window):
    """skimage's own arithmetic: scipy.ndimage filters over the whole image (reflect border), then the crop."""
    ndi = pytest.importorskip("scipy.ndimage")
    a, b = (t.astype(np.float64) for t in FIX[name])
    for sample in (True, False):
        chans = []
        for c in range(3):
            x, y = a[:, :, c], b[:, :, c]
            if window == "gaussian":
                f = lambda t: ndi.gaussian_filter(t, sigma=1.5, truncate=3.5, mode="reflect")
            else:
                f = lambda t: ndi.uniform_filter(t, size=7)
            npx = float(O.WIN[window] ** 2)
            cn = npx / (npx - 1) if sample else 1.0
            ux, uy = f(x), f(y)
            vx, vy, vxy = cn * (f(x * x) - ux * ux), cn * (f(y * y) - uy * uy), cn * (f(x * y) - ux * uy)
            S = ((2 * ux * uy + O.C1) * (2 * vxy + O.C2)) / ((ux ** 2 + uy ** 2 + O.C1) * (vx + vy + O.C2))
            pad = (O.WIN[window] - 1) // 2
            chans.append(S[pad:-pad, pad:-pad].mean(dtype=np.float64))
        err = np.abs(np.array(chans) - O.ssim_channels(*FIX[name], window, sample)).max()
        assert err < 1e-9, (sample, err)        # both float64; scipy's running sums round differently (measured <= 2e-11)


@pytest.mark.parametrize("name,window", CASES)
def test_oracle_equals_skimage(name, window):
    metrics = pytest.importorskip("skimage.metrics")
    kw = dict(gaussian_weights=True, sigma=1.5) if window == "gaussian" else {}
    for sample in (True, False):
        want = metrics.structural_similarity(*FIX[name], channel_axis=-1, data_range=255, use_sample_covariance=sample, **kw)
        assert abs(O.ssim(*FIX[name], window, sample) - want) < 1e-9


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/ssim_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("ssim") / "ssim_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "ssim_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_tool(exe, tmp_path, a, b, window, sample=True):
    pa, pb = str(tmp_path / "a.raw"), str(tmp_path / "b.raw")
    a.tofile(pa)
    b.tofile(pb)
    flags = (["--gaussian"] if window == "gaussian" else []) + ([] if sample else ["--population"])
    r = subprocess.run([exe, *flags, str(a.shape[0]), str(a.shape[1]), pa, pb], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    f = r.stdout.decode().split()
    assert len(f) == 9
    return np.array([float(v) for v in f[:3]]), [int(v) for v in f[3:6]], [int(v) for v in f[6:]]


@pytest.mark.parametrize("name,window", CASES)
def test_host_tool_on_every_fixture(host_tool, tmp_path, name, window):
    a, b = FIX[name]
    sse, sad = O.sse_sad(a, b)
    for sample in (True, False):
        got, gsse, gsad = run_tool(host_tool, tmp_path, a, b, window, sample)
        err = np.abs(got - O.ssim_channels(a, b, window, sample)).max()
        print(f"{name}, {window}, sample_covariance={sample}: |core - oracle| {err:.2e}")
        assert err <= O.BUDGET
        assert gsse == sse.tolist() and gsad == sad.tolist()
        if name == "identical":
            assert (got == 1.0).all(), got.tolist()


def test_host_tool_smallest_images_and_refusals(host_tool, tmp_path):
    rng = np.random.RandomState(3)
    for side, window in ((7, "uniform"), (11, "gaussian")):
        a, b = (rng.randint(0, 256, size=(side, side, 3)).astype(np.uint8) for _ in range(2))
        got, _, _ = run_tool(host_tool, tmp_path, a, b, window)
        assert np.abs(got - O.ssim_channels(a, b, window)).max() <= O.BUDGET      # one map value per channel
    a = np.zeros((6, 9, 3), dtype=np.uint8)
    a.tofile(str(tmp_path / "s.raw"))
    r = subprocess.run([host_tool, "6", "9", str(tmp_path / "s.raw"), str(tmp_path / "s.raw")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"window" in r.stderr
    r = subprocess.run([host_tool, "7", "9", str(tmp_path / "s.raw"), str(tmp_path / "s.raw")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"exactly" in r.stderr                            # 162 bytes for a 7 x 9 image


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in ("rcdm_frame_metrics", "rcdm_frame_metrics_workspace_bytes"):
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.MetricsDesc) == 56
    text = open(os.path.join(ROOT, "include", "rcdm.h")).read()
    assert f"#define RCDM_SSIM_UNIFORM7 {hip.SSIM_UNIFORM7}\n" in text and f"#define RCDM_SSIM_GAUSS11 {hip.SSIM_GAUSS11}\n" in text


def test_argument_validation_without_gpu():
    """The entry point refuses bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    H, W, n = 37, 53, 2
    a, b, win, ssim, sse, sad, ws = 0x1001, 0x2003, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000       # never dereferenced

    def desc(**kw):
        f = dict(a_pitch=3 * W, a_stride=3 * W * H, b_pitch=3 * W + 5, b_stride=(3 * W + 5) * H, n=n, H=H, W=W, channels=3,
                 window=hip.SSIM_UNIFORM7, sample_covariance=1)
        f.update(kw)
        return hip.MetricsDesc(**f)

    def call(d=None, need=None, **kw):
        d = desc() if d is None else d
        p = dict(a=a, b=b, win=win, ssim=ssim, sse=sse, sad=sad, ws=ws)
        p.update(kw)
        need = lib.rcdm_frame_metrics_workspace_bytes(ctypes.byref(d)) if need is None else need
        return lib.rcdm_frame_metrics(ctypes.byref(d), p["a"], p["b"], p["win"], p["ssim"], p["sse"], p["sad"], p["ws"], need, None)

    need = lib.rcdm_frame_metrics_workspace_bytes(ctypes.byref(desc()))
    assert need > 0 and need % 8 == 0 and need % (n * 9 * 8) == 0
    assert lib.rcdm_frame_metrics_workspace_bytes(None) == 0
    assert lib.rcdm_frame_metrics(None, a, b, win, ssim, sse, sad, ws, need, None) == EINVAL
    for k in ("a", "b", "ssim", "sse", "sad"):
        assert call(**{k: None}) == EINVAL, k
    assert call(desc(window=hip.SSIM_GAUSS11), win=None) == EINVAL
    for bad in (dict(n=0), dict(n=-3), dict(H=0), dict(W=-1), dict(window=2), dict(window=-1), dict(a_pitch=3 * W - 1),
                dict(b_pitch=3 * W - 1), dict(a_stride=-1), dict(b_stride=-1)):
        assert call(desc(**bad), need=need) == EINVAL, bad
        assert lib.rcdm_frame_metrics_workspace_bytes(ctypes.byref(desc(**bad))) == 0, bad
    for bad in (dict(H=6), dict(W=6), dict(H=10, window=hip.SSIM_GAUSS11), dict(W=10, window=hip.SSIM_GAUSS11), dict(channels=4),
                dict(H=8193, a_pitch=3 * 8193), dict(n=65536)):
        assert call(desc(**bad), need=need) == ESHAPE, bad
        assert lib.rcdm_frame_metrics_workspace_bytes(ctypes.byref(desc(**bad))) == 0, bad
    for k in ("win", "ssim", "sse", "sad", "ws"):
        assert call(**{k: 0x9004}) == EINVAL, k                                  # 8-byte alignment of the float64 / int64 buffers
    assert call(ws=None) == EWORKSPACE and call(need=need - 1) == EWORKSPACE and call(need=0) == EWORKSPACE
    # the smallest images each window takes have a workspace of one tile per pair
    for side, window in ((7, hip.SSIM_UNIFORM7), (11, hip.SSIM_GAUSS11)):
        d = desc(H=side, W=side, a_pitch=3 * side, b_pitch=3 * side, window=window)
        assert lib.rcdm_frame_metrics_workspace_bytes(ctypes.byref(d)) == n * 9 * 8


def test_frame_metrics_has_no_cpu_path():
    import torch
    from rcdms_amd import hip
    from rcdms_amd import metrics as M
    a = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(hip.RcdmError):
        M.frame_metrics(a, a)                                                    # a host tensor, with or without a GPU
    with pytest.raises(ValueError):
        M.frame_metrics(a.float(), a.float())
    with pytest.raises(ValueError):
        M.frame_metrics(a, a[:7])
    with pytest.raises(ValueError):
        M.frame_metrics(a, a, window="box")
    with pytest.raises(TypeError):
        M.frame_metrics(a.numpy(), a.numpy())
