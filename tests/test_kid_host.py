"""CPU: the kernel distance before a GPU runs it.  The numpy model (tests/kid_oracle.py) against the 60-digit goldens
(tools/mint_kid_golden.py) within the a-priori bound B, the unmasked kernel matrix against scikit-learn's polynomial_kernel,
integer cases against Python-int arithmetic bit for bit, the shared core csrc/kid_core.h compiled into tools/kid_host.cpp — it
must give the model's bits —, draw_subsets, and the argument checks of the new entry points and of the Python layer, which need
no device."""
import ctypes
import os
import subprocess
from decimal import Decimal, localcontext

import numpy as np
import pytest

from tests import kid_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_poly_mmd_workspace_bytes", "rcdm_poly_mmd", "rcdm_poly_gram_f64")
INTEGER_SHAPES = [(2, 1), (3, 3), (17, 5), (63, 16), (64, 48), (65, 130), (97, 16)]      # (m, d)


def error_to_digits(value, digits):
    """|value - the 50-digit decimal| without rounding the reference to float64 first."""
    with localcontext() as ctx:
        ctx.prec = 80
        return float(abs(Decimal(float(value)) - Decimal(str(digits))))


@pytest.fixture(scope="module")
def models():
    """case -> (golden file, the model's (subsets, 4) on its features), computed once."""
    out = {}
    for name in O.CASES:
        g = O.load(name)
        out[name] = (g, O.evaluate(g["x"], g["y"], g["ia"], g["ib"], float(g["gamma"]), float(g["coef0"]), int(g["degree"])))
    return out


def test_cases_cover_the_edges():
    g = {name: O.load(name) for name in O.CASES}
    shape = {name: (v["ia"].shape[1], v["x"].shape[1]) for name, v in g.items()}
    assert shape["m2_d1"] == (2, 1) and shape["m17_d5"] == (17, 5) and shape["m33_d48_relu"] == (33, 48)
    assert shape["m65_d130"] == (65, 130) and shape["m40_d256_relu"] == (40, 256)
    assert g["m33_d48_relu"]["x"].min() >= 0 and g["m40_d256_relu"]["y"].min() >= 0
    assert np.array_equal(g["self"]["x"], g["self"]["y"]) and np.array_equal(g["self"]["ia"], g["self"]["ib"])
    diff = g["mean_offset"]["y"].astype(np.float64) - g["mean_offset"]["x"].astype(np.float64)
    assert (diff == diff[0]).all() and np.ptp(diff[0]) > 0
    for k in ("x", "y"):
        assert np.array_equal(g["f16"][k].astype(np.float16).astype(np.float32), g["f16"][k])
    s3 = g["subsets3"]
    assert s3["ia"].shape == (3, 19) and s3["x"].shape[0] == 31 and s3["y"].shape[0] == 45
    assert (int(g["linear"]["degree"]), float(g["linear"]["coef0"])) == (1, 0.0)
    assert (int(g["quadratic"]["degree"]), float(g["quadratic"]["gamma"])) == (2, 0.5)
    for name, v in g.items():
        if name not in ("linear", "quadratic"):
            assert (int(v["degree"]), float(v["gamma"]), float(v["coef0"])) == (3, 1.0 / v["x"].shape[1], 1.0)


@pytest.mark.parametrize("name", list(O.CASES))
def test_model_against_the_60_digit_value(models, name):
    g, model = models[name]
    B = O.bound(g["x"], g["y"], g["ia"], g["ib"], float(g["gamma"]), float(g["coef0"]), int(g["degree"]))
    assert np.array_equal(B, g["bound"])                     # the bound is a-priori: a function of the inputs alone
    assert O.same_bits(model, g["model"])                    # no BLAS, no library reduction: the file's figures to the bit
    for s in range(model.shape[0]):
        err = error_to_digits(model[s, 3], g["mp_digits"][s, 3])
        print(f"{name}[{s}]: model {model[s, 3]:.17g}, mpmath {g['mp_digits'][s, 3]}, |diff| {err:.3e} = {err / B[s]:.2e} B")
        assert err <= B[s]
        assert abs(err - float(g["model_error"][s])) <= 2.0 ** -52 * abs(model[s, 3])
        # the three sums, each within its share of the same budget (the bound on mmd2 is the sum of theirs over m (m - 1) or m m)
        m = g["ia"].shape[1]
        for k, div in ((0, m * (m - 1)), (1, m * (m - 1)), (2, m * m / 2.0)):
            assert error_to_digits(model[s, k], g["mp_digits"][s, k]) / div <= B[s]


def test_gram_against_sklearn():
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    for name in ("m17_d5", "m40_d256_relu", "quadratic", "linear"):
        g = O.load(name)
        x, y = g["x"].astype(np.float64)[g["ia"][0]], g["y"].astype(np.float64)[g["ib"][0]]
        gamma, coef0, degree, d = float(g["gamma"]), float(g["coef0"]), int(g["degree"]), x.shape[1]
        K = O.kernel(O.dots(x, y), gamma, coef0, degree)
        want = pairwise.polynomial_kernel(x, y, degree=degree, gamma=gamma, coef0=coef0)
        scale = (abs(gamma) * (np.abs(x) @ np.abs(y).T) + abs(coef0)) ** degree
        # two evaluations inside the rules, each within B of the value at the scale of one element: s -> T_ij^p
        assert (np.abs(K - want) <= 2.0 * O.U * (degree * (d + 2) + O.chain(x.shape[0]) + 4) * scale).all()


@pytest.mark.parametrize("m,d", INTEGER_SHAPES)
def test_integer_cases_are_exact(m, d):
    gamma, den = O.integer_gamma(d)
    x, y = O.integer_features(m + 5, d, 7 * m + d), O.integer_features(m + 2, d, 11 * m + d)
    rng = np.random.RandomState(m)
    ia, ib = np.stack([rng.permutation(m + 5)[:m] for _ in range(2)]), np.stack([rng.permutation(m + 2)[:m] for _ in range(2)])
    sums, grams = O.integer_reference(x, y, ia, ib, den, 1, 3)
    got = O.evaluate(x, y, ia, ib, gamma, 1.0, 3)
    assert O.same_bits(got[:, :3], sums)
    assert O.same_bits(got[:, 3], [O.mmd2(*row, m) for row in sums])
    assert O.same_bits(O.kernel(O.dots(x[ia[0]], y[ib[0]]), gamma, 1.0, 3), grams[0])


def test_chain_and_weights():
    assert O.chain(2) == 16 + 8 + 1 + 8 and O.chain(64) == 33 and O.chain(65) == 33 and O.chain(1025) == 16 + 8 + 2 + 8
    assert O.chain(65536) == 16 + 8 + 4096 + 8
    rows, cols = O.element_maps()
    seen = set(zip(rows.reshape(-1).tolist(), cols.reshape(-1).tolist()))
    assert len(seen) == 64 * 64 and rows.min() == 0 and rows.max() == 63 and cols.max() == 63     # every element once


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/kid_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("kid") / "kid_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "kid_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_host(host_tool, tmp_path, x, y, ia, ib, gamma, coef0, degree):
    paths = []
    for key, arr, dt in (("x", x, np.float64), ("y", y, np.float64), ("ia", ia, np.int32), ("ib", ib, np.int32)):
        if arr is None:
            continue
        paths.append(str(tmp_path / f"{key}.raw"))
        np.ascontiguousarray(arr, dt).tofile(paths[-1])
    subsets, m = (1, min(len(x), len(y))) if ia is None else ia.shape
    args = [host_tool, str(len(x)), str(len(y)), str(x.shape[1]), str(subsets), str(m), str(degree), float(gamma).hex(), float(coef0).hex()]
    r = subprocess.run(args + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([[float(v) for v in line.split()] for line in r.stdout.decode().splitlines()])


@pytest.mark.parametrize("name", list(O.CASES))
def test_host_tool_gives_the_models_bits(host_tool, tmp_path, models, name):
    g, model = models[name]
    got = run_host(host_tool, tmp_path, g["x"], g["y"], g["ia"], g["ib"], float(g["gamma"]), float(g["coef0"]), int(g["degree"]))
    assert O.same_bits(got, model), (got, model)


def test_host_tool_without_lists_and_with_a_repeated_row(host_tool, tmp_path):
    x, y = O.integer_features(70, 5, 1), O.integer_features(66, 5, 2)
    ident = np.arange(66, dtype=np.int32)[None, :]
    got = run_host(host_tool, tmp_path, x, y, None, None, 1.0, 1.0, 3)
    assert O.same_bits(got, O.evaluate(x, y, ident, ident, 1.0, 1.0, 3))
    # the mask goes by position: row 4 twice in one list contributes k(x4, x4) twice to Sxx
    ia, ib = np.array([[4, 9, 4, 1]], np.int32), np.array([[0, 1, 2, 3]], np.int32)
    got = run_host(host_tool, tmp_path, x, y, ia, ib, 1.0, 1.0, 3)
    sums, _ = O.integer_reference(x, y, ia, ib, 1, 1, 3)
    assert O.same_bits(got[:, :3], sums)
    k44 = (int((x[4] * x[4]).sum()) + 1) ** 3                    # a mask by row number would drop these two entries
    assert k44 > 0 and got[0, 0] != sums[0, 0] - 2 * k44


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(3).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("2", "2", "2", "1", "2", "3", "0.5", "1", p, p)
    assert r.returncode == 2 and b"exactly" in r.stderr
    assert run("2", "2", "1", "1", "1", "3", "0.5", "1", p, p).returncode == 2                # m = 1
    assert run("2", "2", "1", "1", "3", "3", "0.5", "1", p, p).returncode == 2                # m above the rows, no lists
    assert run("2", "2", "1", "1", "2", "9", "0.5", "1", p, p).returncode == 2                # degree 9
    r = run("2")
    assert r.returncode == 2 and b"usage" in r.stderr
    q = str(tmp_path / "i.raw")
    np.array([0, 3], np.int32).tofile(q)
    r = run("3", "3", "1", "1", "2", "3", "0.5", "1", p, p, q, q)
    assert r.returncode == 2 and b"outside" in r.stderr


# ------------------------------------------------------------------------------------------------ draw_subsets
def test_draw_subsets_rule_and_golden():
    from rcdms_amd.kid import draw_subsets
    g = O.load("subsets3")
    ia, ib = draw_subsets(31, 45, 3, 19, 7)
    assert ia.dtype == np.int32 and ib.dtype == np.int32 and ia.shape == (3, 19)
    assert np.array_equal(ia, g["ia"]) and np.array_equal(ib, g["ib"])             # the draws are pinned by the file
    rng = np.random.RandomState(7)
    for s in range(3):
        assert np.array_equal(ia[s], rng.choice(31, 19, replace=False)) and np.array_equal(ib[s], rng.choice(45, 19, replace=False))
        assert len(set(ia[s].tolist())) == 19 and len(set(ib[s].tolist())) == 19   # without replacement
        assert ia[s].min() >= 0 and ia[s].max() < 31 and ib[s].max() < 45
    full, _ = draw_subsets(5, 9, 2, 5, 0)
    assert sorted(full[0].tolist()) == list(range(5))
    for bad in ((5, 9, 2, 6, 0), (9, 5, 2, 6, 0), (5, 5, 2, 1, 0), (5, 5, 0, 2, 0)):
        with pytest.raises(ValueError):
            draw_subsets(*bad)


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in NEW_SYMBOLS:
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.MmdDesc) == 72 and hip.MmdDesc.gamma.offset == 48 and hip.MmdDesc.flags.offset == 64
    assert lib.rcdm_version() == 0x000300


def test_argument_validation_without_gpu():
    """The entry points refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    F32 = hip.FSTATS_F32

    def desc(ldx=8, ldy=8, nx=10, ny=10, d=8, subsets=2, m=4, degree=3, dtype=F32, gamma=0.125, coef0=1.0, flags=0):
        return hip.MmdDesc(ldx, ldy, nx, ny, d, subsets, m, degree, dtype, gamma, coef0, flags)

    wsb = lambda dd: lib.rcdm_poly_mmd_workspace_bytes(ctypes.byref(dd))
    assert wsb(desc()) == 2 * 3 * 1 * 8 and wsb(desc(m=65, nx=70, ny=70)) == 2 * 3 * 4 * 8
    assert wsb(desc(m=65536, subsets=1, nx=65536, ny=65536)) == 3 * 1024 * 1024 * 8 and wsb(desc(d=4096, ldx=4096, ldy=4096)) > 0
    invalid = (desc(d=0), desc(m=1), desc(subsets=0), desc(nx=0), desc(ny=0), desc(ldx=7), desc(ldy=7), desc(degree=0), desc(degree=9),
               desc(dtype=7), desc(flags=1))
    shape = (desc(d=4097, ldx=4097, ldy=4097), desc(m=65537), desc(subsets=65536))
    for bad in invalid + shape:
        assert wsb(bad) == 0
    assert lib.rcdm_poly_mmd_workspace_bytes(None) == 0

    x, y, ix, iy, out, ws, st = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0          # never dereferenced
    mmd = lambda dd, *a: lib.rcdm_poly_mmd(ctypes.byref(dd), *a)
    good, nb = desc(), 48
    for bad in invalid:
        assert mmd(bad, x, y, ix, iy, out, ws, 1 << 20, st) == EINVAL
    for bad in shape:
        assert mmd(bad, x, y, ix, iy, out, ws, 1 << 30, st) == ESHAPE
    assert lib.rcdm_poly_mmd(None, x, y, ix, iy, out, ws, nb, st) == EINVAL
    for a in ((0, y, ix, iy, out), (x, 0, ix, iy, out), (x, y, ix, iy, 0)):                # null pointers
        assert mmd(good, *a, ws, nb, st) == EINVAL
    assert mmd(good, x + 2, y, ix, iy, out, ws, nb, st) == EINVAL                          # float32 rows at an odd half
    assert mmd(desc(dtype=hip.FSTATS_F16), x + 1, y, ix, iy, out, ws, nb, st) == EINVAL
    assert mmd(good, x, y, ix + 2, iy, out, ws, nb, st) == EINVAL and mmd(good, x, y, ix, iy + 1, out, ws, nb, st) == EINVAL
    assert mmd(good, x, y, ix, iy, out + 4, ws, nb, st) == EINVAL and mmd(good, x, y, ix, iy, out, ws + 4, nb, st) == EINVAL
    assert mmd(desc(nx=3), x, y, 0, iy, out, ws, nb, st) == EINVAL                         # rows 0 .. 3 of a set of 3
    assert mmd(desc(ny=3), x, y, ix, 0, out, ws, nb, st) == EINVAL
    assert mmd(good, x, y, ix, iy, out, 0, nb, st) == EWORKSPACE and mmd(good, x, y, ix, iy, out, ws, nb - 8, st) == EWORKSPACE

    gram = lambda dd, *a: lib.rcdm_poly_gram_f64(ctypes.byref(dd), *a)
    assert gram(good, x, y, ix, iy, out, 3, st) == EINVAL                                  # ldo < m
    assert gram(good, x, y, ix, iy, out + 4, 4, st) == EINVAL and gram(good, 0, y, ix, iy, out, 4, st) == EINVAL
    assert gram(desc(degree=9), x, y, ix, iy, out, 4, st) == EINVAL and gram(desc(m=65537), x, y, ix, iy, out, 1 << 17, st) == ESHAPE
    assert lib.rcdm_poly_gram_f64(None, x, y, ix, iy, out, 4, st) == EINVAL


def test_python_layer_refuses_before_any_device_access(tmp_path):
    import torch
    from rcdms_amd import hip
    from rcdms_amd.kid import FeatureBank, kernel_distance, polynomial_mmd
    with pytest.raises(hip.RcdmError):
        FeatureBank(8, "cpu")
    with pytest.raises(hip.RcdmError):
        FeatureBank(8, "cuda").append(torch.zeros(3, 8))
    with pytest.raises(TypeError):
        FeatureBank(8, "cuda").append(np.zeros((3, 8), np.float32))
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            FeatureBank(bad, "cuda")
    with pytest.raises(ValueError):
        FeatureBank(8, "cuda", dtype=torch.float64)
    bank = FeatureBank(8, "cuda")
    assert len(bank) == 0 and tuple(bank.rows().shape) == (0, 8)
    with pytest.raises(ValueError):
        bank.stats()
    with pytest.raises(ValueError, match="no rows"):
        kernel_distance(bank, bank)
    host = torch.zeros(6, 8)
    with pytest.raises(hip.RcdmError):
        kernel_distance(host, host)
    with pytest.raises(hip.RcdmError):
        polynomial_mmd(host, host)
    with pytest.raises(ValueError, match="above"):
        kernel_distance(host, torch.zeros(4, 8), subset_size=5)
    with pytest.raises(ValueError, match="at least 2"):
        kernel_distance(host, host, subset_size=1)
    with pytest.raises(ValueError, match="at least 2"):
        kernel_distance(host, torch.zeros(1, 8))                     # subset_size=None: min(1000, 6, 1)
    with pytest.raises(ValueError):
        kernel_distance(host, host, subsets=0)
    with pytest.raises(TypeError):
        kernel_distance(np.zeros((6, 8)), host)
    with pytest.raises(ValueError):
        kernel_distance(host, host, indices=(np.zeros((1, 3), np.int32),))
    np.savez(tmp_path / "bad.npz", features=np.zeros((3, 8)))
    with pytest.raises(ValueError):
        FeatureBank.load(tmp_path / "bad.npz", "cuda")
