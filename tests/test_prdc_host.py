"""CPU: the manifold figures before a GPU runs them.  The numpy model (tests/prdc_oracle.py) against the goldens
(tools/mint_prdc_golden.py): counts equal, radii within the a-priori bound of the 60-digit values; against scikit-learn's
neighbours and pairwise distances; integer cases against Python-int arithmetic bit for bit, with ties at the radius (which pin
`<=`) and a repeated row (which pins exclusion by position); the three mistakes a kernel could make each change a count on every
integer shape the GPU test uses; the shared core csrc/prdc_core.h compiled into tools/prdc_host.cpp — it must give the model's
bits —; the closed forms; and the argument checks of the new entry points and of the Python layer, which need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import prdc_oracle as O
from tests.test_cabi_symbols import declared_symbols
from tests.test_kid_host import error_to_digits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_row_norms2_f64", "rcdm_knn_radii2_workspace_bytes", "rcdm_knn_radii2", "rcdm_prdc_counts_workspace_bytes",
               "rcdm_prdc_counts")


@pytest.fixture(scope="module")
def models():
    """case -> (golden file, the model's result on its features), computed once."""
    out = {}
    for name in O.CASES:
        g = O.load(name)
        out[name] = (g, O.evaluate(g["x"], g["y"], int(g["k"])))
    return out


def test_cases_cover_the_edges():
    g = {name: O.load(name) for name in O.CASES}
    shape = {name: (v["x"].shape[0], v["y"].shape[0], v["x"].shape[1], int(v["k"])) for name, v in g.items()}
    assert shape["n17_23_d5_k3"] == (17, 23, 5, 3) and shape["n33_40_d48_k5"] == (33, 40, 48, 5)
    assert shape["n65_70_d130_k5"] == (65, 70, 130, 5) and shape["n300_300_d256_k5"] == (300, 300, 256, 5)
    assert shape["k1"][3] == 1 and shape["k16"][3] == 16
    for k in ("x", "y"):
        assert np.array_equal(g["f16"][k].astype(np.float16).astype(np.float32), g["f16"][k])
        assert g["relu"][k].min() >= 0 and (g["relu"][k] == 0).any()
    assert np.array_equal(g["self"]["x"], g["self"]["y"]) and int(g["self"]["margin_safe"]) == 0
    diff = g["mean_offset"]["y"].astype(np.float64) - g["mean_offset"]["x"].astype(np.float64)
    assert (diff == diff[0]).all() and np.ptp(diff[0]) > 0
    assert tuple(g["clusters"]["counts"]) == (0, 0, 0, 0)
    for name, v in g.items():
        assert int(v["margin_safe"]) == (0 if name == "self" else 1) and float(v["worst_margin"]) > 1.0
        for key in ("x", "y"):                               # on the grid: the file's integers are exact
            q = v[key].astype(np.float64) * 2.0 ** int(v["grid"])
            assert np.array_equal(q, np.round(q))
        assert os.path.getsize(os.path.join(O.GOLDEN, f"prdc_{name}.npz")) < 1 << 19


@pytest.mark.parametrize("name", list(O.CASES))
def test_model_against_the_goldens(models, name):
    g, model = models[name]
    assert np.array_equal(O.radius_bound(g["x"]), g["bound_real"]) and np.array_equal(O.radius_bound(g["y"]), g["bound_fake"])
    for key in ("counts", "fake_count", "real_hit"):
        assert np.array_equal(model[key], g[key]), key
    for key, digits, B in (("radii2_real", g["radii2_real_digits"], g["bound_real"]), ("radii2_fake", g["radii2_fake_digits"], g["bound_fake"])):
        assert O.same_bits(model[key], g["model_" + key])          # no BLAS, no library reduction: the file's figures to the bit
        err = np.array([error_to_digits(v, s) for v, s in zip(model[key], digits)])
        print(f"{name} {key}: largest |diff| {err.max():.3e}, largest share of its bound {(err / B).max():.2e}")
        assert (err <= B).all()
        assert (np.abs(g[key] - np.array([float(s) for s in digits])) <= 2.0 ** -52 * g[key]).all()     # the exact float64 and the digits agree
    assert O.same_bits(model["real_min2"], g["model_real_min2"])
    assert (np.abs(model["real_min2"] - g["real_min2"]) <= g["bound_min2"]).all()


def test_model_against_sklearn():
    neighbors = pytest.importorskip("sklearn.neighbors")
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    for name in O.CASES:
        g = O.load(name)
        x, y, k = g["x"].astype(np.float64), g["y"].astype(np.float64), int(g["k"])
        model = O.evaluate(x, y, k)
        radii = {}
        for key, z in (("radii2_real", x), ("radii2_fake", y)):
            dist, _ = neighbors.NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(z).kneighbors(z)      # the row itself first
            radii[key] = dist[:, k] ** 2
            B = O.radius_bound(z)
            # sklearn takes a square root and the test squares it again: two more roundings of the value on top of its own D2
            assert (np.abs(radii[key] - model[key]) <= 2.0 * B + 4.0 * 2.0 ** -53 * model[key]).all(), (name, key)
        if not int(g["margin_safe"]):
            continue
        D = pairwise.pairwise_distances(x, y, metric="sqeuclidean")
        got = O.figures(D, radii["radii2_real"], radii["radii2_fake"])
        for key in ("counts", "fake_count", "real_hit"):
            assert np.array_equal(got[key], g[key]), (name, key)


@pytest.mark.parametrize("shape", O.INTEGER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_are_exact_and_tell_the_mistakes_apart(shape):
    nx, ny, d, k = shape
    x, y = O.integer_pair(nx, ny, d)
    assert x.min() >= -3 and x.max() <= 3 and y.min() >= -3 and y.max() <= 3
    want = O.integer_reference(x, y, k)
    assert O.same_result(O.evaluate(x, y, k), want)
    # ties at the radius exist on every shape, so the closed ball matters; so do the masks
    assert not np.array_equal(O.evaluate(x, y, k, strict=True)["counts"], want["counts"])
    assert not np.array_equal(O.evaluate(x, y, k, zero_rows=1)["counts"], want["counts"])
    assert not np.array_equal(O.evaluate(x, y, k, strict_coverage=True)["counts"], want["counts"])


def test_ties_and_a_repeated_row():
    # one dimension, points 0 1 2 4: k = 1 radii are 1 1 1 4 (squared); the fake point 3 is at squared distance 1 of real 2
    # and of real 4: a tie with r2 = 1 of real 2, which only the closed ball counts (the fake radii are 49 4 4: every real row is hit)
    x, y = np.array([[0], [1], [2], [4]]), np.array([[3], [10], [12]])
    r = O.integer_reference(x, y, 1)
    assert r["radii2_real"].tolist() == [1, 1, 1, 4] and r["fake_count"].tolist() == [2, 0, 0] and r["counts"].tolist() == [1, 4, 2, 2]
    assert O.same_result(O.evaluate(x, y, 1), r)
    assert O.evaluate(x, y, 1, strict=True)["counts"].tolist() == [1, 4, 1, 1]
    # a repeated row: by position the twin is a neighbour at distance 0; exclusion by value would give radius 1 and 4
    x = np.array([[0], [0], [1], [3]])
    r = O.integer_reference(x, y, 1)
    assert r["radii2_real"].tolist() == [0, 0, 1, 4]
    assert O.same_result(O.evaluate(x, y, 1), r)
    three = np.array([[5, 5], [0, 1], [5, 5], [2, 2], [5, 5]])
    assert O.integer_reference(three, three, 2)["radii2_real"][[0, 2, 4]].tolist() == [0, 0, 0]
    assert O.same_result(O.evaluate(three, three, 2), O.integer_reference(three, three, 2))


def test_closed_forms(models):
    for name in ("n33_40_d48_k5", "self", "k16"):
        g, _ = models[name]
        k, n = int(g["k"]), len(g["x"])
        own = O.evaluate(g["x"], g["x"], k)
        p, r, dens, c = O.ratios(own["counts"], n, n, k)
        assert (p, r, c) == (1.0, 1.0, 1.0) and dens == (k + 1) / k          # no ties: every ball holds its centre and k more
    g, model = models["clusters"]
    assert O.ratios(model["counts"], len(g["x"]), len(g["y"]), int(g["k"])) == (0.0, 0.0, 0.0, 0.0)
    assert (model["fake_count"] == 0).all() and (model["real_hit"] == 0).all()


def test_bound_is_a_priori_and_holds_on_random_rows():
    from fractions import Fraction
    rng = np.random.RandomState(3)
    x, y = rng.standard_normal((9, 37)).astype(np.float32), (rng.standard_normal((7, 37)) * 3).astype(np.float32)
    D = O.dist2(O.norms2(x), O.norms2(y), O.dots(x, y))
    B = O.bound(x, y)
    for i in range(9):
        for j in range(7):
            exact = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(x[i], y[j]))
            assert abs(Fraction(float(D[i, j])) - exact) <= Fraction(float(B[i, j]))


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/prdc_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("prdc") / "prdc_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "prdc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_host(host_tool, tmp_path, x, y, k, chunks):
    px, py = str(tmp_path / "x.raw"), str(tmp_path / "y.raw")
    np.ascontiguousarray(x, np.float64).tofile(px)
    np.ascontiguousarray(y, np.float64).tofile(py)
    r = subprocess.run([host_tool, str(len(x)), str(len(y)), str(x.shape[1]), str(k), str(chunks), px, py], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    out = {}
    for line in r.stdout.decode().splitlines():
        key, *vals = line.split()
        out[key] = np.array([float(v) for v in vals])
    for key, dt in (("counts", np.int64), ("fake_count", np.int32), ("real_hit", np.int32)):
        out[key] = out[key].astype(dt)
    return out


@pytest.mark.parametrize("name", [n for n in O.CASES if n != "n300_300_d256_k5"])
def test_host_tool_gives_the_models_bits(host_tool, tmp_path, models, name):
    g, model = models[name]
    for chunks in (0, 2):
        assert O.same_result(run_host(host_tool, tmp_path, g["x"], g["y"], int(g["k"]), chunks), model), chunks


def test_host_tool_on_integers_and_across_chunks(host_tool, tmp_path):
    for nx, ny, d, k in O.INTEGER_SHAPES[:5]:
        x, y = O.integer_pair(nx, ny, d)
        want = O.integer_reference(x, y, k)
        for chunks in (1, 3):                                    # 3: more chunks than tile columns
            assert O.same_result(run_host(host_tool, tmp_path, x, y, k, chunks), want), (nx, ny, d, k, chunks)
    rng = np.random.RandomState(0)                               # rounded dots, three tile columns
    x, y = rng.standard_normal((130, 33)).astype(np.float32), rng.standard_normal((70, 33)).astype(np.float32)
    want = O.evaluate(x, y, 5)
    for chunks in (0, 1, 2, 5):
        assert O.same_result(run_host(host_tool, tmp_path, x, y, 5, chunks), want)


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(7).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("4", "4", "2", "3", "0", p, p)
    assert r.returncode == 2 and b"exactly" in r.stderr
    assert run("3", "4", "2", "3", "0", p, p).returncode == 2                 # nx = k
    assert run("4", "4", "2", "0", "0", p, p).returncode == 2 and run("20", "20", "2", "17", "0", p, p).returncode == 2
    assert run("4", "4", "2", "3", "1025", p, p).returncode == 2 and run("4", "4", "4097", "3", "0", p, p).returncode == 2
    r = run("2")
    assert r.returncode == 2 and b"usage" in r.stderr


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
    assert ctypes.sizeof(hip.KnnDesc) == 32 and hip.KnnDesc.k.offset == 16 and hip.KnnDesc.flags.offset == 28
    assert ctypes.sizeof(hip.PrdcDesc) == 40 and hip.PrdcDesc.nx.offset == 16 and hip.PrdcDesc.flags.offset == 36
    assert (hip.PRDC_MAX_K, hip.PRDC_MAX_N) == (O.MAX_K, O.MAX_N)
    assert lib.rcdm_version() == 0x000300
    header = open(os.path.join(ROOT, "include", "rcdm.h")).read()
    for words in ("Manifold figures", "closed (<=)", "BY\n *               POSITION", "compares strictly"):
        assert words in header, words


def test_argument_validation_without_gpu():
    """The entry points refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    F32 = hip.FSTATS_F32

    def knn(ld=8, n=10, d=8, k=3, dtype=F32, col_chunks=2, flags=0):
        return hip.KnnDesc(ld, n, d, k, dtype, col_chunks, flags)

    kws = lambda dd: lib.rcdm_knn_radii2_workspace_bytes(ctypes.byref(dd))
    assert kws(knn()) == (10 + 2 * 10 * 3) * 8 and kws(knn(col_chunks=0)) == (10 + 10 * 3) * 8        # one tile column: one chunk
    assert kws(knn(n=300, col_chunks=0)) == (300 + 5 * 300 * 3) * 8                                    # five tile columns, all used
    assert kws(knn(n=10000, col_chunks=0)) == (10000 + 14 * 10000 * 3) * 8                             # 157 strips: 14 chunks, 2198 workgroups
    assert kws(knn(n=65536, k=16, col_chunks=0)) == (65536 + 2 * 65536 * 16) * 8 and kws(knn(d=4096, ld=4096)) > 0
    k_invalid = (knn(d=0), knn(n=0), knn(ld=7), knn(k=0), knn(k=17, n=40), knn(n=3), knn(col_chunks=-1), knn(col_chunks=1025),
                 knn(dtype=7), knn(flags=1))
    k_shape = (knn(d=4097, ld=4097), knn(n=65537))
    for bad in k_invalid + k_shape:
        assert kws(bad) == 0
    assert lib.rcdm_knn_radii2_workspace_bytes(None) == 0

    x, y, r2, ws, st = 0x1000, 0x2000, 0x3000, 0x6000, 0                                              # never dereferenced
    call = lambda dd, *a: lib.rcdm_knn_radii2(ctypes.byref(dd), *a)
    good, nb = knn(), (10 + 60) * 8
    for bad in k_invalid:
        assert call(bad, x, r2, ws, 1 << 30, st) == EINVAL
    for bad in k_shape:
        assert call(bad, x, r2, ws, 1 << 40, st) == ESHAPE
    assert lib.rcdm_knn_radii2(None, x, r2, ws, nb, st) == EINVAL
    assert call(good, 0, r2, ws, nb, st) == EINVAL and call(good, x, 0, ws, nb, st) == EINVAL
    assert call(good, x + 2, r2, ws, nb, st) == EINVAL and call(knn(dtype=hip.FSTATS_F16), x + 1, r2, ws, nb, st) == EINVAL
    assert call(good, x, r2 + 4, ws, nb, st) == EINVAL and call(good, x, r2, ws + 4, nb, st) == EINVAL
    assert call(good, x, r2, 0, nb, st) == EWORKSPACE and call(good, x, r2, ws, nb - 8, st) == EWORKSPACE

    def cnt(ldx=8, ldy=8, nx=10, ny=12, d=8, dtype=F32, col_chunks=2, flags=0):
        return hip.PrdcDesc(ldx, ldy, nx, ny, d, dtype, col_chunks, flags)

    cws = lambda dd: lib.rcdm_prdc_counts_workspace_bytes(ctypes.byref(dd))
    assert cws(cnt()) == (10 + 12 + 2 * 10) * 8 + 4 * 8 + 2 * 10 * 4 + 16                              # 12 bytes of column counts -> 16
    assert cws(cnt(nx=65536, ny=65536, col_chunks=0)) > 0
    c_invalid = (cnt(d=0), cnt(nx=0), cnt(ny=0), cnt(ldx=7), cnt(ldy=7), cnt(col_chunks=-1), cnt(col_chunks=1025), cnt(dtype=7),
                 cnt(flags=1))
    c_shape = (cnt(d=4097, ldx=4097, ldy=4097), cnt(nx=65537), cnt(ny=65537))
    for bad in c_invalid + c_shape:
        assert cws(bad) == 0
    assert lib.rcdm_prdc_counts_workspace_bytes(None) == 0
    rx, ry, out, fc, rh, rm = 0x3000, 0x4000, 0x5000, 0x7000, 0x8000, 0x9000
    call = lambda dd, *a: lib.rcdm_prdc_counts(ctypes.byref(dd), *a)
    good, nb = cnt(), cws(cnt())
    ptrs = (x, y, rx, ry, out, fc, rh, rm)
    for bad in c_invalid:
        assert call(bad, *ptrs, ws, 1 << 30, st) == EINVAL
    for bad in c_shape:
        assert call(bad, *ptrs, ws, 1 << 40, st) == ESHAPE
    assert lib.rcdm_prdc_counts(None, *ptrs, ws, nb, st) == EINVAL
    for i in range(8):                                                                                 # every pointer: null, then misaligned
        a = list(ptrs)
        a[i] = 0
        assert call(good, *a, ws, nb, st) == EINVAL, i
        a[i] = ptrs[i] + 2
        assert call(good, *a, ws, nb, st) == EINVAL, i
    assert call(good, *ptrs, ws + 4, nb, st) == EINVAL
    assert call(good, *ptrs, 0, nb, st) == EWORKSPACE and call(good, *ptrs, ws, nb - 8, st) == EWORKSPACE

    norms = lib.rcdm_row_norms2_f64
    assert norms(0, 4, 8, 8, F32, out, st) == EINVAL and norms(x, 4, 8, 8, F32, 0, st) == EINVAL
    assert norms(x, 0, 8, 8, F32, out, st) == EINVAL and norms(x, 4, 0, 8, F32, out, st) == EINVAL and norms(x, 4, 8, 7, F32, out, st) == EINVAL
    assert norms(x, 4, 8, 8, 7, out, st) == EINVAL and norms(x + 2, 4, 8, 8, F32, out, st) == EINVAL and norms(x, 4, 8, 8, F32, out + 4, st) == EINVAL
    assert norms(x, 4, 4097, 4097, F32, out, st) == ESHAPE and norms(x, 65537, 8, 8, F32, out, st) == ESHAPE


def test_python_layer_refuses_before_any_device_access():
    import torch
    from rcdms_amd import hip
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.prdc import PrdcResult, knn_radii2, manifold_metrics
    host = torch.zeros(8, 6)
    with pytest.raises(hip.RcdmError):
        manifold_metrics(host, host)
    with pytest.raises(hip.RcdmError):
        knn_radii2(host, 3)
    with pytest.raises(TypeError):
        manifold_metrics(np.zeros((8, 6), np.float32), host)
    for bad in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError, match="nearest_k"):
            manifold_metrics(host, host, nearest_k=bad)
        with pytest.raises(ValueError, match="nearest_k"):
            knn_radii2(host, bad)
    with pytest.raises(ValueError, match="at least"):
        manifold_metrics(host, host, nearest_k=8)                     # 8 rows at k = 8
    with pytest.raises(ValueError, match="at least"):
        manifold_metrics(torch.zeros(9, 6), torch.zeros(5, 6))        # the default k = 5 needs 6 rows
    with pytest.raises(ValueError, match="float32 or float16"):
        manifold_metrics(host.double(), host)
    with pytest.raises(ValueError, match=r"\(n, d\)"):
        knn_radii2(torch.zeros(8), 3)
    with pytest.raises(ValueError, match="d is"):
        knn_radii2(torch.zeros(8, 4097), 3)
    with pytest.raises(ValueError, match="at most"):
        knn_radii2(torch.zeros(65537, 1), 3)
    bank = FeatureBank(6, "cuda")
    with pytest.raises(ValueError, match="no rows"):
        manifold_metrics(bank, bank)
    with pytest.raises(ValueError, match="at least"):
        bank.radii2(3)                                                # an empty bank
    with pytest.raises(ValueError, match="nearest_k"):
        bank.radii2(0)
    assert bank._radii2 == {}
    assert [f for f in PrdcResult.__dataclass_fields__] == ["precision", "recall", "density", "coverage", "counts", "n_real", "n_fake",
                                                            "nearest_k", "fake_count", "real_hit", "real_min2", "radii2_real",
                                                            "radii2_fake"]
