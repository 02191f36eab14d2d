"""CPU: the pivoted-Cholesky route of the Fréchet distance before a GPU runs it.  The numpy model (tests/frechet_chol_oracle.py)
against the 60-digit goldens, old and new (tools/mint_frechet_chol_golden.py); exact answers on integer factors, where any
summation order must return the factor bit for bit; the shared core csrc/frechet_core.h compiled into tools/frechet_host.cpp,
which must take the model's pivots and give its bits; and the argument checks of the two new entry points, which need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import frechet_chol_oracle as C
from tests import frechet_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_cholesky_workspace_bytes", "rcdm_cholesky_pivoted_f64")
EXACT_D = (1, 2, 17, 33, 40, 70)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


@pytest.fixture(scope="module")
def models():
    """case -> (golden file, the Cholesky model's result on its moments), computed once."""
    out = {}
    for name in C.CASES:
        g = C.load(name)
        out[name] = (g, C.distance_from_moments(g["mu_a"], g["cov_a"], g["mu_b"], g["cov_b"]))
    return out


def test_new_cases_are_what_they_claim():
    g = {name: C.load(name) for name in C.NEW_CASES}
    assert g["illcond"]["xa"].shape == (256, 64) and g["illcond"]["xb"].shape == (256, 64)
    assert g["illcond_deficient"]["xa"].shape == (20, 48) and g["illcond_deficient"]["xb"].shape == (30, 48)
    assert g["illcond_deficient"]["chol_model_ranks"].tolist() == [19, 29]
    for key in ("cov_a", "cov_b"):
        lam = np.linalg.eigvalsh(g["illcond"][key])
        cond = lam[-1] / lam[0]
        print(f"illcond {key}: condition {cond:.2e}")
        assert 1e10 < cond < 1.0 / (64 * O.EPS) / 100.0          # ill-conditioned, and two decades inside the cut
        diag = np.diag(g["tie"][key])
        assert same_bits(diag[:3], diag[3:6]) and same_bits(diag[:3], diag[12:15]) and len(set(diag[:3].tolist())) == 3
    # the lowest index wins a tie: the five copies of the largest diagonal first, in ascending order, then the next value's
    assert g["tie"]["chol_pivots_a"].tolist()[:5] == list(range(int(np.argmax(np.diag(g["tie"]["cov_a"])[:3])), 15, 3))


@pytest.mark.parametrize("name", C.CASES)
def test_model_against_the_60_digit_value(models, name):
    g, m = models[name]
    d, s = g["mu_a"].shape[0], float(g["scale"])
    err = abs(m["distance"] - float(g["mp_distance"]))
    print(f"{name}: Cholesky model {m['distance']:.17g}, mpmath {float(g['mp_distance']):.17g}, |diff| {err:.3e} = "
          f"{err / (d * O.EPS * s):.2f} d eps s, sweeps {m['sweeps']}, ranks {m['rank_a']}/{m['rank_b']}, block {m['block']}")
    assert err <= O.budget(d, s, C.MODEL_ERROR[name])
    # float(mp value) is itself rounded: half an ulp of the distance
    assert err <= C.MODEL_ERROR[name] + abs(float(g["mp_distance"])) * O.EPS
    assert err <= 4.0 * d * O.EPS * s
    assert [m["rank_a"], m["rank_b"]] == g["model_ranks"].tolist()              # the Jacobi model's ranks, on all twelve
    assert m["sweeps"][:2] == (0, 0) and m["sweeps"][2] <= O.MAX_SWEEPS
    assert m["block"] == (m["rank_b"] + (m["rank_b"] & 1), m["rank_a"])
    if name in C.NEW_CASES:
        # deterministic: the file's figures are reproduced to the bit
        assert m["distance"] == float(g["chol_model_distance"]) and m["sqrt_trace"] == float(g["chol_model_sqrt_trace"])
        assert C.MODEL_ERROR[name] == float(g["chol_model_error"])
        assert [m["rank_a"], m["rank_b"]] == g["chol_model_ranks"].tolist()
        assert list(m["pivots"][0]) == g["chol_pivots_a"].tolist() and list(m["pivots"][1]) == g["chol_pivots_b"].tolist()
        assert m["counts"] == g["chol_model_counts_m"].tolist()


@pytest.mark.parametrize("name", O.CASES)
def test_the_two_models_agree(models, name):
    g, m = models[name]
    d, s = g["mu_a"].shape[0], float(g["scale"])
    assert abs(m["distance"] - float(g["model_distance"])) <= O.budget(d, s, C.MODEL_ERROR[name]) + O.budget(d, s, O.MODEL_ERROR[name])


@pytest.mark.parametrize("nb", C.PANELS)
@pytest.mark.parametrize("d", EXACT_D)
def test_model_exact_answers(d, nb):
    for name, sigma, want, rank in C.exact_cases(d):
        F, r, piv = C.pivoted_cholesky(sigma, nb)
        assert r == rank, (name, r, rank)
        assert same_bits(F, want), (name, np.argwhere(F != want)[:4])
        if name != "zero":
            assert piv == list(range(rank)), (name, piv)


def test_model_cut_and_hostile_diagonals():
    F, r, piv = C.pivoted_cholesky(np.diag([4.0, -1.0, np.nan, 9.0, 0.0]))
    assert r == 2 and piv == [3, 0] and same_bits(F[:, :2], np.array([[0, 2.0], [0, 0], [0, 0], [3.0, 0], [0, 0]])) and not F[:, 2:].any()
    F, r, piv = C.pivoted_cholesky(-np.eye(3))
    assert r == 0 and not F.any()
    # a diagonal exactly at d 2^-52 x the largest is cut, the next double above it is kept
    cut = 2 * O.EPS * 1.0
    assert C.pivoted_cholesky(np.diag([1.0, cut]))[1] == 1 and C.pivoted_cholesky(np.diag([1.0, np.nextafter(cut, 1.0)]))[1] == 2
    F, r, piv = C.pivoted_cholesky(C.tie_covariance())
    assert r == 15 and piv == [0, 3, 6, 9, 12, 1, 4, 7, 10, 13, 2, 5, 8, 11, 14]
    assert np.abs(F @ F.T - C.tie_covariance()).max() <= 4 * 15 * O.EPS * 4.0


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/frechet_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("frechet_chol") / "frechet_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "frechet_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def host_factor(host_tool, tmp_path, sigma, nb):
    """-> (F, rank, pivots) of the host program's --cholesky-factor mode."""
    d = sigma.shape[0]
    src, dst = str(tmp_path / "cov.raw"), str(tmp_path / "f.raw")
    np.ascontiguousarray(sigma, np.float64).tofile(src)
    r = subprocess.run([host_tool, "--cholesky-factor", str(d), str(nb), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    lines = r.stdout.decode().split("\n")
    return np.fromfile(dst, np.float64).reshape(d, d), int(lines[0]), [int(v) for v in lines[1].split()]


@pytest.mark.parametrize("name", C.CASES)
def test_host_tool_gives_the_models_factor(host_tool, tmp_path, models, name):
    g, m = models[name]
    for key, want_f, want_piv in zip(("cov_a", "cov_b"), m["factors"], m["pivots"]):
        F, rank, piv = host_factor(host_tool, tmp_path, g[key], C.NB)
        assert piv == list(want_piv) and rank == len(want_piv)
        assert same_bits(F, want_f), np.argwhere(F != want_f)[:4]


@pytest.mark.parametrize("nb", C.PANELS)
def test_host_tool_panel_widths_and_exact_answers(host_tool, tmp_path, models, nb):
    """Every panel width on a case that crosses panels with rounding in the trailing update (illcond, d 64, at nb 16 and 32), and the
    integer factors at sizes below, at and above a panel."""
    g, _ = models["illcond"]
    want_f, want_rank, want_piv = C.pivoted_cholesky(g["cov_a"], nb)
    F, rank, piv = host_factor(host_tool, tmp_path, g["cov_a"], nb)
    assert piv == want_piv and rank == want_rank and same_bits(F, want_f)
    for d in EXACT_D + (nb, nb + 1, 2 * nb):
        for name, sigma, want, want_rank in C.exact_cases(d):
            F, rank, piv = host_factor(host_tool, tmp_path, sigma, nb)
            assert rank == want_rank and same_bits(F, want), (d, name)
            assert name == "zero" or piv == list(range(rank))


@pytest.mark.parametrize("name", C.CASES)
def test_host_tool_distance(host_tool, tmp_path, models, name):
    g, m = models[name]
    d = g["mu_a"].shape[0]
    paths = []
    for key in ("mu_a", "cov_a", "mu_b", "cov_b"):
        paths.append(str(tmp_path / f"{key}.raw"))
        np.ascontiguousarray(g[key], np.float64).tofile(paths[-1])
    r = subprocess.run([host_tool, "--cholesky", str(d), *paths], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    lines = r.stdout.decode().split("\n")
    f = lines[0].split()
    got = [float(v) for v in f[:5]]
    assert got == [m["distance"], m["mean_term"], m["trace_a"], m["trace_b"], m["sqrt_trace"]], (got, m["distance"])
    assert [int(f[5]), int(f[6])] == [m["rank_a"], m["rank_b"]]
    assert [int(v) for v in lines[1].split()] == list(m["pivots"][0]) and [int(v) for v in lines[2].split()] == list(m["pivots"][1])
    assert [int(v) for v in lines[3].split()] == m["counts"]


def test_host_tool_refusals(host_tool, tmp_path):
    p, q = str(tmp_path / "x.raw"), str(tmp_path / "f.raw")
    np.zeros(3).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("--cholesky-factor", "2", "64", p, q)
    assert r.returncode == 2 and b"exactly" in r.stderr
    assert run("--cholesky-factor", "2", "48", p, q).returncode == 2 and run("--cholesky-factor", "0", "64", p, q).returncode == 2
    assert run("--cholesky", "2", p, p, p, p).returncode == 2
    assert not os.path.exists(q)


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
    assert ctypes.sizeof(hip.CholeskyDesc) == 24
    assert lib.rcdm_version() == 0x000300


def test_argument_validation_without_gpu():
    """The two entries refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    D = hip.CholeskyDesc                                            # (ld, ldf, d, nb)
    a, f, rank, ws, st = 0x1000, 0x2000, 0x3000, 0x4000, 0         # never dereferenced
    wsb = lambda desc: lib.rcdm_cholesky_workspace_bytes(ctypes.byref(desc))
    need = lambda d, nb: (8 + d * d + nb * d + 2 * d) * 8 + 2 * (d + (d & 1)) * 4
    assert wsb(D(8, 8, 8, 0)) == need(8, C.NB) and wsb(D(9, 10, 7, 32)) == need(7, 32) and wsb(D(4096, 4096, 4096, 128)) == need(4096, 128)
    for bad in (D(8, 8, 0, 0), D(7, 8, 8, 0), D(8, 7, 8, 0), D(8, 8, 8, 8), D(8, 8, 8, -1), D(8, 8, -3, 0), D(4097, 4097, 4097, 0)):
        assert wsb(bad) == 0
    assert lib.rcdm_cholesky_workspace_bytes(None) == 0
    run = lambda desc, *args: lib.rcdm_cholesky_pivoted_f64(ctypes.byref(desc), *args)
    good, nbytes = D(8, 8, 8, 0), need(8, C.NB)
    assert lib.rcdm_cholesky_pivoted_f64(None, a, f, rank, ws, nbytes, st) == EINVAL
    assert run(D(8, 8, 0, 0), a, f, rank, ws, nbytes, st) == EINVAL                       # d < 1
    assert run(D(7, 8, 8, 0), a, f, rank, ws, nbytes, st) == EINVAL                       # ld < d
    assert run(D(8, 7, 8, 0), a, f, rank, ws, nbytes, st) == EINVAL                       # ldf < d
    assert run(D(8, 8, 8, 48), a, f, rank, ws, 1 << 20, st) == EINVAL                     # no such panel width
    assert run(D(4097, 4097, 4097, 0), a, f, rank, ws, 1 << 40, st) == ESHAPE             # d > 4096
    for bad in ((0, f, rank), (a, 0, rank), (a, f, 0), (a + 4, f, rank), (a, f + 4, rank), (a, f, rank + 2)):
        assert run(good, *bad, ws, nbytes, st) == EINVAL                                  # null and misaligned pointers
    assert run(good, a, f, rank, ws + 4, nbytes, st) == EINVAL
    assert run(good, a, f, rank, 0, nbytes, st) == EWORKSPACE and run(good, a, f, rank, ws, nbytes - 8, st) == EWORKSPACE


def test_python_refuses_unknown_methods_and_the_host():
    from rcdms_amd import hip
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    a = FeatureStats(8, "cuda")
    with pytest.raises(ValueError, match="jacobi"):
        a.factor(method="qr")
    with pytest.raises(ValueError, match="cholesky"):
        frechet_distance(a, a, factor="eigh")
    with pytest.raises(ValueError):
        frechet_distance(a, a, factor="cholesky")                   # no rows yet: refused before any launch
    with pytest.raises(hip.RcdmError):
        FeatureStats(8, "cpu").factor(method="cholesky")
