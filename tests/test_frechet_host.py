"""CPU: the Fréchet distance before a GPU runs it.  The numpy model (tests/frechet_oracle.py) against the 60-digit goldens
(tools/mint_frechet_golden.py), a definition-level value through eigh / svd against the model, the shared core
csrc/frechet_core.h compiled into tools/frechet_host.cpp — it must take the model's rotations sweep for sweep and give its bits —
and the argument checks of the new entry points, which need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import frechet_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_feature_stats_update", "rcdm_gemm_tn_f64", "rcdm_feature_stats_finalize", "rcdm_frechet_trace",
               "rcdm_frechet_mean_term", "rcdm_jacobi_workspace_bytes", "rcdm_jacobi_sweep", "rcdm_jacobi_norm_sum",
               "rcdm_frechet_factor")


@pytest.fixture(scope="module")
def models():
    """case -> (golden file, the model's result on its features), computed once."""
    out = {}
    for name in O.CASES:
        g = O.load(name)
        out[name] = (g, O.distance(g["xa"], g["xb"]))
    return out


def test_cases_cover_the_edges():
    shapes = {name: O.load(name) for name in O.CASES}
    d = {name: g["xa"].shape[1] for name, g in shapes.items()}
    n = {name: (g["xa"].shape[0], g["xb"].shape[0]) for name, g in shapes.items()}
    assert d["d1"] == 1 and d["d2_n2"] == 2 and n["d2_n2"] == (2, 2) and d["d31_odd"] == 31 and d["d48_full"] == 48
    assert n["n_lt_d_one"][0] < d["n_lt_d_one"] <= n["n_lt_d_one"][1]
    assert max(n["n_lt_d_both"]) < d["n_lt_d_both"]
    assert np.array_equal(shapes["self"]["xa"], shapes["self"]["xb"])
    assert tuple(shapes["d48_full"]["model_ranks"]) == (48, 48)


@pytest.mark.parametrize("name", O.CASES)
def test_model_against_the_60_digit_value(models, name):
    g, m = models[name]
    d, s = g["xa"].shape[1], float(g["scale"])
    err = abs(m["distance"] - float(g["mp_distance"]))
    print(f"{name}: model {m['distance']:.17g}, mpmath {float(g['mp_distance']):.17g}, |diff| {err:.3e} = {err / (d * O.EPS * s):.2f} d eps s, "
          f"sweeps {m['sweeps']}, ranks {m['rank_a']}/{m['rank_b']}")
    # the model is deterministic (no BLAS, no library reduction): the file's figures are reproduced to the bit
    assert m["distance"] == float(g["model_distance"]) and m["sqrt_trace"] == float(g["model_sqrt_trace"])
    assert [m["rank_a"], m["rank_b"]] == g["model_ranks"].tolist()
    assert O.MODEL_ERROR[name] == float(g["model_error"])
    # float(mp value) is itself rounded: half an ulp of the distance
    assert err <= O.MODEL_ERROR[name] + abs(float(g["mp_distance"])) * O.EPS
    assert err <= 4.0 * d * O.EPS * s
    assert max(m["sweeps"]) <= O.MAX_SWEEPS
    if name == "self":
        assert abs(m["distance"]) <= O.budget(d, s, O.MODEL_ERROR[name])


@pytest.mark.parametrize("name", O.CASES)
def test_definition_against_the_model(models, name):
    g, m = models[name]
    d, s = g["xa"].shape[1], float(g["scale"])
    want = O.distance_definition(g["mu_a"], g["cov_a"], g["mu_b"], g["cov_b"])
    err = abs(want - m["distance"])
    print(f"{name}: eigh / svd {want:.17g}, |diff to the model| {err:.3e} = {err / (d * O.EPS * s):.2f} d eps s")
    # two float64 routes to one number, each within 4 d eps s of it
    assert err <= 8.0 * d * O.EPS * s
    try:
        root = O.distance_sqrtm(g["mu_a"], g["cov_a"], g["mu_b"], g["cov_b"])
        print(f"  sqrtm route: off by {abs(root - float(g['mp_distance'])) / s:.1e} s (comparison only)")
    except ImportError:
        pass


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/frechet_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("frechet") / "frechet_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "frechet_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


@pytest.mark.parametrize("name", O.CASES)
def test_host_tool_takes_the_models_rotations(host_tool, tmp_path, models, name):
    g, m = models[name]
    d = g["xa"].shape[1]
    paths = []
    for key in ("mu_a", "cov_a", "mu_b", "cov_b"):
        paths.append(str(tmp_path / f"{key}.raw"))
        np.ascontiguousarray(g[key], np.float64).tofile(paths[-1])
    r = subprocess.run([host_tool, str(d), *paths], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 4
    f = lines[0].split()
    got = [float(v) for v in f[:5]]
    assert got == [m["distance"], m["mean_term"], m["trace_a"], m["trace_b"], m["sqrt_trace"]], (got, m)
    assert [int(f[5]), int(f[6])] == [m["rank_a"], m["rank_b"]]
    for line, counts, key in zip(lines[1:], m["counts"], ("model_counts_a", "model_counts_b", "model_counts_m")):
        assert [int(v) for v in line.split()] == counts == g[key].tolist()


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(3).tofile(p)
    r = subprocess.run([host_tool, "2", p, p, p, p], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"exactly" in r.stderr
    r = subprocess.run([host_tool, "0", p, p, p, p], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2
    r = subprocess.run([host_tool, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"usage" in r.stderr


def test_round_robin_meets_every_pair_once(host_tool):
    """fr::pair of the core header, through the host program: every round touches every row once, every pair meets once per
    sweep, and the numpy model pairs the same rows in the same places."""
    for rows in (2, 4, 18, 32, 50):
        r = subprocess.run([host_tool, "--pairs", str(rows)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        rounds = [[tuple(int(v) for v in pq.split(":")) for pq in line.split()] for line in r.stdout.decode().splitlines()]
        assert len(rounds) == rows - 1
        seen = set()
        for rnd, got in enumerate(rounds):
            assert len(got) == rows // 2 and all(0 <= p < q < rows for p, q in got)
            assert len({v for pq in got for v in pq}) == rows           # disjoint: a round touches every row once
            p, q = O.pairs(rows, rnd)
            assert got == list(zip(p.tolist(), q.tolist()))
            seen |= set(got)
        assert len(seen) == rows * (rows - 1) // 2
    r = subprocess.run([host_tool, "--pairs", "7"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"even" in r.stderr


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
    assert ctypes.sizeof(hip.FStatsDesc) == 24 and ctypes.sizeof(hip.JacobiDesc) == 24
    assert lib.rcdm_version() == 0x000300


def test_argument_validation_without_gpu():
    """The entry points refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    x, k, s, o, st = 0x1000, 0x2000, 0x3000, 0x4000, 0          # never dereferenced
    upd = lambda desc, *a: lib.rcdm_feature_stats_update(ctypes.byref(desc), *a)
    ok = (x, k, s, o, st)
    assert upd(hip.FStatsDesc(8, 4, 0, hip.FSTATS_F32, 0), *ok) == EINVAL                  # d = 0
    assert upd(hip.FStatsDesc(8, 0, 8, hip.FSTATS_F32, 0), *ok) == EINVAL                  # n = 0
    assert upd(hip.FStatsDesc(7, 4, 8, hip.FSTATS_F32, 0), *ok) == EINVAL                  # ld < d
    assert upd(hip.FStatsDesc(8, 4, 8, 7, 0), *ok) == EINVAL                               # unknown dtype
    assert upd(hip.FStatsDesc(4097, 4, 4097, hip.FSTATS_F32, 0), *ok) == ESHAPE            # d > 4096
    good = hip.FStatsDesc(8, 4, 8, hip.FSTATS_F32, 0)
    for bad in ((0, k, s, o, st), (x, 0, s, o, st), (x, k, 0, o, st), (x, k, s, 0, st)):   # null pointers
        assert upd(good, *bad) == EINVAL
    assert upd(good, x, k, s + 4, o, st) == EINVAL and upd(good, x, k, s, o + 4, st) == EINVAL      # misaligned float64
    assert upd(good, x + 2, k, s, o, st) == EINVAL                                         # float32 rows at an odd half
    assert lib.rcdm_feature_stats_update(None, *ok) == EINVAL

    gemm = lib.rcdm_gemm_tn_f64
    assert gemm(0, 4, 4, x, 4, k, 4, s, 4, st) == EINVAL and gemm(4, 4, 4, x, 3, k, 4, s, 4, st) == EINVAL
    assert gemm(4, 4, 4, x, 4, k, 4, s, 3, st) == EINVAL and gemm(4, 4, 4, 0, 4, k, 4, s, 4, st) == EINVAL
    assert gemm(4, 4, 4, x + 4, 4, k, 4, s, 4, st) == EINVAL and gemm(4097, 4, 4, x, 4097, k, 4, s, 4, st) == ESHAPE

    fin = lib.rcdm_feature_stats_finalize
    assert fin(0, 5, k, s, o, x, 0x5000, 0x6000, st) == EINVAL and fin(8, 0, k, s, o, x, 0x5000, 0x6000, st) == EINVAL
    assert fin(8, 1, k, s, o, x, 0x5000, 0x6000, st) == EINVAL                             # a covariance of one row
    assert fin(8, 5, k, s, o, x + 4, 0x5000, 0x6000, st) == EINVAL and fin(8, 5, 0, s, o, x, 0x5000, 0x6000, st) == EINVAL
    assert fin(4097, 5, k, s, o, x, 0x5000, 0x6000, st) == ESHAPE
    assert lib.rcdm_frechet_trace(0, x, s, st) == EINVAL and lib.rcdm_frechet_trace(4, x + 4, s, st) == EINVAL
    assert lib.rcdm_frechet_trace(4097, x, s, st) == ESHAPE
    assert lib.rcdm_frechet_mean_term(4, x, 0, s, st) == EINVAL and lib.rcdm_frechet_mean_term(4, x, k + 4, s, st) == EINVAL
    assert lib.rcdm_frechet_mean_term(4097, x, k, s, st) == ESHAPE

    J = hip.JacobiDesc
    wsb = lambda desc: lib.rcdm_jacobi_workspace_bytes(ctypes.byref(desc))
    assert wsb(J(8, 8, 8, 8, 0)) == (4 + 8) * 8 and wsb(J(4096, 4096, 4096, 4095, 0)) == (4 + 4096) * 8
    for bad in (J(8, 7, 8, 8, 0), J(8, 0, 8, 8, 0), J(7, 8, 8, 8, 0), J(8, 8, 0, 8, 0), J(8, 8, 8, 0, 0), J(4098, 4098, 4098, 4098, 0),
                J(4097, 8, 4097, 8, 0), J(8, 8, 8, 4097, 0)):
        assert wsb(bad) == 0
    assert lib.rcdm_jacobi_workspace_bytes(None) == 0
    good = J(8, 8, 8, 8, 0)
    w, cnt, ws, nb = 0x1000, 0x2000, 0x3000, (4 + 8) * 8
    sweep = lambda desc, *a: lib.rcdm_jacobi_sweep(ctypes.byref(desc), *a)
    assert sweep(J(8, 7, 8, 8, 0), w, cnt, ws, nb, st) == EINVAL and sweep(J(7, 8, 8, 8, 0), w, cnt, ws, nb, st) == EINVAL
    assert sweep(J(4098, 4098, 4098, 4096, 0), w, cnt, ws, 1 << 20, st) == ESHAPE
    assert sweep(good, 0, cnt, ws, nb, st) == EINVAL and sweep(good, w, 0, ws, nb, st) == EINVAL
    assert sweep(good, w + 4, cnt, ws, nb, st) == EINVAL and sweep(good, w, cnt, ws + 4, nb, st) == EINVAL
    assert sweep(good, w, cnt, 0, nb, st) == EWORKSPACE and sweep(good, w, cnt, ws, nb - 8, st) == EWORKSPACE
    nsum = lambda desc, *a: lib.rcdm_jacobi_norm_sum(ctypes.byref(desc), *a)
    assert nsum(good, w, 0, ws, nb, st) == EINVAL and nsum(good, w, cnt + 4, ws, nb, st) == EINVAL
    assert nsum(good, w, cnt, ws, nb - 8, st) == EWORKSPACE
    fac = lambda desc, *a: lib.rcdm_frechet_factor(ctypes.byref(desc), *a)
    assert fac(good, w, 0, 8, cnt, ws, nb, st) == EINVAL and fac(good, w, 0x5000, 7, cnt, ws, nb, st) == EINVAL      # ldf < rows
    assert fac(good, w, 0x5004, 8, cnt, ws, nb, st) == EINVAL and fac(good, w, 0x5000, 8, 0, ws, nb, st) == EINVAL
    assert fac(good, w, 0x5000, 8, cnt, 0, nb, st) == EWORKSPACE


def test_feature_stats_refuse_the_host():
    import torch
    from rcdms_amd import hip
    from rcdms_amd.frechet import FeatureStats
    with pytest.raises(hip.RcdmError):
        FeatureStats(8, "cpu")
    with pytest.raises(hip.RcdmError):
        FeatureStats(8, "cuda").update(torch.zeros(3, 8))
    with pytest.raises(ValueError):
        FeatureStats(0, "cuda")
    with pytest.raises(ValueError):
        FeatureStats(4097, "cuda")
    with pytest.raises(ValueError):
        FeatureStats(8, "cuda").cov()
