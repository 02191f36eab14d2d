"""CPU: which tile variant and split-K factor the library picks for a GEMM / conv3x3, pinned over the whole decision surface.

The query entry points (plan_query, workspace_bytes, stat_parts, lnx_parts_ok, gnstat_ok, up2_supported) need no device:
sweep() drives them over a fixed grid — the step's own shapes plus the prior's and the encoders', which include every row of
the shape-rule table — and a fixed subset of the grid is repeated under every process-wide switch state (setters in this
process, environment switches in fresh child processes).  The answers must equal tests/golden/igemm_plan.npz exactly.

The fixture is recorded from the PARENT of a change to the planner, never from the code under test: build the parent commit
elsewhere and run `RCDM_LIB=<the parent's librcdm_hip.so> python tests/test_igemm_plan.py --record`.

The expectations assume 256 compute units: what the library falls back to without a device, and the MI355X's count."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "igemm_plan.npz")

GEMM_M = (10, 160, 640, 970, 2560, 5120, 10240, 20480, 40960, 81920, 163840)
GEMM_N = (8, 64, 320, 640, 960, 1280, 1920, 2048, 2560, 5120, 6144, 10240)
GEMM_K = (64, 320, 640, 960, 1280, 1920, 2048, 2560, 3200, 6400)
GEMM_SPLIT = (0, 1, 4)
FLAGS = ((0, 0), (1, 0), (0, 1), (1, 1))   # (producer, consumer)
EPI_GEGLU = 8
CONV_NIMG = (5, 10, 20, 40)
CONV_SIDE = (8, 16, 32, 64, 128)
CONV_CIN = (64, 320, 640, 960, 1280, 1920, 2560)
CONV_COUT = (8, 320, 640, 1280)
CONV_SPLIT = (0, 4)
# (stride, upsample, c_in2): the pairs the library accepts — a strided conv does not upsample, a second input comes with neither
CONV_FORMS = ((1, 0, 0), (1, 0, 320), (1, 1, 0), (1, 2, 0), (2, 0, 0))

# a grid row is a descriptor (*_DESC_COLS); the arrays hold one row of answers (*_COLS) per descriptor, in grid order
GEMM_DESC_COLS = ("M", "N", "K", "split_k", "epilogue", "producer", "consumer")
GEMM_COLS = ("variant", "BM", "BN", "tilesM", "tilesN", "splits", "blocks_per_cu", "nk", "workspace_bytes",
             "stat_parts", "lnx_stat_parts", "parts_ok_n64", "parts_ok_n128", "parts_ok_3", "gnstat_ok")
CONV_DESC_COLS = ("n_img", "side", "c_in", "c_out", "stride", "upsample", "split_k", "c_in2")
CONV_COLS = ("rc", "variant", "BM", "BN", "tilesM", "tilesN", "splits", "blocks_per_cu", "nk",
             "workspace_bytes", "up2_supported", "gnstat_ok")


def gemm_grid():
    for M, N, K, sk in itertools.product(GEMM_M, GEMM_N, GEMM_K, GEMM_SPLIT):
        for epi in (0, EPI_GEGLU) if N % 32 == 0 else (0,):
            for p, c in FLAGS:
                yield M, N, K, sk, epi, p, c


def conv_grid():
    for n, side, ci, co, sk in itertools.product(CONV_NIMG, CONV_SIDE, CONV_CIN, CONV_COUT, CONV_SPLIT):
        for stride, up, ci2 in CONV_FORMS:
            yield n, side, ci, co, stride, up, sk, ci2


def gemm_row(lib, hip, row):
    M, N, K, sk, epi, p, c = row
    d = hip.GemmDesc(M, N, K, K, N // 2 if epi & EPI_GEGLU else N, 0, epi, 1, 0, 1.0, sk, 0)
    out = (C.c_int32 * 8)()
    rc = lib.rcdm_gemm_plan_query(C.byref(d), p, c, out)
    assert rc == 0, (row, rc)
    ws = lib.rcdm_gemm_lnx_workspace_bytes(C.byref(d), p, c) if (p or c) else lib.rcdm_gemm_workspace_bytes(C.byref(d))
    n64, n128 = (N + 63) // 64, (N + 127) // 128
    gn = hip.GroupNormDesc(10, M // 10, N, 32, N, N, 1e-5, 1)   # the norm that would read the output next: 10 samples
    return tuple(out) + (
        ws, lib.rcdm_gemm_stat_parts(C.byref(d)), lib.rcdm_gemm_lnx_stat_parts(C.byref(d), c),
        lib.rcdm_gemm_lnx_parts_ok(C.byref(d), n64, c), lib.rcdm_gemm_lnx_parts_ok(C.byref(d), n128, c),
        lib.rcdm_gemm_lnx_parts_ok(C.byref(d), 3, c), lib.rcdm_gemm_gnstat_ok(C.byref(d), C.byref(gn)))


def conv_row(lib, hip, row):
    n, side, ci, co, stride, up, sk, ci2 = row
    d = hip.ConvDesc(n, side, side, ci, co, stride, up, ci, co, 0, 1, 1, 0, 1.0, sk, 0, 0, ci2, ci2)
    out = (C.c_int32 * 8)()
    rc = lib.rcdm_conv3x3_plan_query(C.byref(d), out)
    plan = tuple(out) if rc == 0 else (0,) * 8
    so = ((side << (1 if up else 0)) - 1) // stride + 1
    gn = hip.GroupNormDesc(n, so * so, co, 32, co, co, 1e-5, 1)
    return (rc,) + plan + (lib.rcdm_conv3x3_workspace_bytes(C.byref(d)), lib.rcdm_conv3x3_up2_supported(C.byref(d)),
                          lib.rcdm_conv3x3_gnstat_ok(C.byref(d), C.byref(gn)))


def sweep(lib, hip):
    return {"gemm": np.array([gemm_row(lib, hip, r) for r in gemm_grid()], dtype=np.int64),
            "conv": np.array([conv_row(lib, hip, r) for r in conv_grid()], dtype=np.int64)}


# The rows repeated under every switch state: every SUBSET_GEMM_STEP-th / SUBSET_CONV_STEP-th row of the grids (the steps are
# coprime to the grids' inner axes, so every flag pair, epilogue, split and conv form occurs) plus the shapes the two-rule
# string below names.  test_fixture_is_not_hollow checks that they reach every variant.
SUBSET_GEMM_STEP, SUBSET_CONV_STEP = 211, 113
TWO_RULES = "1,2560,1280,1280,5,2;9,40960,320,320,6,0"


def subset_rows():
    g = [r for i, r in enumerate(gemm_grid()) if i % SUBSET_GEMM_STEP == 0]
    g += [(2560, 1280, 1280, 0, 0, p, c) for p, c in FLAGS]
    c = [r for i, r in enumerate(conv_grid()) if i % SUBSET_CONV_STEP == 0]
    c += [(10, 64, 320, 320, 1, 0, 0, 0)]
    return g, c


def subset_sweep(lib, hip):
    g, c = subset_rows()
    return (np.array([gemm_row(lib, hip, r) for r in g], dtype=np.int64),
            np.array([conv_row(lib, hip, r) for r in c], dtype=np.int64))


def setter_states(lib, hip):
    """The subset under each state the setters reach, defaults restored afterwards."""
    out = {}

    def run(name):
        out[name + "_gemm"], out[name + "_conv"] = subset_sweep(lib, hip)

    try:
        for v in range(11):
            hip.set_igemm_variant(v)
            run(f"variant{v}")
        hip.set_igemm_variant(-1)
        hip.set_shape_rules("off")
        run("rules_off")
        hip.set_shape_rules(TWO_RULES)
        run("rules_two")
        hip.set_shape_rules(None)
        hip.set_igemm_pingpong(0)
        run("pp_off")
    finally:
        hip.set_igemm_variant(-1)
        hip.set_shape_rules(None)
        hip.set_igemm_pingpong(1)
    return out


ENV_STATES = {"env_rules": {"RCDM_SHAPE_RULES": TWO_RULES}, "env_pp0": {"RCDM_PP": "0"}, "env_i16_0": {"RCDM_I16": "0"},
              "env_dma64": {"RCDM_IGEMM": "dma64"}}


def env_states():
    """The subset in one fresh process per environment switch (the library reads each switch once per process)."""
    procs = {}
    for name, extra in ENV_STATES.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("RCDM_") or k == "RCDM_LIB"}
        env.update(extra)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--subset"]
        procs[name] = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE)
    out = {}
    for name, p in procs.items():
        text, _ = p.communicate()
        assert p.returncode == 0, f"child process for {name} failed"
        res = json.loads(text.decode().strip().splitlines()[-1])
        out[name + "_gemm"] = np.array(res["gemm"], dtype=np.int64)
        out[name + "_conv"] = np.array(res["conv"], dtype=np.int64)
    return out


def load_lib():
    from rcdms_amd import hip
    return hip.load(), hip


def everything():
    lib, hip = load_lib()
    res = sweep(lib, hip)            # first: the defaults, before any setter has been called
    res["default_gemm"], res["default_conv"] = subset_sweep(lib, hip)
    res.update(setter_states(lib, hip))
    after = sweep(lib, hip)          # the setters' "back to the default" really is the default
    for k in after:
        assert np.array_equal(res[k], after[k]), f"{k}: the defaults did not come back after the setters"
    res.update(env_states())
    return res


_cache = {}


def results():
    if "got" not in _cache:
        set_ = [k for k in ("RCDM_SHAPE_RULES", "RCDM_PP", "RCDM_I16", "RCDM_IGEMM") if k in os.environ]
        assert not set_, f"the recorded plans are the defaults': unset {set_}"
        import __graft_entry__
        __graft_entry__.build()
        _cache["got"] = everything()
        _cache["want"] = dict(np.load(GOLDEN))
    return _cache["got"], _cache["want"]


def first_differences(name, got, want, limit=5):
    gemm = name.endswith("gemm")
    cols, desc_cols = (GEMM_COLS, GEMM_DESC_COLS) if gemm else (CONV_COLS, CONV_DESC_COLS)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, expected {want.shape}"
    descs = list(gemm_grid() if gemm else conv_grid()) if name in ("gemm", "conv") else subset_rows()[0 if gemm else 1]
    lines = []
    for i in np.flatnonzero((got != want).any(axis=1))[:limit]:
        bad = [f"{cols[j]} {want[i, j]} -> {got[i, j]}" for j in np.flatnonzero(got[i] != want[i])]
        lines.append(f"{name}[{i}] " + ", ".join(f"{c}={v}" for c, v in zip(desc_cols, descs[i])) + ": " + "; ".join(bad))
    return "\n".join(lines)


def test_plans_equal_the_recorded_ones():
    got, want = results()
    assert sorted(got) == sorted(want)
    report = [first_differences(k, got[k], want[k]) for k in sorted(want) if not np.array_equal(got[k], want[k])]
    print("\n".join(report))
    assert not report, "the planner's answers changed:\n" + "\n".join(report)


def test_fixture_is_not_hollow():
    want = dict(np.load(GOLDEN))
    g, c = want["gemm"], want["conv"]
    assert len(g) == 30360 and len(c) == 5600
    gcol, ccol = GEMM_COLS.index, CONV_COLS.index
    ok = c[:, ccol("rc")] == 0
    variants = set(g[:, gcol("variant")]) | set(c[ok, ccol("variant")])
    assert variants == set(range(1, 11)), variants
    assert set(range(1, 11)) <= set(want["default_gemm"][:, gcol("variant")]) | set(want["default_conv"][:, ccol("variant")])
    assert (g[:, gcol("splits")] > 1).any() and (c[:, ccol("splits")] > 1).any()
    assert (g[:, gcol("workspace_bytes")] > 0).any() and (c[:, ccol("workspace_bytes")] > 0).any()
    assert set(c[:, ccol("up2_supported")]) == {0, 1}
    assert set(c[:, ccol("gnstat_ok")]) == {0, 1} and set(g[:, gcol("gnstat_ok")]) == {0, 1}
    for name in ("parts_ok_n64", "parts_ok_n128", "parts_ok_3"):
        assert set(g[:, gcol(name)]) == {0, 1}, name
    assert (c[:, ccol("rc")] != 0).any()
    # every switch state changes something, so a setter or a latch that stopped working cannot hide
    for state in [f"variant{v}" for v in range(1, 11)] + ["rules_off", "rules_two", "pp_off"] + list(ENV_STATES):
        assert any(not np.array_equal(want[f"{state}_{kind}"], want[f"default_{kind}"]) for kind in ("gemm", "conv")), state
    assert np.array_equal(want["env_rules_gemm"], want["rules_two_gemm"])
    assert np.array_equal(want["env_pp0_conv"], want["pp_off_conv"])


if __name__ == "__main__":
    if "--subset" in sys.argv:
        lib_, hip_ = load_lib()
        g_, c_ = subset_sweep(lib_, hip_)
        print(json.dumps({"gemm": g_.tolist(), "conv": c_.tolist()}))
    elif "--record" in sys.argv:
        assert os.environ.get("RCDM_LIB"), "record from the PARENT's library: set RCDM_LIB to it"
        np.savez_compressed(GOLDEN, **everything())
        print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
