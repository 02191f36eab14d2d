"""GPU: exact-answer tests of the implicit-GEMM family — rcdm_gemm, rcdm_conv3x3 (every form), rcdm_conv3x3_add1x1, the
*_gnstat entries, rcdm_conv_taps_gather and rcdm_conv3x3_wino — on every tile variant, through split-K in both slab formats.

The operands are the small integers of tests/gemm_exact.py, the reference is its numpy code, and the outputs are compared
with torch.equal: a dropped, doubled or misplaced product changes an integer.  Before a launch the conditions that make the
answer exact (expected outputs are f16 values; every split-K partial — taken from the planner's own split count — is an
integer <= 2048, every Winograd partial a multiple of 1/4 below 512) are asserted on the reference alone.

Last, the f16 slabs at the edge of their range: partials that cancel (the error bound comes from the f16 spacing at the
reference's own partials) and partials or transform-domain values beyond 65504 (exactly right or non-finite, never finite
and wrong)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gemm_exact as X
from tests.guard import check_all
from tests.test_hip_kernels import DEV, gin, gout, gvec, gw, ws

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = list(range(1, 11))
SLABS = [0, 1]


def t16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).half()


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


@contextlib.contextmanager
def switches(hip, variant=-1, slab16=-1, wino16=-1):
    hip.set_igemm_variant(variant)
    hip.set_splitk_slab_f16(slab16)
    hip.set_wino_slab_f16(wino16)
    try:
        yield
    finally:
        hip.set_igemm_variant(-1)
        hip.set_splitk_slab_f16(-1)
        hip.set_wino_slab_f16(-1)


def exact(out, ref, what=""):
    """torch.equal against the integer reference; on a mismatch the integer difference names the missing product."""
    want = t16(ref)
    got = out.detach().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if torch.equal(got, want):
        return
    diff = got.double() - want.double()
    bad = (got != want)
    r, c = (int(v) for v in bad.nonzero()[0])
    rows = bad.any(dim=1).nonzero().reshape(-1)
    raise AssertionError(f"{what}{int(bad.sum())} of {bad.numel()} elements differ, rows {int(rows[0])}..{int(rows[-1])}; first at row {r}, "
                         f"column {c}: got {got[r, c].item()}, expected {want[r, c].item()}; differences seen: "
                         f"{sorted(set(diff[bad].tolist()))[:8]}")


_checked = set()


def partials_ok(key, problem, splits):
    """The split-K conditions of this (case, split count), asserted once."""
    if splits > 1 and (key, splits) not in _checked:
        X.check_partials(problem.partials(splits))
        _checked.add((key, splits))


# ---- rcdm_gemm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("M,N,K,epi,split,scale", X.GEMM_CASES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm(hiplib, M, N, K, epi, split, scale, variant, slab16):
    from rcdms_amd import hip
    _gemm(hip, (M, N, K, epi, split, scale), variant, slab16)


def _gemm(hip, case, variant, slab16):
    M, N, K, epi, split, scale = case
    c = X.gemm_case(M, N, K, epi, scale)
    lda, ldc, ldr, ldt = K + 8, N + 16, N + 8, N + 8
    d = hip.GemmDesc(M, N, K, lda, ldc, ldr, epi, c["rps"], ldt, scale, split)
    Ad, Wd, Rd = gin(t16(c["A"]), lda), gw(t16(c["W"])), gin(t16(c["res"]), ldr)
    bd, rvd = gvec(t32(c["bias"])), gin(t32(c["rowvec"]), ldt, guard_rows=8)
    out = gout(M, N, ldc)
    with switches(hip, variant, slab16):
        splits = hip.gemm_plan_query(d)["splits"]
        assert split in (0, 1) or splits > 1, "the case is meant to run through slabs"
        partials_ok(("gemm", M, N, K), c["problem"], splits)
        w = ws(hip.gemm_workspace_bytes(d))
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), rvd.data_ptr(), Rd.data_ptr(), out.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
    exact(out[:, :N], c["ref"], f"{splits} splits: ")
    check_all(out, Ad, Wd, Rd, bd, rvd)


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("variant", [1, 2, 5, 6, 8, 9])
def test_gemm_dup_rows(hiplib, variant, split, slab16):
    """dup_rows: every output row is stored a second time dup_rows further down, from the fused epilogue and from the reduce pass."""
    from rcdms_amd import hip
    M, N, K = 300, 320, 256
    c = X.gemm_case(M, N, K, 1, 1.0)
    Ad, Wd, bd = gin(t16(c["A"])), gw(t16(c["W"])), gvec(t32(c["bias"]))
    out = gout(2 * M + 3, N)
    d = hip.GemmDesc(M, N, K, K, N, 0, 1, 1, 0, 1.0, split, M + 3)
    with switches(hip, variant, slab16):
        splits = hip.gemm_plan_query(d)["splits"]
        assert (splits > 1) == (split > 1)
        partials_ok(("gemm", M, N, K), c["problem"], splits)
        w = ws(hip.gemm_workspace_bytes(d))
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
    exact(out[:M], c["ref"])
    exact(out[M + 3:], c["ref"], "second copy: ")
    assert torch.isnan(out[M:M + 3].float()).all()
    check_all(out, Ad, Wd, bd)


# ---- rcdm_conv3x3 / rcdm_conv3x3_add1x1 -----------------------------------------------------------------------------------
def _conv(hip, case, variant, slab16, gn=False):
    n_img, H, W, cin, cout, stride, up, pao, split, cin2 = case
    epi, scale = 7, (0.5 if cin2 else 1.0)
    c = X.conv_case(n_img, H, W, cin, cout, stride, up, pao, cin2, epi, scale)
    p = c["problem"]
    M = n_img * p.Ho * p.Wo
    lda, lda2 = cin + 8, (cin2 + 16 if cin2 else 0)
    ldc = cout + 8 if gn else cout
    xd, rd = gin(t16(c["x"].reshape(-1, cin)), lda), gin(t16(c["res"]))
    w32, bd, td = gvec(t32(c["w"])), gvec(t32(c["bias"])), gvec(t32(c["rowvec"]))
    wp = gout(cout, 9 * cin)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    ins = [xd, rd, w32, bd, td]
    wk = wp
    if cin2:
        x2d = gin(t16(c["x2"].reshape(-1, cin2)), lda2)
        wk = gw(torch.cat([wp[:, :9 * cin], t16(c["w2"]).to(DEV)], dim=1))
        ins += [x2d, wk]
    out = gout(M, cout, ldc)
    d = hip.ConvDesc(n_img, H, W, cin, cout, stride, up, lda, ldc, cout, epi, c["rps"], cout, scale, split, pao, 0, cin2, lda2)
    with switches(hip, variant, slab16):
        plan = hip.conv3x3_plan_query(d)
        assert plan["k_steps"] == p.nk
        assert split == 1 or plan["splits"] > 1, "the case is meant to run through slabs"
        partials_ok(("conv",) + case, p, plan["splits"])
        wsb = ws(hip.conv3x3_workspace_bytes(d))
        args = (bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(), wsb.data_ptr(), wsb.numel())
        if gn:
            gnd = hip.GroupNormDesc(n_img, p.Ho * p.Wo, cout, 32, ldc, cout, 1e-5, 0)
            assert hip.conv3x3_gnstat_ok(d, gnd)
            gk = ws(hip.groupnorm_workspace_bytes(gnd))
            hip.conv3x3_gnstat(d, gnd, xd.data_ptr(), wk.data_ptr(), *args, gk.data_ptr(), gk.numel())
        elif cin2:
            hip.conv3x3_add1x1(d, xd.data_ptr(), x2d.data_ptr(), wk.data_ptr(), *args)
        else:
            hip.conv3x3(d, xd.data_ptr(), wk.data_ptr(), *args)
        torch.cuda.synchronize()
    exact(out[:, :cout], c["ref"], f"{plan['splits']} splits: ")
    check_all(out, wp, *ins)


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("case", X.CONV_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("variant", VARIANTS)
def test_conv3x3(hiplib, case, variant, slab16):
    from rcdms_amd import hip
    _conv(hip, case, variant, slab16)


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("case", X.ADD1X1_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("variant", [1, 3, 5, 6, 7, 8, 9])
def test_conv3x3_add1x1(hiplib, case, variant, slab16):
    from rcdms_amd import hip
    _conv(hip, case, variant, slab16)


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("n_img,H,W,cin,cout,variant,split", X.UP2_CASES)
def test_conv3x3_up2(hiplib, n_img, H, W, cin, cout, variant, split, slab16):
    """upsample = 2: the packed phase weights (sums of at most four +-1 taps) and the four phase convolutions."""
    from rcdms_amd import hip
    c = X.up2_case(n_img, H, W, cin, cout)
    lda = cin + 8
    xd = gin(t16(c["x"].reshape(-1, cin)), lda)
    w32, bd = gvec(t32(c["w"])), gvec(t32(c["bias"]))
    wp2 = gout(4 * cout, 4 * cin)
    hip.pack_conv3x3_up2(w32.data_ptr(), cout, cin, wp2.data_ptr())
    torch.cuda.synchronize()
    exact(wp2, X.up2_pack(c["w"]).reshape(4 * cout, 4 * cin), "packed weights: ")
    out = gout(4 * n_img * H * W, cout)
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 2, lda, cout, 0, X.EPI_BIAS, 1, 0, 1.0, split)
    with switches(hip, variant, slab16):
        assert hip.conv3x3_up2_supported(d)
        splits = hip.conv3x3_plan_query(d)["splits"]
        assert (splits > 1) == (split > 1)
        for ph, p in enumerate(c["problems"]):
            partials_ok(("up2", n_img, H, W, cin, cout, ph), p, splits)
        w2 = ws(hip.conv3x3_workspace_bytes(d))
        hip.conv3x3(d, xd.data_ptr(), wp2.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w2.data_ptr(), w2.numel())
        torch.cuda.synchronize()
    exact(out, c["ref"], f"{splits} splits: ")
    check_all(out, wp2, xd, w32, bd)


@pytest.mark.parametrize("up", [0, 1])
def test_conv_taps_gather(hiplib, up):
    """One GEMM over nine stacked tap planes + rcdm_conv_taps_gather: the planes (|P| <= 2 c_in) and the gathered sums."""
    from rcdms_amd import hip
    n_img, H, W, cin, cout = 3, 4, 6, 64, 64
    c = X.conv_case(n_img, H, W, cin, cout, 1, up, 0, 0, 1, 1.0)
    M, lda, ldp, ldc = n_img * H * W, cin + 8, 9 * cout + 8, cout + 8
    W9 = c["w"].transpose(2, 3, 0, 1).reshape(9 * cout, cin)
    planes = c["x"].reshape(M, cin) @ W9.T
    X.check_output(planes)
    xd, W9d, bd = gin(t16(c["x"].reshape(M, cin)), lda), gw(t16(W9)), gvec(t32(c["bias"]))
    P = gout(M, 9 * cout, ldp)
    d = hip.GemmDesc(M, 9 * cout, cin, lda, ldp, 0, 0, 1, 0, 1.0, 0, 0)
    wsb = ws(hip.gemm_workspace_bytes(d))
    hip.gemm(d, xd.data_ptr(), W9d.data_ptr(), 0, 0, 0, P.data_ptr(), wsb.data_ptr(), wsb.numel())
    out = gout(M << (2 * up), cout, ldc)
    hip.conv_taps_gather(P.data_ptr(), ldp, n_img, H, W, cout, up, bd.data_ptr(), out.data_ptr(), ldc)
    torch.cuda.synchronize()
    exact(P[:, :9 * cout], planes, "tap planes: ")
    exact(out[:, :cout], c["ref"])
    check_all(out, P, xd, W9d, bd)


# ---- RCDM_PP_ROTATE=1: the ping-pong kernel's per-block k rotation in front of the shared k-step decode ---------------------
# Split GEMM, split conv and second-input cases of the lists above, and one GEMM and one conv with more than eight row tiles:
# the rotation of a block is its position in its XCD's run of tiles (blockIdx.x >> 3), zero for every block of the small cases.
ROTATED_GEMMS = [(161, 168, 704, 1, 3, 1.0), (2305, 168, 704, 1, 3, 1.0)]
ROTATED_CONVS = [(2, 8, 8, 320, 320, 1, 0, 0, 4, 0), (2, 8, 8, 320, 320, 1, 0, 0, 4, 640), (40, 8, 8, 128, 64, 1, 0, 0, 1, 0)]


def rotated_child():
    """Runs in a process of its own (the switch is latched at the first ping-pong launch)."""
    assert os.environ.get("RCDM_PP_ROTATE") == "1"
    from rcdms_amd import hip
    hip.load()
    for variant in (6, 8):
        for slab16 in SLABS:
            for case in ROTATED_GEMMS:
                _gemm(hip, case, variant, slab16)
            for case in ROTATED_CONVS:
                _conv(hip, case, variant, slab16)
    print("rotated: ok")


def test_pingpong_rotated_k_order(hiplib):
    """Bit for bit in any k order: integer sums below 2^24 are exact, and the rotation stays inside a split, so every slab
    holds the same set of k-steps."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("RCDM_") or k == "RCDM_LIB"}
    env["RCDM_PP_ROTATE"] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_hip_gemm_exact", "--rotated"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and text.strip().endswith("rotated: ok"), text[-4000:]


# ---- the *_gnstat entries: the output rows (their statistics keep their bit-identity test in tests/test_hip_kernels.py) -------
@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("variant", [1, 9])
def test_gemm_gnstat_rows(hiplib, variant, slab16):
    from rcdms_amd import hip
    M, N, K, epi = 320, 320, 320, 7
    c = X.gemm_case(M, N, K, epi, 1.0)
    ldc = N + 8
    d = hip.GemmDesc(M, N, K, K, ldc, N, epi, c["rps"], N, 1.0, 2)
    gnd = hip.GroupNormDesc(2, M // 2, N, 32, ldc, N, 1e-5, 0)
    Ad, Wd, Rd = gin(t16(c["A"])), gw(t16(c["W"])), gin(t16(c["res"]))
    bd, rvd = gvec(t32(c["bias"])), gvec(t32(c["rowvec"]))
    out = gout(M, N, ldc)
    with switches(hip, variant, slab16):
        splits = hip.gemm_plan_query(d)["splits"]
        assert splits > 1 and hip.gemm_gnstat_ok(d, gnd)
        partials_ok(("gemm", M, N, K), c["problem"], splits)
        w, gk = ws(hip.gemm_workspace_bytes(d)), ws(hip.groupnorm_workspace_bytes(gnd))
        hip.gemm_gnstat(d, gnd, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), rvd.data_ptr(), Rd.data_ptr(), out.data_ptr(),
                        w.data_ptr(), w.numel(), gk.data_ptr(), gk.numel())
        torch.cuda.synchronize()
    exact(out[:, :N], c["ref"])
    check_all(out, Ad, Wd, Rd, bd, rvd)


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("variant", [1, 9])
def test_conv3x3_gnstat_rows(hiplib, variant, slab16):
    from rcdms_amd import hip
    _conv(hip, (2, 8, 8, 128, 320, 1, 0, 0, 3, 0), variant, slab16, gn=True)


# ---- rcdm_conv3x3_wino ----------------------------------------------------------------------------------------------------
def _wino_launch(hip, c, n_img, H, W, cin, cin2, cout, epi, split, scale, gn, wino16, expect_splits=True):
    lda, lda2 = cin + 8, (cin2 + 16 if cin2 else 0)
    xd, rd = gin(t16(c["x"].reshape(-1, cin)), lda), gin(t16(c["res"])) if epi & 4 else None
    x2d = gin(t16(c["x2"].reshape(-1, cin2)), lda2) if cin2 else None
    w2d = gw(t16(c["w2"])) if cin2 else None
    w32 = gvec(t32(c["w"]))
    U = gout(16 * cout, cin)
    hip.pack_conv3x3_wino(w32.data_ptr(), cout, cin, U.data_ptr())
    bd = gvec(t32(c["bias"])) if epi & 1 else None
    td = gvec(t32(c["rowvec"])) if epi & 2 else None
    out = gout(n_img * H * W, cout)
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, lda, cout, cout if epi & 4 else 0, epi, H * W, cout, scale, split, 0, 0, cin2, lda2)
    assert hip.conv3x3_wino_supported(d)
    gnd = stat = gd = bed = None
    if gn:   # the norm as an exact affine map: (mean, rstd) = (0, 1), integer gamma and beta, no activation
        gnd = hip.GroupNormDesc(n_img, H * W, cin, 32, lda, lda, 1e-5, 0)
        stat = gvec(torch.tensor([0.0, 1.0]).repeat(n_img * 32))
        gd, bed = gvec(torch.full((cin,), X.GN_GAMMA)), gvec(torch.full((cin,), X.GN_BETA))
    with switches(hip, wino16=wino16):
        splits = hip.conv3x3_wino_plan_query(d)[5]
        assert split <= 1 or splits > 1, "the case is meant to run through more than one slab"
        if expect_splits and ("wino", id(c), splits) not in _checked:
            X.wino_check(c, splits)
            _checked.add(("wino", id(c), splits))
        wsb = ws(hip.conv3x3_wino_workspace_bytes(d))
        hip.conv3x3_wino(d, xd.data_ptr(), U.data_ptr(), bd.data_ptr() if epi & 1 else 0, td.data_ptr() if epi & 2 else 0,
                         rd.data_ptr() if epi & 4 else 0, out.data_ptr(), wsb.data_ptr(), wsb.numel(),
                         x2=x2d.data_ptr() if cin2 else 0, W2=w2d.data_ptr() if cin2 else 0, gn=gnd,
                         gn_stat=stat.data_ptr() if gn else 0, gn_gamma=gd.data_ptr() if gn else 0, gn_beta=bed.data_ptr() if gn else 0)
        torch.cuda.synchronize()
    check_all(out, U, *[t for t in (xd, rd, x2d, w2d, w32, bd, td, stat, gd, bed) if t is not None])
    return out, splits


@pytest.mark.parametrize("wino16", SLABS)
@pytest.mark.parametrize("n_img,H,W,cin,cin2,cout,epi,split,scale,gn", X.WINO_CASES)
def test_conv3x3_wino(hiplib, n_img, H, W, cin, cin2, cout, epi, split, scale, gn, wino16):
    from rcdms_amd import hip
    c = X.wino_case(n_img, H, W, cin, cin2, cout, epi, scale, gn)
    out, splits = _wino_launch(hip, c, n_img, H, W, cin, cin2, cout, epi, split, scale, gn, wino16)
    exact(out, c["ref"], f"{splits} splits: ")


# ---- slab range -----------------------------------------------------------------------------------------------------------
def _cancel_gemm(hip, P, variant, slab16):
    c = X.cancel_gemm_case(P)
    M, N, K = X.CANCEL_M, X.CANCEL_N, X.CANCEL_K
    Ad, Wd = gin(t16(c["A"]), K + 8), gw(t16(c["W"]))
    out = gout(M, N, N + 8)
    d = hip.GemmDesc(M, N, K, K + 8, N + 8, 0, 0, 1, 0, 1.0, 2)
    with switches(hip, variant, slab16):
        assert hip.gemm_plan_query(d)["splits"] == 2
        w = ws(hip.gemm_workspace_bytes(d))
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), 0, 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
    check_all(out, Ad, Wd)
    return c, out[:, :N].double().cpu().numpy()


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("P", [2048, 40000])
@pytest.mark.parametrize("variant", [1, 9])
def test_gemm_partials_cancel(hiplib, variant, P, slab16):
    """Split-K partials (P, -P + r): fp32 slabs give r exactly; f16 slabs give a finite value within the sum of half the f16
    spacing at each partial plus half the spacing at the result."""
    from rcdms_amd import hip
    c, got = _cancel_gemm(hip, P, variant, slab16)
    if not slab16:
        assert (got == c["r"]).all()
        return
    assert np.isfinite(got).all()
    err, bound = np.abs(got - c["r"]), X.slab_error_bound(c["problem"].partials(2), c["r"])
    print(f"P = {P}: largest error {err.max()}, bound {bound.max()}")
    assert (err <= bound).all(), f"largest error {err.max()} against the bound {bound.max()}"


@pytest.mark.parametrize("slab16", SLABS)
@pytest.mark.parametrize("variant", [1, 9])
def test_gemm_partials_out_of_range(hiplib, variant, slab16):
    """Partials of +-81920 whose sum r fits: fp32 slabs give r; with f16 slabs an element is r or non-finite, never finite and wrong."""
    from rcdms_amd import hip
    c, got = _cancel_gemm(hip, 81920, variant, slab16)
    if not slab16:
        assert (got == c["r"]).all()
        return
    wrong = np.isfinite(got) & (got != c["r"])
    print(f"{int((~np.isfinite(got)).sum())} of {got.size} elements non-finite")
    assert not wrong.any(), f"{int(wrong.sum())} elements finite and wrong, e.g. {got[wrong][:4]} for {c['r'][wrong][:4]}"


@pytest.mark.parametrize("wino16", SLABS)
@pytest.mark.parametrize("A", X.WINO_CANCEL_LEVELS)
def test_wino_partials_cancel(hiplib, A, wino16):
    from rcdms_amd import hip
    c = X.cancel_wino_case(A)
    out, splits = _wino_launch(hip, c, 2, 8, 8, 128, 0, 64, 0, 2, 1.0, False, wino16, expect_splits=False)
    assert splits == 2
    got = out.double().cpu().numpy()
    if not wino16:
        assert (got == c["acc"]).all()
        return
    _, slabs, V, U = X.wino_model(c["x"], c["w"], 2, None, None, np.float16, None)
    assert (V == np.rint(V)).all() and np.abs(V).max() <= 2048 and (4 * U == np.rint(4 * U)).all()    # the operand roundings are exact
    err, bound = np.abs(got - c["acc"]), X.wino_slab_error_bound(slabs, c["acc"])
    print(f"pixel level {A}: largest slab value {np.abs(slabs).max()}, largest error {err.max()}, bound {bound.max()}")
    assert np.isfinite(got).all() and (err <= bound).all(), f"largest error {err.max()} against the bound {bound.max()}"


@pytest.mark.parametrize("wino16", SLABS)
def test_wino_input_transform_out_of_range(hiplib, wino16):
    """A checkerboard of +-20000 pixels: B^T d B = 80000 leaves f16 although every pixel and every output fits.  The nine-tap
    form gives the bias exactly; the Winograd form gives that or a non-finite value, and is exact on the image that fits."""
    from rcdms_amd import hip
    c = X.overflow_wino_case()
    c = dict(c, bias=X.ints(X.gen(7), 8, 64))
    want = c["acc"] + c["bias"][None, :]
    out, _ = _wino_launch(hip, c, 2, 8, 8, 64, 0, 64, 1, 1, 1.0, False, wino16, expect_splits=False)
    got = out.double().cpu().numpy()
    big = c["big_rows"]
    assert (got[~big] == want[~big]).all()
    wrong = np.isfinite(got[big]) & (got[big] != want[big])
    print(f"{int((~np.isfinite(got[big])).sum())} of {got[big].size} elements of the out-of-range image non-finite")
    assert not wrong.any(), f"{int(wrong.sum())} elements finite and wrong"
    # the nine-tap form on the same operands
    xd, w32, bd = gin(t16(c["x"].reshape(-1, 64)), 72), gvec(t32(c["w"])), gvec(t32(c["bias"]))
    wp = gout(64, 9 * 64)
    hip.pack_conv3x3(w32.data_ptr(), 64, 64, 64, wp.data_ptr())
    out9 = gout(128, 64)
    d = hip.ConvDesc(2, 8, 8, 64, 64, 1, 0, 72, 64, 0, 1, 1, 0, 1.0, 1)
    hip.conv3x3(d, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), 0, 0, out9.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    exact(out9, want, "nine-tap form: ")
    check_all(out9, wp, xd, w32, bd)


if __name__ == "__main__":
    if "--rotated" in sys.argv:
        rotated_child()
