"""GPU: every place the library forms GroupNorm statistics, on groups far from zero (tests/gn_cond.py: the cases, the float64
reference and the budgets, which come from the f16 output and not from any kernel):

  a  rcdm_groupnorm_stats (the single-launch kernel and statistics + finalize) against float64
  b  rcdm_groupnorm_silu on the same shapes, the apply kernel that finalises by itself (bit-identical), rcdm_groupnorm_apply alone
  c  the producers' statistics: rcdm_conv3x3_gnstat / rcdm_gemm_gnstat / rcdm_conv3x3_add1x1_gnstat + the *_prestat norms, and the
     Winograd output transform's per-tile partials + rcdm_groupnorm_finalize, against float64 statistics of the rows the
     producer STORED; the offsets are placed by the epilogue (bias, row vector or residual), the weights carry the sigma

32 groups, ldx = C + 8, eps 1e-5 (the cross-frame norms) and 1e-6 (the per-frame ones).  Which kernel runs is asked of the
library's own predicates and asserted, so a planner change cannot move a case to another kernel unnoticed.  The split-K
producers at 16x16 take partials only for a cross-frame norm (per frame a 16x16 image is a single-launch norm, which takes
none), so those run at eps 1e-5 and a 32x32 conv in front of a per-frame norm runs at eps 1e-6; the Winograd partials serve
both."""
import functools

import numpy as np
import pytest
import torch

from tests import gn_cond as G
from tests.guard import check_all, check_written
from tests.test_hip_kernels import gin, gout, gvec, gw, ws

pytestmark = pytest.mark.gpu

GR = G.GROUPS
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@functools.lru_cache(maxsize=None)
def _input(shape, case):
    return G.make_input(*shape, GR, case)


@functools.lru_cache(maxsize=None)
def _ref(shape, case, eps):
    return G.reference(_input(shape, case), *shape, GR, eps)


def _splits(hip, d):
    """split count of the three-launch form, from the workspace size ([samples][groups][splits][3] + [samples][groups][2] floats)"""
    return (hip.groupnorm_workspace_bytes(d) // 4 - d.samples * d.groups * 2) // (d.samples * d.groups * 3)


def _assert_form(hip, d, shape):
    """The form the shape table promises is the one the library takes."""
    three = bool(hip.groupnorm_prestat_ok(d))
    assert three == (shape not in G.SINGLE_LAUNCH), f"{shape}: the library takes the {'three' if three else 'single'}-launch form"
    if three:
        splits = _splits(hip, d)
        assert splits > 1, "one split: rows_per_split == rows"
        if shape == (1, 1283, 320):
            rps = -(-shape[1] // splits)
            assert shape[1] % rps, "the last split is not short"


def _stats(got, samples):
    got = got.cpu().numpy().reshape(samples, GR, 2)
    return got[..., 0], got[..., 1]


# ---- a. statistics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=_ids)
def test_groupnorm_stats_far_from_zero(hiplib, shape, case):
    from rcdms_amd import hip
    samples, rows, C = shape
    x = _input(shape, case)
    kinds = G.group_kinds(samples, GR, case)
    xd = gin(torch.from_numpy(x).half(), C + 8)
    for eps in G.EPS:
        d = hip.GroupNormDesc(samples, rows, C, GR, C + 8, C, eps, 0)
        _assert_form(hip, d, shape)
        stat = gout(1, samples * GR * 2, dtype=torch.float32, guard_rows=1)
        w = ws(hip.groupnorm_workspace_bytes(d))
        hip.groupnorm_stats(d, xd.data_ptr(), stat.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
        check_all(stat, xd)
        check_written(stat)
        G.assert_stats(*_stats(stat, samples), x, samples, rows, C, GR, eps, kinds, f"stats {shape} {case} eps {eps}")


# ---- b. output ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=_ids)
def test_groupnorm_silu_far_from_zero(hiplib, shape, case):
    from rcdms_amd import hip
    samples, rows, C = shape
    x = _input(shape, case)
    kinds = G.group_kinds(samples, GR, case)
    gamma, beta = G.affine(C)
    xd, gd, bd = gin(torch.from_numpy(x).half(), C + 8), gvec(torch.from_numpy(gamma)), gvec(torch.from_numpy(beta))
    for eps in G.EPS:
        m64, _, r64 = _ref(shape, case, eps)
        for silu in (0, 1):
            d = hip.GroupNormDesc(samples, rows, C, GR, C + 8, C, eps, silu)
            _assert_form(hip, d, shape)
            y = gout(samples * rows, C)
            w = ws(hip.groupnorm_workspace_bytes(d))
            hip.groupnorm_silu(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), w.data_ptr(), w.numel())
            torch.cuda.synchronize()
            check_all(y, xd, gd, bd)
            check_written(y)
            y64 = G.apply64(x, samples, rows, C, GR, m64, r64, gamma, beta, bool(silu))
            G.assert_output(y.float().cpu().numpy(), y64, gamma, C, GR, kinds, samples, rows, bool(silu),
                            f"groupnorm_silu {shape} {case} eps {eps} silu {silu}")


@pytest.mark.parametrize("case", G.CASES)
def test_groupnorm_fold_far_from_zero(hiplib, case):
    """The apply kernel that finalises the groups itself (rcdm_set_groupnorm_fold(1), >= 4 samples): inside the output budget and
    bit-identical to the three-launch form."""
    from rcdms_amd import hip
    shape = G.FOLD_SHAPE
    samples, rows, C = shape
    x = _input(shape, case)
    kinds = G.group_kinds(samples, GR, case)
    gamma, beta = G.affine(C)
    xd, gd, bd = gin(torch.from_numpy(x).half(), C + 8), gvec(torch.from_numpy(gamma)), gvec(torch.from_numpy(beta))
    for eps in G.EPS:
        d = hip.GroupNormDesc(samples, rows, C, GR, C + 8, C, eps, 1)
        _assert_form(hip, d, shape)
        assert _splits(hip, d) <= 128
        outs = []
        try:
            for mode in (0, 1):
                hip.set_groupnorm_fold(mode)
                y = gout(samples * rows, C)
                w = ws(hip.groupnorm_workspace_bytes(d))
                hip.groupnorm_silu(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), w.data_ptr(), w.numel())
                torch.cuda.synchronize()
                outs.append(y)
        finally:
            hip.set_groupnorm_fold(-1)
        check_all(*outs, xd, gd, bd)
        check_written(outs[0]), check_written(outs[1])
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "fold 1 differs from fold 0"
        m64, _, r64 = _ref(shape, case, eps)
        y64 = G.apply64(x, samples, rows, C, GR, m64, r64, gamma, beta, True)
        G.assert_output(outs[1].float().cpu().numpy(), y64, gamma, C, GR, kinds, samples, rows, True, f"fold {shape} {case} eps {eps}")


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("shape", [G.SINGLE_LAUNCH[0], G.THREE_LAUNCH[0], G.THREE_LAUNCH[2]], ids=_ids)
def test_groupnorm_apply_far_from_zero(hiplib, shape, case):
    """rcdm_groupnorm_apply alone, handed the float64 statistics rounded to fp32: the apply arithmetic by itself."""
    from rcdms_amd import hip
    samples, rows, C = shape
    x = _input(shape, case)
    kinds = G.group_kinds(samples, GR, case)
    gamma, beta = G.affine(C)
    xd, gd, bd = gin(torch.from_numpy(x).half(), C + 8), gvec(torch.from_numpy(gamma)), gvec(torch.from_numpy(beta))
    for eps in G.EPS:
        m64, _, r64 = _ref(shape, case, eps)
        st = np.stack([m64, r64], axis=-1).astype(np.float32)
        sd = gvec(torch.from_numpy(st))
        for silu in (0, 1):
            d = hip.GroupNormDesc(samples, rows, C, GR, C + 8, C, eps, silu)
            y = gout(samples * rows, C)
            hip.groupnorm_apply(d, xd.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr())
            torch.cuda.synchronize()
            check_all(y, xd, sd, gd, bd)
            check_written(y)
            y64 = G.apply64(x, samples, rows, C, GR, m64, r64, gamma, beta, bool(silu))
            G.assert_output(y.float().cpu().numpy(), y64, gamma, C, GR, kinds, samples, rows, bool(silu),
                            f"groupnorm_apply {shape} {case} eps {eps} silu {silu}")


# ---- c. producers ---------------------------------------------------------------------------------------------------------------
def _weights(g, cout, k, scale):
    """[cout][k] f16 weights whose GEMM with N(0, 1) inputs has std scale[c] in column c."""
    w = torch.randn(cout, k, generator=g) * k ** -0.5 * torch.from_numpy(scale)[:, None]
    return w.half()


PRODUCERS = [
    # kind, b, f, H, W, cin, cout, split, variant, where the offset sits, cross-frame norm (eps 1e-5) or per-frame (eps 1e-6)
    ("conv", 2, 5, 16, 16, 128, 320, 4, 9, "bias", True),
    ("conv", 2, 5, 16, 16, 128, 320, 4, -1, "rowvec", True),
    ("gemm", 2, 5, 16, 16, 640, 640, 2, -1, "residual", True),
    ("conv+1x1", 2, 5, 16, 16, 128, 320, 4, 9, "bias", True),
    ("conv", 2, 5, 32, 32, 128, 640, 3, -1, "bias", False),    # 1024 rows per frame: a per-frame norm that takes partials
]


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("kind,b,f,H,W,cin,cout,split,variant,where,cross", PRODUCERS,
                         ids=[f"{p[0]}-{p[6]}-v{p[8]}-{p[9]}-{'cross' if p[10] else 'perframe'}" for p in PRODUCERS])
def test_splitk_gnstat_far_from_zero(hiplib, kind, b, f, H, W, cin, cout, split, variant, where, cross, case):
    """The split-K reduce pass that leaves the next norm's partials (cross-frame norm: samples = b, eps 1e-5; per-frame norm:
    samples = images, eps 1e-6), against float64 statistics of the rows it stored; and still bit-identical to the separate
    launches."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(77 + cin + cout + split)
    n_img, M, rps = b * f, b * f * H * W, f * H * W      # rps: rows per row-vector sample (the epilogue's)
    ns, nrows, eps = (b, rps, 1e-5) if cross else (n_img, H * W, 1e-6)      # the norm's samples
    assert cross or where == "bias"
    offset, scale, kinds = G.producer_plan(ns, cout, GR, case, per_sample=(where == "rowvec"))
    zeros = torch.zeros(cout)
    bias = gvec(torch.from_numpy(offset[0]) if where == "bias" else zeros)
    rv = gvec(torch.from_numpy(offset) if where == "rowvec" else torch.zeros(b, cout))     # (row vector: cross-frame cases only, ns = b)
    res = gin((torch.from_numpy(offset[0]).half()[None, :].expand(M, cout) if where == "residual" else torch.zeros(M, cout).half()).contiguous())
    gam, bet = G.affine(cout)
    gamma, beta = gvec(torch.from_numpy(gam)), gvec(torch.from_numpy(bet))
    ldc = cout + 8
    gnd = hip.GroupNormDesc(ns, nrows, cout, GR, ldc, cout, eps, 1)
    epi = 1 | 2 | 4
    x = gin(torch.randn(M, cin, generator=g).half())
    if kind == "conv+1x1":
        cin2 = 192
        x2 = gin(torch.randn(M, cin2, generator=g).half())
        w = gw(_weights(g, cout, 9 * cin + cin2, scale))
        d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin, ldc, cout, epi, rps, cout, 1.0, split, 0, 0, cin2, cin2)
        wsb, ok = hip.conv3x3_workspace_bytes(d), hip.conv3x3_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.conv3x3_add1x1(d, x.data_ptr(), x2.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(),
                                                o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.conv3x3_add1x1_gnstat(d, gnd, x.data_ptr(), x2.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(),
                                                          res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
        ins = [x, x2, w]
    elif kind == "conv":
        w = gw(_weights(g, cout, 9 * cin, scale))
        d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin, ldc, cout, epi, rps, cout, 1.0, split, 0, 0)
        wsb, ok = hip.conv3x3_workspace_bytes(d), hip.conv3x3_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.conv3x3(d, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.conv3x3_gnstat(d, gnd, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(),
                                                   k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
        ins = [x, w]
    else:
        w = gw(_weights(g, cout, cin, scale))
        d = hip.GemmDesc(M, cout, cin, cin, ldc, cout, epi, rps, cout, 1.0, split, 0)
        wsb, ok = hip.gemm_workspace_bytes(d), hip.gemm_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.gemm(d, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.gemm_gnstat(d, gnd, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(),
                                                k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
        ins = [x, w]
    assert wsb > 0 and ok and hip.groupnorm_prestat_ok(gnd), "the pair does not take the statistics-in-the-reduce-pass form"
    hip.set_igemm_variant(variant)
    outs = []
    try:
        for mode in ("separate", "fused"):
            o, y = gout(M, cout, ldc), gout(M, cout)
            stat = gout(1, ns * GR * 2, dtype=torch.float32, guard_rows=1)
            k, gk = ws(wsb), ws(hip.groupnorm_workspace_bytes(gnd))
            if mode == "separate":
                plain(o, k)
                hip.groupnorm_silu(gnd, o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), gk.data_ptr(), gk.numel())
            else:
                fused(o, k, gk)
                hip.groupnorm_stats_prestat(gnd, stat.data_ptr(), gk.data_ptr(), gk.numel())
                hip.groupnorm_silu_prestat(gnd, o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), gk.data_ptr(), gk.numel())
            torch.cuda.synchronize()
            check_all(o, y, *ins, bias, rv, res, gamma, beta)
            check_written(o), check_written(y)
            outs.append((o, y, stat))
    finally:
        hip.set_igemm_variant(-1)
    assert torch.equal(outs[0][0][:, :cout].view(torch.int16), outs[1][0][:, :cout].view(torch.int16)), "the producer's rows differ"
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16)), "the norm's output differs (separate / fused)"
    o, y, stat = outs[1]
    check_all(stat)
    check_written(stat)
    stored = o[:, :cout].float().cpu().numpy()
    G.assert_stored_band(stored, ns, nrows, cout, GR, kinds)
    what = f"{kind} v{variant} {where} {case} eps {eps}"
    G.assert_stats(*_stats(stat, ns), stored, ns, nrows, cout, GR, eps, kinds, f"gnstat {what}")
    m64, _, r64, y64 = G.reference(stored, ns, nrows, cout, GR, eps, gam, bet, True)
    G.assert_output(y.float().cpu().numpy(), y64, gam, cout, GR, kinds, ns, nrows, True, f"silu_prestat {what}")


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("cin,cout", [(64, 320), (128, 640)])
def test_wino_gn_out_far_from_zero(hiplib, cin, cout, case):
    """The Winograd output transform's per-tile partials (one per 2x2 tile) + rcdm_groupnorm_finalize, for the cross-frame norm
    (one sample of 5 frames, eps 1e-5) and the per-frame norm (5 samples, eps 1e-6) behind the conv, against float64 statistics
    of the stored rows."""
    from rcdms_amd import hip
    n_img, H, W = 5, 16, 16
    M = n_img * H * W
    g = torch.Generator().manual_seed(78 + cin + cout)
    offset, scale, kinds1 = G.producer_plan(1, cout, GR, case, per_sample=False)
    x = gin(torch.randn(M, cin, generator=g).half(), cin + 8)
    w32 = gvec(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5 * torch.from_numpy(scale)[:, None, None, None])
    bias = gvec(torch.from_numpy(offset[0]))
    U = gout(16 * cout, cin)
    hip.pack_conv3x3_wino(w32.data_ptr(), cout, cin, U.data_ptr())
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin + 8, cout, 0, 1, n_img * H * W, cout, 1.0, 0, 0, 0, 0, 0)
    assert hip.conv3x3_wino_supported(d)
    wsb = ws(hip.conv3x3_wino_workspace_bytes(d))
    for samples, eps in ((1, 1e-5), (n_img, 1e-6)):
        rps = M // samples
        kinds = np.repeat(kinds1, samples, axis=0)
        god = hip.GroupNormDesc(samples, rps, cout, GR, cout, cout, eps, 0)
        part = ws(samples * GR * (rps // 4) * 3 * 4)
        out = gout(M, cout)
        hip.conv3x3_wino(d, x.data_ptr(), U.data_ptr(), bias.data_ptr(), 0, 0, out.data_ptr(), wsb.data_ptr(), wsb.numel(),
                         gn_out=god, gn_out_partial=part.data_ptr())
        stat = gout(1, samples * GR * 2, dtype=torch.float32, guard_rows=1)
        hip.groupnorm_finalize(samples, GR, rps // 4, eps, part.data_ptr(), stat.data_ptr())
        torch.cuda.synchronize()
        check_all(out, stat, x, w32, bias, U)
        check_written(out), check_written(stat)
        stored = out.float().cpu().numpy()
        G.assert_stored_band(stored, samples, rps, cout, GR, kinds)
        G.assert_stats(*_stats(stat, samples), stored, samples, rps, cout, GR, eps, kinds,
                       f"wino gn_out {cin}->{cout} {case} samples {samples} eps {eps}")
