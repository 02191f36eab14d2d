"""GPU: every site that evaluates a pointwise transcendental — erf GELU in its two polynomial forms, quick-GELU, SiLU, Mish,
the sinusoidal timestep embedding — on every f16 input (tests/act_sweep.py: GRID16, GRID_FF, and the same values off the f16
grid for the fp32 sites) against float64, inside the derived budget rounding + form + evaluation of that module.  The
operands are chosen so that the pre-activation reaches the function EXACTLY (identity weights, zero bias, two-valued norm
rows): the budget needs no term for it.  No value of a grid is skipped or masked; every test prints its largest
|err| / budget and where it occurred, and for the f16 outputs whether the site keeps or flushes f16 subnormals.

Roundings to f16 per site (n of the rounding term), read from the code:
  GEMM epilogues, LDS-staged (igemm.hip, igemm_epilogue.h)   the accumulator is staged as f16 first — here the f16
      pre-activation itself, exactly — then bias + activation in fp32 and ONE rounding of (v + residual) * out_scale     n = 1
  split-K reduce (epilogue_store)   fp32 (or, f16 slabs, exact) partials summed, activation, one rounding                n = 1
  GEGLU (geglu8 / epilogue_store)   (h + bh) * gelu(g + bg) * scale in fp32, one rounding                                n = 1
  fused feed-forward (geglu_slice)  (ah + bh) * gelu in fp32, one rounding to the GEMM2 operand; everything behind it
      (2^13 h, + b2, + residual) is exact or rounded away by construction (act_sweep.ff_case)                            n = 1
  GroupNorm apply (both kernels)    fma in fp32, silu_f, one rounding                                                    n = 1
  rcdm_small_linear, rcdm_mish, rcdm_timestep_embed   fp32 in and out                                                    n = 0

The Winograd input transform (wino.hip) calls the same silu_f and is left out on purpose: its values are summed by the
transform before anything can be observed.

Buffers are guarded (tests/guard.py); check_all after every launch."""
import numpy as np
import pytest
import torch

from tests import act_sweep as A
from tests.guard import check_all, check_written
from tests.test_hip_gemm_exact import t16, t32
from tests.test_hip_kernels import gin, gout, gvec, gw, ws

pytestmark = pytest.mark.gpu

X64 = A.GRID16.astype(np.float64)
K = 128                                  # N = K = 128: one tile column of every variant, and two k-steps for the forced split
M = -(-A.GRID16.size // K)               # 481 rows; the 126 values of padding are zeros (a grid value)
DMA, PP = (1, 2, 3, 4, 5, 10), (6, 7, 8)      # tile variants of igemm_dma / igemm8; 9 is igemm16 (igemm_plan.h)


def _rows(vals, cols, dtype=np.float64):
    """vals row by row into [rows][cols], zero-padded."""
    rows = -(-vals.size // cols)
    a = np.zeros(rows * cols, dtype=dtype)
    a[:vals.size] = vals
    return a.reshape(rows, cols)


XG = _rows(X64, K)
_REF = {}


def ref_of(kind):
    """The float64 reference on the GEMM operand, computed once, shared, never modified."""
    if kind not in _REF:
        _REF[kind] = {"gelu": A.gelu64, "quick": A.quick64}[kind](XG)
        _REF[kind].setflags(write=False)
    return _REF[kind]


def subnormals(got, ref):
    """keeps | flushes | n/a: what the site does with results in the f16 subnormal range."""
    sub = (np.abs(ref) < 2.0 ** -14) & (np.abs(ref) >= 2.0 ** -23)
    if not sub.any():
        return "n/a"
    return "keeps" if (got[sub] != 0).any() else "flushes"


F16_OVER = 65520.0       # the first magnitude that rounds to infinity in f16


def judge(site, got, ref, bud, where, f16_out=True):
    """Every element: |got - ref| <= budget.  An f16 output whose true value rounds to infinity (GEGLU with hidden -1.5 on the
    largest gates: -1.5 * 65504) has to BE that infinity — compared as such, not left out; within the budget of the
    overflow threshold either answer is right."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bud.shape, (got.shape, ref.shape, bud.shape)
    where = np.broadcast_to(np.asarray(where, dtype=np.float64), got.shape)
    must_inf = (np.abs(ref) - bud >= F16_OVER) if f16_out else np.zeros(got.shape, dtype=bool)
    may_inf = (np.abs(ref) + bud >= F16_OVER) if f16_out else must_inf
    assert not np.isnan(got).any(), f"{site}: NaN at x = {where[np.isnan(got)][:4]}"
    inf = np.isinf(got)
    assert (inf <= may_inf).all(), f"{site}: infinite output at x = {where[inf & ~may_inf][:4]}"
    assert inf[must_inf].all() and (np.sign(got[inf]) == np.sign(ref[inf])).all(), f"{site}: an overflow that is not the signed infinity"
    err = np.where(inf, 0.0, np.abs(np.where(inf, ref, got) - ref))
    r, at = A.worst(err, bud, where)
    sub = f"; f16 subnormals: {subnormals(got, ref)}" if f16_out else ""
    over = f"; {int(inf.sum())} overflow to the signed infinity, as they must" if inf.any() else ""
    print(f"[act_sweep] {site}: max |err| / budget {r:.4f} at x = {at:.9g} over {got.size} values{sub}{over}")
    assert r <= 1.0, f"{site}: {r:.4f} of the budget at x = {at:.9g}"
    return r


def _site(plan_variant, splits, quick):
    if splits > 1:
        return "split-K reduce, epilogue_store<QG> (igemm.hip)" if quick else "split-K reduce, epilogue_store (igemm.hip)"
    if plan_variant in DMA:
        return "LDS-staged igemm_dma_kernel, LX = 4 (igemm.hip)" if quick else "LDS-staged igemm_dma_kernel (igemm.hip)"
    return ("igemm8" if plan_variant in PP else "igemm16") + " shared epilogue, act8 / gelu8 (igemm_epilogue.h)"


@pytest.fixture(scope="module")
def gemm_operands(hiplib):
    A16 = gin(t16(XG), K + 8)
    W = gw(t16(np.eye(K)))
    bias = gvec(torch.zeros(K))
    return A16, W, bias


# ---- 1. GELU and quick-GELU epilogues -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gelu", "quick"])
def test_gemm_epilogues(hiplib, gemm_operands, kind):
    """out = act(A I^T + 0): the accumulator is x * 1 plus zeros.  Every tile variant, unsplit and split in two (the reduce
    kernel has its own epilogue), and the plan query has to show that between them the variants reached every tile kernel
    with an activation in its epilogue."""
    from rcdms_amd import hip
    A16, W, bias = gemm_operands
    quick = kind == "quick"
    epi = hip.EPI_BIAS | (hip.EPI_QUICK_GELU if quick else hip.EPI_GELU)
    ref = ref_of(kind)
    bud = A.budget("quick" if quick else "gelu3", XG, ref, n_round=1)
    want = {_site(v, s, quick) for v in (1, 6, 9) for s in (1, 2)}
    reached, worst = {}, 0.0
    try:
        for variant in range(1, 11):
            for split in (1, 2):
                hip.set_igemm_variant(variant)
                d = hip.GemmDesc(M, K, K, K + 8, K + 16, 0, epi, 1, 0, 1.0, split)
                plan = hip.gemm_plan_query(d)
                assert plan["splits"] == split, plan
                site = _site(plan["variant"], plan["splits"], quick)
                reached.setdefault(site, []).append((variant, plan["variant"]))
                out = gout(M, K, K + 16)
                w = ws(hip.gemm_workspace_bytes(d))
                hip.gemm(d, A16.data_ptr(), W.data_ptr(), bias.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
                torch.cuda.synchronize()
                check_all(out, A16, W, bias)
                check_written(out)
                worst = max(worst, judge(f"{kind} variant {variant} (runs as {plan['variant']}) split {split}, {site}",
                                         out[:, :K].cpu().double().numpy(), ref, bud, XG))
    finally:
        hip.set_igemm_variant(-1)
    for site in sorted(want):
        assert site in reached, f"no variant reached {site}"
        print(f"[act_sweep] reached {site}: forced variant (ran as) {reached[site]}")
    assert set(reached) == want, set(reached) - want
    assert {p for v in reached.values() for _, p in v} >= ({1, 3, 4, 5, 6, 7, 8, 9, 10} | (set() if quick else {2}))
    print(f"[act_sweep] {kind} GEMM epilogues, all variants: max {worst:.4f}")


# ---- 2. GEGLU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hb", [1.0, -1.5])
def test_geglu(hiplib, gemm_operands, hb):
    """Gate rows: the identity; hidden rows: zero with bias hb, so out = f16(hb * gelu(x)) — hb = 1 the function alone,
    hb = -1.5 the sign and the single rounding of the product.  Weights through rcdm_pack_geglu_rows.  Sites:
    the GEGLU branch of epilogue_store (split-K reduce), geglu8 of the LDS-staged igemm_dma_kernel and of the shared epilogue
    of igemm8 / igemm16 (igemm_epilogue.h)."""
    from rcdms_amd import hip
    A16 = gemm_operands[0]
    w = np.zeros((2 * K, K))
    w[K + np.arange(K), np.arange(K)] = 1.0
    b = np.zeros(2 * K)
    b[:K] = hb
    w32, b32 = gin(t32(w)), gvec(t32(b))
    wp = gout(2 * K, K)
    bp = gout(1, 2 * K, dtype=torch.float32, guard_rows=1)
    hip.pack_geglu_rows(w32.data_ptr(), b32.data_ptr(), 2 * K, K, wp.data_ptr(), bp.data_ptr())
    torch.cuda.synchronize()
    check_all(wp, bp, w32, b32)
    ref = hb * ref_of("gelu")
    bud = A.budget("gelu3", XG, ref, n_round=1, scale=hb)

    def site_of(pv, splits):
        if splits > 1:
            return "split-K reduce, epilogue_store GEGLU branch (igemm.hip)"
        return "geglu8, LDS-staged igemm_dma_kernel (igemm.hip)" if pv in DMA else \
            ("igemm8" if pv in PP else "igemm16") + " shared epilogue, geglu8 (igemm_epilogue.h)"

    want = {site_of(v, s) for v in (1, 6, 9) for s in (1, 2)}
    reached, worst = {}, 0.0
    try:
        for variant in range(1, 11):
            for split in (1, 2):
                hip.set_igemm_variant(variant)
                d = hip.GemmDesc(M, 2 * K, K, K + 8, K + 16, 0, hip.EPI_BIAS | hip.EPI_GEGLU, 1, 0, 1.0, split)
                plan = hip.gemm_plan_query(d)
                assert plan["splits"] == split, plan
                site = site_of(plan["variant"], plan["splits"])
                reached.setdefault(site, []).append((variant, plan["variant"]))
                out = gout(M, K, K + 16)
                wsp = ws(hip.gemm_workspace_bytes(d))
                hip.gemm(d, A16.data_ptr(), wp.data_ptr(), bp.data_ptr(), 0, 0, out.data_ptr(), wsp.data_ptr(), wsp.numel())
                torch.cuda.synchronize()
                check_all(out, A16, wp, bp)
                check_written(out)
                worst = max(worst, judge(f"GEGLU hidden {hb} variant {variant} (runs as {plan['variant']}) split {split}, {site}",
                                         out[:, :K].cpu().double().numpy(), ref, bud, XG))
    finally:
        hip.set_igemm_variant(-1)
    for site in sorted(want):
        assert site in reached, f"no variant reached {site}"
        print(f"[act_sweep] reached {site}: forced variant (ran as) {reached[site]}")
    print(f"[act_sweep] GEGLU hidden bias {hb}, all variants: max {worst:.4f}")


# ---- 3. the fused feed-forward: the five-term form ----------------------------------------------------------------------------
def _ff_chain_case(c, form):
    """act_sweep.ff_case as a case of tests/test_hip_rowchain_exact._launch: rcdm_ff_fused, or rcdm_rowchain with tail 0 behind
    an identity stage A (tok = a exactly)."""
    C = A.FF_C
    d = dict(name="act-sweep", form=form, tail=0, M=A.FF_M, alias=None, ln_g=c["ln_g"], ln_b=c["ln_b"], w1=c["w1"], b1=c["b1"],
             w2=c["w2"], b2=c["b2"], a=c["tok"], pe=None, res=None, gn=None, rpf=1, frames=1, pe_frames=0)
    if form == "chain":
        d.update(wa=np.eye(C), ba=np.zeros(C))
    return d


@pytest.mark.parametrize("form", ["ff", "chain"])
def test_fused_feed_forward(hiplib, form):
    """rcdm_ff_fused and the feed-forward tail of rcdm_rowchain on GRID_FF, 320 gate values per launch, h read back bit for bit
    as out / 2^13 (act_sweep.ff_case asserts the conditions on the reference before the launch).  Judged by the FIVE-term
    budget only: the three-term budget would also let the three-term form through."""
    from rcdms_amd import hip
    from tests.test_hip_rowchain_exact import _launch
    if form == "chain":
        assert hip.rowchain_config_supported(A.FF_C, 0, 0)
    else:
        assert hip.ff_fused_supported(A.FF_C)
    worst, at_worst, seen = 0.0, 0.0, 0
    for i in range(0, A.GRID_FF.size, A.FF_C):
        c = A.ff_case(A.GRID_FF[i:i + A.FF_C])
        tok, out, _ = _launch(hip, _ff_chain_case(c, form))
        got = out[:, :A.FF_C].cpu().double().numpy()
        if tok is not None:
            assert (tok[:, :A.FF_C].cpu().double().numpy() == c["tok"]).all(), "stage A did not pass the token rows through"
        h = np.where(c["zero"][None, :], got - c["tok"], got) / A.FF_SCALE
        x = np.broadcast_to(c["vals"][None, :], h.shape)
        ref = np.broadcast_to(c["h_ref"][None, :], h.shape)
        bud = A.budget("gelu5", x, ref, n_round=1, scale=np.broadcast_to(c["p"][None, :], h.shape))
        assert np.isfinite(got).all(), f"non-finite output, launch {i // A.FF_C}"
        zero_cols = np.broadcast_to(c["zero"][None, :], h.shape)
        assert (got[zero_cols] == c["tok"][zero_cols]).all(), "a column whose true h is 0 does not return the token row"
        r, at = A.worst(np.abs(h - ref), bud, x)
        if r > worst:
            worst, at_worst = r, at
        seen += c["n"]
    assert seen == A.GRID_FF.size
    print(f"[act_sweep] fused feed-forward ({'rcdm_ff_fused' if form == 'ff' else 'rcdm_rowchain tail 0'}), geglu_slice (rowff.hip): max |err| / "
          f"five-term budget {worst:.4f} at gate {at_worst:.9g} over {seen} gate values x {A.FF_M} rows")
    assert worst <= 1.0


# ---- 4. SiLU, f16 out ---------------------------------------------------------------------------------------------------
GN_C = 320


@pytest.mark.parametrize("silu", [1, 0])
def test_groupnorm_apply_silu(hiplib, silu):
    """rcdm_groupnorm_apply (gn_apply_kernel) with statistics (mean 0, rstd 1), gamma 1 and beta -0.0 (a zero
    whose sum with the zero shift keeps the sign of a -0 input): the pre-activation is x itself, so silu = 0 has to return
    the input bit for bit."""
    from rcdms_amd import hip
    xg = _rows(X64, GN_C)
    rows = xg.shape[0]
    groups = 32
    st = np.zeros((1, groups, 2))
    st[..., 1] = 1.0
    xd, sd, gd, bd = gin(t16(xg), GN_C + 8), gvec(t32(st)), gvec(torch.ones(GN_C)), gvec(torch.full((GN_C,), -0.0))
    y = gout(rows, GN_C, GN_C + 24)
    d = hip.GroupNormDesc(1, rows, GN_C, groups, GN_C + 8, GN_C + 24, 1e-5, silu)
    hip.groupnorm_apply(d, xd.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    check_all(y, xd, sd, gd, bd)
    check_written(y)
    if silu:
        ref = A.silu64(xg)
        judge("SiLU, rcdm_groupnorm_apply (gn_apply_kernel)", y[:, :GN_C].cpu().double().numpy(), ref, A.budget("silu", xg, ref, n_round=1), xg)
    else:
        same = torch.equal(y[:, :GN_C].cpu().view(torch.int16), xd[:, :GN_C].cpu().view(torch.int16))
        print(f"[act_sweep] rcdm_groupnorm_apply, silu = 0: output {'==' if same else '!='} input bit for bit over {xg.size} values")
        assert same


FUSED_C, FUSED_G, FUSED_P, GN_EPS = 7680, 64, 8, 1e-5


def test_groupnorm_fused_silu(hiplib):
    """The self-finalising kernel (gn_fused_kernel) through rcdm_groupnorm_silu: rows of +1 and -1 in turn, so
    every group is two-valued with mean 0 and variance 1; gamma = the swept values (7680 per launch), beta 0: the
    pre-activation is +-gamma_c / sqrt(1 + eps), formed by the kernel in fp32 (1.1 * 4 u |f| more in the budget)."""
    from rcdms_amd import hip
    x = np.tile(np.where(np.arange(FUSED_P) % 2 == 0, 1.0, -1.0)[:, None], (1, FUSED_C))
    d = hip.GroupNormDesc(1, FUSED_P, FUSED_C, FUSED_G, FUSED_C + 8, FUSED_C + 24, GN_EPS, 1)
    assert not hip.groupnorm_prestat_ok(d), "this shape is meant to take the single-launch form"
    xd, bd = gin(t16(x), FUSED_C + 8), gvec(torch.zeros(FUSED_C))
    wsp = ws(hip.groupnorm_workspace_bytes(d))
    rstd = 1.0 / np.sqrt(1.0 + float(np.float32(GN_EPS)))
    gam = _rows(X64, FUSED_C)
    worst, at_worst, kept = 0.0, 0.0, set()
    for i in range(gam.shape[0]):
        gd = gvec(t32(gam[i]))
        y = gout(FUSED_P, FUSED_C, FUSED_C + 24)
        hip.groupnorm_silu(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), wsp.data_ptr(), wsp.numel())
        torch.cuda.synchronize()
        check_all(y, xd, gd, bd)
        check_written(y)
        f = x * gam[i][None, :] * rstd
        ref = A.silu64(f)
        got = y[:, :FUSED_C].cpu().double().numpy()
        assert np.isfinite(got).all()
        r, at = A.worst(np.abs(got - ref), A.budget("silu", f, ref, n_round=1, extra=1.1 * 4 * A.U * np.abs(f)), f)
        if r > worst:
            worst, at_worst = r, at
        kept.add(subnormals(got, ref))
    print(f"[act_sweep] SiLU, rcdm_groupnorm_silu single launch (gn_fused_kernel): max |err| / budget {worst:.4f} at f = {at_worst:.9g} over "
          f"{gam.size} gammas x {FUSED_P} rows; f16 subnormals: {sorted(kept - {'n/a'})}")
    assert worst <= 1.0


# ---- 5. SiLU, fp32 in and out -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_args():
    xs = A.off_grid(A.GRID16)
    assert xs.min() < -87.3 and xs.max() > 88
    return xs


@pytest.mark.parametrize("rows", [8, 1])
@pytest.mark.parametrize("where", ["silu_in", "silu_out"])
def test_small_linear_silu(hiplib, fp32_args, where, rows):
    """rcdm_small_linear (small_linear_kernel: on the staged input, on the output) with W the identity (K = N = 64): out = silu(x) or silu(x * 1 + zeros), fp32 in and
    out, on the f16 values and on the same values times 1 + 2^-13; every launch takes `rows` rows of one big guarded pair of
    buffers."""
    from rcdms_amd import hip
    KN = 64
    xg = _rows(fp32_args, 8 * KN, dtype=np.float32).reshape(-1, KN)
    n_rows = xg.shape[0]
    xd = gin(torch.from_numpy(xg), KN)
    W = gw(t16(np.eye(KN)))
    out = gout(n_rows, KN, dtype=torch.float32)
    si, so = (1, 0) if where == "silu_in" else (0, 1)
    for r0 in range(0, n_rows, rows):
        hip.small_linear(xd.data_ptr() + r0 * KN * 4, rows, KN, W.data_ptr(), 0, KN, si, so, out.data_ptr() + r0 * KN * 4)
    torch.cuda.synchronize()
    check_all(out, xd, W)
    check_written(out)
    x64 = xg.astype(np.float64)
    ref = A.silu64(x64)
    judge(f"SiLU, rcdm_small_linear {where}, {rows} row(s) per launch (small_linear_kernel)", out.cpu().double().numpy(), ref,
          A.budget("silu", x64, ref), x64, f16_out=False)


# ---- 6. Mish ------------------------------------------------------------------------------------------------------------
def test_mish(hiplib, fp32_args):
    """rcdm_mish on the same fp32 arguments and on softplus's threshold 20 with both of its neighbours; relative budget."""
    from rcdms_amd import hip
    t = np.float32(20.0)
    x = np.concatenate([fp32_args, [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(99))]]).astype(np.float32)
    xd = gvec(torch.from_numpy(x))
    y = gout(1, x.size, dtype=torch.float32, guard_rows=1)
    hip.mish(xd.data_ptr(), y.data_ptr(), x.size)
    torch.cuda.synchronize()
    check_all(y, xd)
    check_written(y)
    x64 = x.astype(np.float64)
    ref = A.mish64(x64)
    judge("Mish, rcdm_mish (mish_kernel)", y[0].cpu().double().numpy(), ref, A.budget("mish", x64, ref), x64, f16_out=False)


# ---- 7. the timestep embedding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", A.TEMB_ROWS)
@pytest.mark.parametrize("dim", A.TEMB_DIMS)
def test_timestep_embed(hiplib, dim, rows):
    from rcdms_amd import hip
    t = A.temb_rows(rows)
    td = gvec(torch.from_numpy(t))
    out = gout(rows, dim, dtype=torch.float32)
    hip.timestep_embed(td.data_ptr(), rows, dim, out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, td)
    check_written(out)
    ref = A.temb64(t, dim)
    judge(f"timestep embedding dim {dim} rows {rows} (timestep_embed_kernel)", out.cpu().double().numpy(), ref, A.budget_temb(t, dim),
          np.broadcast_to(t.astype(np.float64)[:, None], ref.shape), f16_out=False)
