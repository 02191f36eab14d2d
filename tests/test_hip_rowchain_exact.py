"""GPU: exact-answer tests of the row chains and the fused feed-forward — rcdm_rowchain with every tail (q / q|k|v GEMM,
feed-forward, feed-forward + trailing projection, q|k|v + temporal attention), with and without the stage-A residual, pe
and the GroupNorm prologue, and rcdm_ff_fused — through their packers (rcdm_pack_rowchain, rcdm_pack_ff_stream).

The operands are the small integers of tests/rowchain_exact.py, the reference is its float64 model, and the token rows and
the tail's output are compared with torch.equal: a k-step that reads zeros, a stale ring slot, a bias paired with the wrong
hidden unit, a pe row or a GroupNorm sample off by one changes an integer.  Before a launch the conditions that make the
answer exact are asserted on the reference alone (check_case).  The one comparison with a tolerance is the tail output of
the dense stage A without a residual (sections A and B, "-dense"): its token rows are compared bit for bit, but they are not
two-valued, so the LayerNorm behind them has no single right f16 answer and the output goes through close() against the
float64 chain started from those token rows.

Tail 4 runs WITHOUT pe here: the pe row map of the frame-major blocks stays with tests/test_hip_motion_fused.py (as do GELU
between its saturated ends and LayerNorm on rows that are not two-valued, with tests/test_hip_rowff.py).

Buffers are guarded (tests/guard.py): row strides above C, poisoned pad columns and guard rows on the way in, NaN on the way
out, check_all / check_out after every launch."""
import pytest
import torch

from tests import rowchain_exact as R
from tests.guard import check_all, check_out, check_written
from tests.test_hip_gemm_exact import exact, t16, t32
from tests.test_hip_kernels import DEV, close, gin, gout, gvec

pytestmark = pytest.mark.gpu

C = R.C
LDA, LDR, LDT, LDZ = C + 24, C + 32, C + 8, C + 40       # every stride above C, all different


def _names(cases):
    return [s["name"] for s in cases]


def _launch(hip, c):
    """Pack, launch once, synchronise, check every guard.  Returns (tok or None, out, ncol)."""
    M, tail, alias = c["M"], c["tail"], c["alias"]
    ff = tail in (0, 2)
    ncol = tail * C if tail in (1, 3) else C
    ln_g, ln_b = gvec(t32(c["ln_g"])), gvec(t32(c["ln_b"]))
    ins = [ln_g, ln_b]
    w1 = b1 = w2 = b2 = b1p = None
    if ff:
        w1, b1, w2, b2 = gin(t32(c["w1"])), gvec(t32(c["b1"])), gin(t32(c["w2"])), gvec(t32(c["b2"]))
        b1p = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
        ins += [w1, b1, w2, b2]
    ptr = lambda t: 0 if t is None else t.data_ptr()

    if c["form"] == "ff":
        ws = gout(1, hip.ff_stream_bytes(C), dtype=torch.uint8, guard_rows=1)
        hip.pack_ff_stream(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), C, ws.data_ptr(), b1p.data_ptr())
        x16 = gin(t16(c["a"]), LDA)
        out = gout(M, C, LDT)
        hip.ff_fused(hip.FFDesc(M, C, LDA, LDT, R.EPS), x16.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), ws.data_ptr(), b1p.data_ptr(),
                     b2.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        check_all(ws, b1p, x16, out, *ins)
        check_written(out)
        return None, out, C

    wa, ba = gin(t32(c["wa"])), gvec(t32(c["ba"]))
    wt = gin(t32(c["wz"] if tail == 2 else c["wt"])) if tail else None
    pe = gin(t32(c["pe"])) if c["pe"] is not None else None
    ins += [t for t in (wa, ba, wt, pe) if t is not None]
    ws = gout(1, hip.rowchain_stream_bytes(C, tail), dtype=torch.uint8, guard_rows=1)
    hip.pack_rowchain(wa.data_ptr(), C, tail, ptr(wt), ptr(w1), ptr(b1), ptr(w2), ws.data_ptr(), ptr(b1p))

    has_res = c["res"] is not None
    ldo = ncol + 16
    if alias is None:
        a16 = gin(t16(c["a"]), LDA)
        res16 = gin(t16(c["res"]), LDR) if has_res else None
        tok, out = gout(M, C, LDT), gout(M, ncol, ldo)
        ins += [a16] + ([res16] if has_res else [])
    else:
        assert has_res
        tok = gout(M, C, LDT)                                 # the residual stream, updated in place
        tok[:, :C] = t16(c["res"]).to(DEV)
        res16 = tok
        if alias == "engine":                                 # tail 4 as the plan calls it: the output over the input rows
            out = gout(M, C, LDA)
            out[:, :C] = t16(c["a"]).to(DEV)
            a16, ldo = out, LDA
        else:
            a16 = gin(t16(c["a"]), LDA)
            ins.append(a16)
            out, ldo = (tok, LDT) if alias == "tok+out" else (gout(M, ncol, ldo), ldo)
    gn = c["gn"]
    gst = gg = gb = z16 = bz = None
    if gn is not None:
        gst, gg, gb = gvec(t32(gn["stat"])), gvec(t32(gn["gamma"])), gvec(t32(gn["beta"]))
        ins += [gst, gg, gb]
    if tail == 2:
        z16, bz = gin(t16(c["zres"]), LDZ), gvec(t32(c["bz"]))
        ins += [z16, bz]
    d = hip.RowChainDesc(M, C, a16.stride(0), res16.stride(0) if has_res else 0, tok.stride(0), ldo, tail, c["rpf"], c["frames"], R.EPS,
                         R.GN_GROUPS if gn else 0, gn["rows"] if gn else 0, LDZ if tail == 2 else 0)
    hip.rowchain(d, a16.data_ptr(), ptr(res16) if has_res else 0, tok.data_ptr(), ba.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), ptr(pe),
                 ws.data_ptr(), ptr(b1p), ptr(b2), out.data_ptr(), gn_stat=ptr(gst), gn_g=ptr(gg), gn_b=ptr(gb), z_res=ptr(z16), z_bias=ptr(bz))
    torch.cuda.synchronize()
    check_all(ws, tok, out, *ins, *([b1p] if ff else []))
    check_written(tok)
    check_written(out)
    return (None if alias == "tok+out" else tok), out, ncol


def _compare(c, tok, out, ncol, what=""):
    ref = c["ref"]
    if tok is not None:
        exact(tok[:, :C], ref["tok"], f"{c['name']} {what}tok: ")
    if c["exact_ln"]:
        exact(out[:, :ncol], ref["out"], f"{c['name']} {what}out: ")
    else:
        close(out[:, :ncol], t32(ref["out"]))


def _run(hip, name):
    c = R.case(name)
    R.check_case(c)
    if c["form"] == "chain":
        assert hip.rowchain_config_supported(C, c["tail"], c["pe_frames"])
    tok, out, ncol = _launch(hip, c)
    _compare(c, tok, out, ncol)
    return c, tok, out, ncol


@pytest.mark.parametrize("name", _names(R.CASES_A))
def test_stage_a(hiplib, name):
    """tok = a W_a^T + b_a (+ res) bit for bit in every instantiation; with a residual or a signed-permutation W_a the rows are
    two-valued and everything behind them is exact in the same launch; tok over res, tails 0 and 2 where the engine writes."""
    from rcdms_amd import hip
    _run(hip, name)


@pytest.mark.parametrize("name", _names(R.CASES_B))
def test_groupnorm_prologue(hiplib, name):
    """Statistics supplied by the test: every (sample, group) has its own (mean, rstd), so a wrong sample or group index for
    any wave of a block that straddles two samples changes integers."""
    from rcdms_amd import hip
    _run(hip, name)


@pytest.mark.parametrize("name", _names(R.CASES_C))
def test_layernorm_pe_tail_gemm(hiplib, name):
    from rcdms_amd import hip
    _run(hip, name)


@pytest.mark.parametrize("name", _names(R.CASES_D))
def test_feed_forward(hiplib, name):
    """Hidden-dense (every phase: each hidden unit is on in exactly one launch) and gate-dense, through rcdm_ff_fused, tail 0 and
    tail 2 (whose trailing projection is a signed permutation)."""
    from rcdms_amd import hip
    _run(hip, name)


@pytest.mark.parametrize("name", _names(R.CASES_E))
def test_temporal_attention_tail(hiplib, name):
    """Unity: the five frames of a pixel share their token row, so out == the row's v whatever the scores.  Selection:
    q_f = t k_(f + 1), so out[f] == v[(f + 1) % 5] of the same pixel.  No pe here (tests/test_hip_motion_fused.py has the pe
    row map of the frame-major blocks)."""
    from rcdms_amd import hip
    _run(hip, name)


@pytest.mark.parametrize("name", R.CASES_F)
def test_two_launches_agree(hiplib, name):
    """The same case launched twice into separate buffers: both exact (which implies bit-identical); asserted separately so
    that a failure names the launch."""
    from rcdms_amd import hip
    c, tok1, out1, ncol = _run(hip, name)
    tok2, out2, _ = _launch(hip, c)
    _compare(c, tok2, out2, ncol, "second launch, ")
    assert torch.equal(tok1[:, :C], tok2[:, :C]) and torch.equal(out1[:, :ncol], out2[:, :ncol])
