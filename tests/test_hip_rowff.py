"""GPU parity of the row-stationary fused feed-forward (rcdm_ff_fused, rowff.hip) against the reference arithmetic
out = x + FeedForward_geglu(LayerNorm(x))  (attention.py:514 / motion_module.py:243; diffusers FeedForward "geglu":
Linear(C -> 8C), hidden * gelu(gate) with the exact erf GELU, Linear(4C -> C)) on f16-rounded inputs, and against the
unfused three-launch path of the library (rcdm_layernorm + rcdm_gemm GEGLU + rcdm_gemm bias + residual).

Tolerance: |hip - ref| <= 4e-3 * max|ref| + 2e-3 * |ref| (tests/test_hip_kernels.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests.guard import check_all, check_in, check_out
from tests.test_hip_kernels import DEV, close, gin, gout, gvec, gw, h16

pytestmark = pytest.mark.gpu


def _dev(w):
    """The fp32 parameters of a block on the device, each inside poison (matrices as rows, vectors 16-byte aligned)."""
    return {k: (None if v is None else gin(v.float()) if v.dim() == 2 else gvec(v)) for k, v in w.items()}


def _weights(C, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(
        ln_g=1.0 + 0.2 * torch.randn(C, generator=g), ln_b=0.1 * torch.randn(C, generator=g),
        w1=h16(torch.randn(8 * C, C, generator=g) * C ** -0.5), b1=0.1 * torch.randn(8 * C, generator=g),
        w2=h16(torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5), b2=0.1 * torch.randn(C, generator=g)), g


def _reference(x, w):
    C = x.shape[1]
    a = h16(F.layer_norm(x, (C,), w["ln_g"], w["ln_b"], 1e-5))       # the MFMA operand is f16
    hg = F.linear(a, w["w1"], w["b1"])
    hidden, gate = hg.chunk(2, dim=-1)
    return x + F.linear(h16(hidden * F.gelu(gate)), w["w2"], w["b2"])


def _run_fused(x16, ld, w, out=None, M=None):
    from rcdms_amd import hip
    M, C = M or x16.shape[0], w["ln_g"].numel()
    dev = _dev(w)
    ws = gout(1, hip.ff_stream_bytes(C), dtype=torch.uint8, guard_rows=1)
    b1p = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    hip.pack_ff_stream(dev["w1"].data_ptr(), dev["b1"].data_ptr(), dev["w2"].data_ptr(), C, ws.data_ptr(), b1p.data_ptr())
    if out is None:
        out = gout(M, C, ld)
    d = hip.FFDesc(M, C, ld, out.stride(0), 1e-5)
    hip.ff_fused(d, x16.data_ptr(), dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), ws.data_ptr(), b1p.data_ptr(),
                 dev["b2"].data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(ws, b1p, *dev.values())
    return out


@pytest.mark.parametrize("M", [160, 16, 333, 2560])   # one block; one wave; ragged tail; many blocks
def test_ff_fused_vs_reference(hiplib, M):
    _ff_fused_vs_reference(M, 64, 8)                      # rows inside wider buffers, the two strides different


@pytest.mark.parametrize("M", [160, 16, 333, 2560])
def test_ff_fused_vs_reference_one_stride(hiplib, M):
    _ff_fused_vs_reference(M, 64, 64)                     # input and output rows at the same stride


def _ff_fused_vs_reference(M, pad_x, pad_o):
    from rcdms_amd import hip
    C = 320
    assert hip.ff_fused_supported(C)
    w, g = _weights(C, 11 + M)
    x = h16(torch.randn(M, C, generator=g) * 1.5 + 0.3)
    ref = _reference(x, w)
    ld, ldo = C + pad_x, C + pad_o
    xb = gin(x.half(), ld)                                # pad columns / guard rows: poison on the way in ...
    out = gout(M, C, ldo)                                 # ... NaN on the way out, and they must stay untouched
    _run_fused(xb, ld, w, out, M=M)
    close(out[:M, :C], ref)
    check_out(out)
    check_in(xb)


def test_ff_fused_in_place_and_vs_unfused_path(hiplib):
    """out aliasing x (how the engine calls it), and agreement with the three-launch path to f16 rounding."""
    from rcdms_amd import hip
    M, C = 1280, 320
    w, g = _weights(C, 5)
    x = h16(torch.randn(M, C, generator=g))
    dev = _dev(w)
    x16 = gin(x.half())
    fused = gout(M, C)                                    # in place: the rows between NaN guard bands
    fused.copy_(x16)
    _run_fused(fused, C, w, fused)
    check_out(fused)
    # unfused: LayerNorm -> GEGLU GEMM -> out GEMM (+bias +residual)
    a = gout(M, C)
    hip.layernorm(hip.LayerNormDesc(M, C, C, C, 1e-5, 1, 1), x16.data_ptr(), dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), 0,
                  a.data_ptr())
    wp = gout(8 * C, C)
    bp = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    hip.pack_geglu_rows(dev["w1"].data_ptr(), dev["b1"].data_ptr(), 8 * C, C, wp.data_ptr(), bp.data_ptr())
    hid = gout(M, 4 * C)
    wsb = torch.full((1 << 24,), 0xFF, dtype=torch.uint8, device=DEV)   # NaN-filled workspace
    hip.gemm(hip.GemmDesc(M, 8 * C, C, C, 4 * C, 0, hip.EPI_BIAS | hip.EPI_GEGLU, 1, 0, 1.0, 1), a.data_ptr(), wp.data_ptr(),
             bp.data_ptr(), 0, 0, hid.data_ptr(), wsb.data_ptr(), wsb.numel())
    w2h = gw(w["w2"])
    unf = gout(M, C)
    hip.gemm(hip.GemmDesc(M, C, 4 * C, 4 * C, C, C, hip.EPI_BIAS | hip.EPI_RESIDUAL, 1, 0, 1.0, 1), hid.data_ptr(), w2h.data_ptr(),
             dev["b2"].data_ptr(), 0, x16.data_ptr(), unf.data_ptr(), wsb.data_ptr(), wsb.numel())
    torch.cuda.synchronize()
    close(fused, _reference(x, w))
    close(fused, unf.float(), rel=3e-3, abs_frac=3e-3)
    check_all(a, wp, bp, hid, unf, w2h, x16, *dev.values())


def test_ff_fused_deterministic_and_rejects(hiplib):
    from rcdms_amd import hip
    M, C = 640, 320
    w, g = _weights(C, 3)
    x16 = gin(h16(torch.randn(M, C, generator=g)).half())
    a = _run_fused(x16, C, w)
    b = _run_fused(x16, C, w)
    assert torch.equal(a, b)
    check_all(a, b, x16)
    assert not hip.ff_fused_supported(64)
    with pytest.raises(hip.RcdmError):
        hip.ff_fused(hip.FFDesc(M, 64, 64, 64, 1e-5), x16.data_ptr(), x16.data_ptr(), x16.data_ptr(), x16.data_ptr(),
                     x16.data_ptr(), x16.data_ptr(), x16.data_ptr())


# ------------------------------------------------------------------------------------------------
# rcdm_rowchain: tok = a W_a^T + b_a (+ res); y = LayerNorm(tok) (+ pe); tail GEMM (q / qkv) or feed-forward

def _chain_weights(C, tail, frames, seed):
    g = torch.Generator().manual_seed(seed)
    w = dict(wa=h16(torch.randn(C, C, generator=g) * C ** -0.5), ba=0.1 * torch.randn(C, generator=g),
             ln_g=1.0 + 0.2 * torch.randn(C, generator=g), ln_b=0.1 * torch.randn(C, generator=g),
             pe=(0.3 * torch.randn(frames, C, generator=g)) if frames else None)
    if tail:
        w["wt"] = h16(torch.randn(tail * C, C, generator=g) * C ** -0.5)
    else:
        w.update(w1=h16(torch.randn(8 * C, C, generator=g) * C ** -0.5), b1=0.1 * torch.randn(8 * C, generator=g),
                 w2=h16(torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5), b2=0.1 * torch.randn(C, generator=g))
    return w, g


def _chain_reference(a, res, w, tail, rpf):
    C = a.shape[1]
    tok = F.linear(a, w["wa"], w["ba"])
    if res is not None:
        tok = tok + res
    tok = h16(tok)                                         # the token rows are stored (and chained) as f16
    y = F.layer_norm(tok, (C,), w["ln_g"], w["ln_b"], 1e-5)
    if w["pe"] is not None:
        frames = w["pe"].shape[0]
        y = y + w["pe"][(torch.arange(a.shape[0]) // rpf) % frames]
    y = h16(y)
    if tail:
        return tok, F.linear(y, w["wt"])
    hidden, gate = F.linear(y, w["w1"], w["b1"]).chunk(2, dim=-1)
    return tok, tok + F.linear(h16(hidden * F.gelu(gate)), w["w2"], w["b2"])


def _run_chain(a16, res16, w, tail, M, rpf, in_place_tok=False, gn=None):
    from rcdms_amd import hip
    C = w["ln_g"].numel()
    dev = _dev(w)
    ws = gout(1, hip.rowchain_stream_bytes(C, tail), dtype=torch.uint8, guard_rows=1)
    b1p = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    hip.pack_rowchain(dev["wa"].data_ptr(), C, tail, dev["wt"].data_ptr() if tail else 0,
                      0 if tail else dev["w1"].data_ptr(), 0 if tail else dev["b1"].data_ptr(),
                      0 if tail else dev["w2"].data_ptr(), ws.data_ptr(), 0 if tail else b1p.data_ptr())
    ncol = tail * C if tail else C
    tok = res16 if in_place_tok else gout(M, C, C + 8)
    out = gout(M, ncol, ncol + 16)
    frames = w["pe"].shape[0] if w["pe"] is not None else 1
    d = hip.RowChainDesc(M, C, a16.stride(0), res16.stride(0) if res16 is not None else 0, tok.stride(0), out.stride(0), tail,
                         rpf, frames, 1e-5, gn[3] if gn else 0, gn[4] if gn else 0)
    hip.rowchain(d, a16.data_ptr(), res16.data_ptr() if res16 is not None else 0, tok.data_ptr(), dev["ba"].data_ptr(),
                 dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), dev["pe"].data_ptr() if dev["pe"] is not None else 0,
                 ws.data_ptr(), 0 if tail else b1p.data_ptr(), 0 if tail else dev["b2"].data_ptr(), out.data_ptr(),
                 gn_stat=gn[0].data_ptr() if gn else 0, gn_g=gn[1].data_ptr() if gn else 0, gn_b=gn[2].data_ptr() if gn else 0)
    torch.cuda.synchronize()
    check_all(ws, out, a16, *([] if in_place_tok else [tok]), *([res16] if res16 is not None and not in_place_tok else []),
              *(v for v in dev.values() if v is not None))
    return tok, out, ncol


@pytest.mark.parametrize("tail,has_res,frames,M", [
    (3, False, 0, 320),     # proj_in -> norm1 -> qkv (spatial)
    (3, False, 5, 640),     # proj_in -> norms[0] + pe -> qkv (motion; rows_per_frame 64: frames change inside a block)
    (3, True, 5, 333),      # to_out + res -> norms[1] + pe -> qkv, ragged tail
    (1, True, 0, 480),      # attn1.to_out + res -> norm2 -> attn2.to_q
    (0, True, 0, 352),      # attn2.to_out + res -> norm3 -> ff -> + res
    (0, False, 0, 160),
])
def test_rowchain_vs_reference(hiplib, tail, has_res, frames, M):
    _rowchain_vs_reference(tail, has_res, frames, M, 24, 32)


@pytest.mark.parametrize("tail,has_res,frames,M", [(3, True, 5, 333), (1, True, 0, 480), (0, True, 0, 352)])
def test_rowchain_vs_reference_dense_inputs(hiplib, tail, has_res, frames, M):
    _rowchain_vs_reference(tail, has_res, frames, M, 0, 0)


def _rowchain_vs_reference(tail, has_res, frames, M, pad_a, pad_r):
    from rcdms_amd import hip
    C, rpf = 320, 64
    assert hip.rowchain_supported(C)
    w, g = _chain_weights(C, tail, frames, 100 + 7 * tail + M)
    a = h16(torch.randn(M, C, generator=g))
    res = h16(torch.randn(M, C, generator=g) * 1.5) if has_res else None
    tok_ref, out_ref = _chain_reference(a, res, w, tail, rpf)
    a16 = gin(a.half(), C + pad_a)
    res16 = gin(res.half(), C + pad_r) if has_res else None
    tok, out, ncol = _run_chain(a16, res16, w, tail, M, rpf)
    close(tok[:M, :C], tok_ref)
    close(out[:M, :ncol], out_ref)
    check_out(tok)      # token stores outside M x C
    check_out(out)      # tail stores outside the result


def test_rowchain_in_place_token_rows(hiplib):
    """tok aliasing res (how the engine updates the residual stream), feed-forward tail written over tok as well."""
    _rowchain_in_place_token_rows(8, 16)


def test_rowchain_in_place_token_rows_dense(hiplib):
    """... with every row stride equal to C."""
    _rowchain_in_place_token_rows(0, 0)


def _rowchain_in_place_token_rows(pad_a, pad_t):
    M, C = 800, 320
    w, g = _chain_weights(C, 0, 0, 77)
    a = h16(torch.randn(M, C, generator=g))
    res = h16(torch.randn(M, C, generator=g))
    tok_ref, out_ref = _chain_reference(a, res, w, 0, 1)
    from rcdms_amd import hip
    dev = _dev(w)
    ws = gout(1, hip.rowchain_stream_bytes(C, 0), dtype=torch.uint8, guard_rows=1)
    b1p = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    hip.pack_rowchain(dev["wa"].data_ptr(), C, 0, 0, dev["w1"].data_ptr(), dev["b1"].data_ptr(), dev["w2"].data_ptr(),
                      ws.data_ptr(), b1p.data_ptr())
    lda, ldt = C + pad_a, C + pad_t
    tokb = gout(M, C, ldt)                                # in place: the residual stream between NaN pad columns and guard bands
    tokb[:, :C] = res.half().to(DEV)
    a16 = gin(a.half(), lda)
    d = hip.RowChainDesc(M, C, lda, ldt, ldt, ldt, 0, 1, 1, 1e-5)
    hip.rowchain(d, a16.data_ptr(), tokb.data_ptr(), tokb.data_ptr(), dev["ba"].data_ptr(), dev["ln_g"].data_ptr(),
                 dev["ln_b"].data_ptr(), 0, ws.data_ptr(), b1p.data_ptr(), dev["b2"].data_ptr(), tokb.data_ptr())
    torch.cuda.synchronize()
    close(tokb[:, :C], out_ref)
    check_all(tokb, ws, b1p, a16, *(v for v in dev.values() if v is not None))


@pytest.mark.parametrize("frames,rows,samples", [(0, 176, 3), (5, 160, 5), (0, 1024, 2)])
def test_rowchain_groupnorm_prologue(hiplib, frames, rows, samples):
    """GroupNorm -> proj_in -> norm -> qkv with the norm's APPLY inside the chain launch (attention.py:328-330,
    motion_module.py:162-166): against the reference arithmetic, and bit-identical to rcdm_groupnorm_silu followed by the
    chain without the prologue.  rows = 176: blocks of 160 rows meet two samples, also in the middle of the tensor."""
    from rcdms_amd import hip
    C, G, M = 320, 32, rows * samples
    w, g = _chain_weights(C, 3, frames, 900 + rows)
    x = h16(torch.randn(M, C, generator=g) * 2.0 + 0.5)
    gn_g = (1.0 + 0.2 * torch.randn(C, generator=g)).float()
    gn_b = (0.3 * torch.randn(C, generator=g)).float()
    xs = x.view(samples, rows, G, C // G)
    mean = xs.mean(dim=(1, 3), keepdim=True)
    var = xs.var(dim=(1, 3), unbiased=False, keepdim=True)
    a_ref = h16((((xs - mean) / torch.sqrt(var + 1e-6)).reshape(M, C) * gn_g + gn_b))
    tok_ref, out_ref = _chain_reference(a_ref, None, w, 3, rows)

    x16 = gin(x.half())
    gd = hip.GroupNormDesc(samples, rows, C, G, C, C, 1e-6, 0)
    wsb = hip.groupnorm_workspace_bytes(gd)
    gws = torch.full((max(wsb, 16),), 0xFF, dtype=torch.uint8, device=DEV)
    gg, gb = gvec(gn_g), gvec(gn_b)
    # (1) separate launches
    a16 = gout(M, C)
    hip.groupnorm_silu(gd, x16.data_ptr(), gg.data_ptr(), gb.data_ptr(), a16.data_ptr(), gws.data_ptr(), gws.numel())
    tok1, out1, ncol = _run_chain(a16, None, w, 3, M, rows)
    # (2) statistics only + the apply in the chain's prologue
    stat = gout(1, samples * G * 2, dtype=torch.float32, guard_rows=1)
    hip.groupnorm_stats(gd, x16.data_ptr(), stat.data_ptr(), gws.data_ptr(), gws.numel())
    tok2, out2, _ = _run_chain(x16, None, w, 3, M, rows, gn=(stat, gg, gb, G, rows))
    close(tok2[:M, :C], tok_ref)
    close(out2[:M, :ncol], out_ref)
    bad = (tok1[:, :C] != tok2[:, :C]).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"prologue GroupNorm differs from the separate launch in token rows {bad[:8]} ... ({len(bad)} rows)"
    assert torch.equal(out1[:, :ncol], out2[:, :ncol])
    check_all(x16, a16, stat, gg, gb)
    # rejected: with a stage-A residual, or with samples that are not whole 16-row fragments
    d = hip.RowChainDesc(M, C, C, C, C, 3 * C, 3, rows, max(frames, 1), 1e-5, G, rows)
    with pytest.raises(hip.RcdmError):
        hip.rowchain(d, x16.data_ptr(), x16.data_ptr(), tok2.data_ptr(), gg.data_ptr(), gg.data_ptr(), gb.data_ptr(), 0,
                     x16.data_ptr(), 0, 0, out2.data_ptr(), gn_stat=stat.data_ptr(), gn_g=gg.data_ptr(), gn_b=gb.data_ptr())
    d.gn_rows = rows + 8
    with pytest.raises(hip.RcdmError):
        hip.rowchain(d, x16.data_ptr(), 0, tok2.data_ptr(), gg.data_ptr(), gg.data_ptr(), gb.data_ptr(), 0,
                     x16.data_ptr(), 0, 0, out2.data_ptr(), gn_stat=stat.data_ptr(), gn_g=gg.data_ptr(), gn_b=gb.data_ptr())


@pytest.mark.parametrize("M", [352, 2560])
def test_rowchain_ff_then_projection(hiplib, M):
    """tail 2: attn.to_out + res -> norm -> ff -> + res -> proj_out + bias -> + the block's input, one launch
    (attention.py:505-514,352-363).  Against the reference arithmetic and against tail 0 followed by rcdm_gemm."""
    from rcdms_amd import hip
    C = 320
    w, g = _chain_weights(C, 0, 0, 4242 + M)
    wz = h16(torch.randn(C, C, generator=g) * C ** -0.5)
    bz = 0.1 * torch.randn(C, generator=g)
    a = h16(torch.randn(M, C, generator=g))
    res = h16(torch.randn(M, C, generator=g) * 1.5)
    zres = h16(torch.randn(M, C, generator=g))
    tok_ref, ff_ref = _chain_reference(a, res, w, 0, 1)
    out_ref = h16(F.linear(h16(ff_ref), wz, bz)) + zres

    dev = _dev(w)
    wzd, bzd = gin(wz), gvec(bz)
    ws = gout(1, hip.rowchain_stream_bytes(C, 2), dtype=torch.uint8, guard_rows=1)
    assert ws.numel() == 2 * C * C * 14
    b1p = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    hip.pack_rowchain(dev["wa"].data_ptr(), C, 2, wzd.data_ptr(), dev["w1"].data_ptr(), dev["b1"].data_ptr(),
                      dev["w2"].data_ptr(), ws.data_ptr(), b1p.data_ptr())
    lda, ldt, ldz = C + 8, C + 16, C + 24
    a16, z16 = gin(a.half(), lda), gin(zres.half(), ldz)
    tok = gout(M, C, ldt)                            # in place on the residual stream, as the engine runs it
    tok[:, :C] = res.half().to(DEV)
    out = gout(M, C, C + 8)
    d = hip.RowChainDesc(M, C, lda, ldt, ldt, out.stride(0), 2, 1, 1, 1e-5, 0, 0, ldz)
    args = (a16.data_ptr(), tok.data_ptr(), tok.data_ptr(), dev["ba"].data_ptr(), dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), 0,
            ws.data_ptr(), b1p.data_ptr(), dev["b2"].data_ptr(), out.data_ptr())
    hip.rowchain(d, *args, z_res=z16.data_ptr(), z_bias=bzd.data_ptr())
    torch.cuda.synchronize()
    close(tok[:, :C], tok_ref)                       # tok keeps stage A's rows (the feed-forward output is not stored)
    close(out[:M, :C], out_ref)
    check_out(out)                                   # stores outside the result
    check_all(tok, ws, b1p, a16, z16, wzd, bzd, *(v for v in dev.values() if v is not None))
    # the two-launch form: tail 0 in place, then proj_out as rcdm_gemm with bias + residual
    _, ff2, _ = _run_chain(a16, gin(res.half()), w, 0, M, 1)
    out2 = gout(M, C)
    gd = hip.GemmDesc(M, C, C, ff2.stride(0), C, C, 1 | 4, 1, 0, 1.0, 0, 0)
    wsz = torch.full((max(hip.gemm_workspace_bytes(gd), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    wzh = gw(wz)
    gd.ldr = ldz
    hip.gemm(gd, ff2.data_ptr(), wzh.data_ptr(), bzd.data_ptr(), 0, z16.data_ptr(), out2.data_ptr(), wsz.data_ptr(), wsz.numel())
    torch.cuda.synchronize()
    close(out[:M, :C], out2.float().cpu())
    check_all(out2, ff2, wzh, bzd, z16)
    # rejected without the residual / bias of the projection, or without a stage-A residual
    with pytest.raises(hip.RcdmError):
        hip.rowchain(d, *args)
    with pytest.raises(hip.RcdmError):
        hip.rowchain(d, a16.data_ptr(), 0, *args[2:], z_res=z16.data_ptr(), z_bias=bzd.data_ptr())
