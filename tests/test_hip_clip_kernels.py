"""GPU, kernel level: what the CLIP encoders added to librcdm_hip.so — the quick-GELU GEMM epilogue in every tile family
and in the split-K reduce, rcdm_embed_tokens, rcdm_patch_rows, flash attention at head dim 104 — on guarded buffers
(tests/guard.py), against fp32 torch on the same f16-rounded operands.  Tolerance: that of tests/test_hip_kernels.py
(|hip - ref| <= 4e-3 max|ref| + 2e-3 |ref|), exact equality for the two data-movement kernels."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O
from tests.guard import check_all, check_in, check_out, guarded_in, guarded_out
from tests.test_hip_kernels import close, gin, gout, gvec, gw, h16, ws

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("variant", [-1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_gemm_quick_gelu(hiplib, variant):
    """Linear -> x * sigmoid(1.702 x) epilogue: the shapes of test_gemm_gelu (plain, forced split-K 3) plus a forced
    split_k = 2, under the automatic tile choice and every forced tile variant."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(23)
    try:
        hip.set_igemm_variant(variant)
        for M, N, K, split in [(970, 512, 256, 1), (130, 72, 200, 3), (970, 512, 256, 2)]:
            A = h16(torch.randn(M, K, generator=g))
            W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
            bias = torch.randn(N, generator=g)
            v = F.linear(A, W, bias)
            ref = v * torch.sigmoid(1.702 * v)
            Ad, Wd, bd = gin(A.half()), gw(W), gvec(bias)
            out = gout(M, N)
            dsc = hip.GemmDesc(M, N, K, K, N, 0, hip.EPI_BIAS | hip.EPI_QUICK_GELU, 1, 0, 1.0, split)
            w = ws(hip.gemm_workspace_bytes(dsc))
            hip.gemm(dsc, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
            torch.cuda.synchronize()
            close(out, ref)
            check_all(out, Ad, Wd, bd)
    finally:
        hip.set_igemm_variant(-1)


def test_gemm_quick_gelu_with_residual(hiplib):
    """out = quick_gelu(acc + bias) + residual: the activation comes before the residual add."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(29)
    M, N, K = 300, 320, 320
    A = h16(torch.randn(M, K, generator=g))
    W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    bias, res = torch.randn(N, generator=g), h16(torch.randn(M, N, generator=g))
    v = F.linear(A, W, bias)
    ref = v * torch.sigmoid(1.702 * v) + res
    Ad, Wd, bd, Rd = gin(A.half(), K + 8), gw(W), gvec(bias), gin(res.half(), N + 8)
    out = gout(M, N, N + 16)
    dsc = hip.GemmDesc(M, N, K, K + 8, N + 16, N + 8, hip.EPI_BIAS | hip.EPI_QUICK_GELU | hip.EPI_RESIDUAL, 1, 0, 1.0, 1)
    hip.gemm(dsc, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, Rd.data_ptr(), out.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    close(out[:, :N], ref)
    check_all(out, Ad, Wd, bd, Rd)


def test_quick_gelu_flag_rules(hiplib):
    """QUICK_GELU | GELU (or GEGLU) is RCDM_EINVAL; the fused-norm GEMM forms refuse the flag with RCDM_ESHAPE."""
    from rcdms_amd import hip
    x = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    f = torch.zeros(1 << 12, dtype=torch.float32, device=DEV)
    p, fp = x.data_ptr(), f.data_ptr()
    for other in (hip.EPI_GELU, hip.EPI_GEGLU):
        d = hip.GemmDesc(64, 64, 64, 64, 64, 0, hip.EPI_QUICK_GELU | other, 1, 0, 1.0, 1)
        assert hiplib.rcdm_gemm(ctypes.byref(d), p, p, 0, 0, 0, p, 0, 0, 0) == -1
    d = hip.GemmDesc(64, 64, 64, 64, 64, 0, hip.EPI_QUICK_GELU, 1, 0, 1.0, 1)
    ln = hip.LnFuse(fp, fp, 0, p, 64, 1, 1, 1e-5)
    assert hiplib.rcdm_gemm_ln(ctypes.byref(d), ctypes.byref(ln), p, p, 0, 0, p, 0) == -2
    lx = hip.Lnx(0, 0, 0, 0, 0, 0, 0, 1e-5, 64)
    assert hiplib.rcdm_gemm_lnx(ctypes.byref(d), ctypes.byref(lx), p, p, 0, 0, 0, p, 0, 0, 0) == -2
    c = hip.ConvDesc(1, 8, 8, 64, 64, 1, 0, 64, 64, 0, hip.EPI_QUICK_GELU, 1, 0, 1.0, 1, 0, 0, 0, 0)
    assert hiplib.rcdm_conv3x3(ctypes.byref(c), p, p, 0, 0, 0, p, 0, 0, 0) == -2


def test_embed_tokens(hiplib):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(31)
    B, L, C, vocab = 3, 85, 768, 512
    ldo = C + 8
    table, pos = torch.randn(vocab, C, generator=g), torch.randn(L, C, generator=g)
    ids = torch.randint(0, vocab, (B, L), generator=g)
    ids[0, 0], ids[1, 7], ids[2, L - 1] = 0, vocab - 1, vocab - 1
    ref = (table[ids] + pos[None]).half().reshape(B * L, C)
    td, pd = gin(table), gin(pos)
    idd = ids.reshape(-1).to(torch.int32).to(DEV)
    out = gout(B * L, C, ldo)
    hip.embed_tokens(idd.data_ptr(), B * L, L, td.data_ptr(), vocab, pd.data_ptr(), C, out.data_ptr(), ldo)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :C].cpu(), ref)
    check_out(out)
    check_in(td)
    check_in(pd)
    assert hiplib.rcdm_embed_tokens(idd.data_ptr(), B * L, L, td.data_ptr(), vocab, pd.data_ptr(), C + 4, out.data_ptr(), ldo, 0) == -2


def test_patch_rows(hiplib):
    from rcdms_amd import hip
    B, S, patch, ldk = 2, 56, 14, 592
    K, P = 3 * patch * patch, (S // patch) ** 2
    pix = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(37))
    pd = gin(pix.reshape(B * 3 * S, S))
    out = gout(B * (P + 1), ldk)
    hip.patch_rows(pd.data_ptr(), B, S, S, patch, out.data_ptr(), ldk)
    torch.cuda.synchronize()
    got = out.cpu().reshape(B, P + 1, ldk)
    ref = F.unfold(pix, patch, stride=patch).transpose(1, 2).half()      # (B, P, 588), columns in (c, ky, kx) order
    assert torch.equal(got[:, 1:, :K], ref)
    assert (got[:, 0] == 0).all(), "class-token rows must be zero"
    assert (got[:, :, K:] == 0).all(), "pad columns must be zero"
    check_out(out)
    check_in(pd)
    assert hiplib.rcdm_patch_rows(pd.data_ptr(), B, 60, S, patch, out.data_ptr(), ldk, 0) == -2
    assert hiplib.rcdm_patch_rows(pd.data_ptr(), B, S, S, patch, out.data_ptr(), 584, 0) == -2


@pytest.mark.parametrize("batch,heads,Lq,Lk", [
    (2, 2, 257, 257),    # a 224^2 image: four 64-key tiles + a one-key tail, three query blocks
    (2, 2, 17, 17),      # a 56^2 image: one ragged tile
    (2, 2, 257, 64),     # exactly one full key tile
])
def test_flash_attn_d104(hiplib, batch, heads, Lq, Lk):
    """Head dim 104 (the CLIP-bigG vision tower), whichever instantiation the library dispatches it to."""
    from rcdms_amd import hip
    d = 104
    g = torch.Generator().manual_seed(3 + Lq + Lk + d)
    C = heads * d
    q = h16(torch.randn(batch, Lq, C, generator=g))
    k = h16(torch.randn(batch, Lk, C, generator=g))
    v = h16(torch.randn(batch, Lk, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    qd = gin(q.reshape(-1, C).half(), 3 * C)
    kv = gin(torch.cat([k.reshape(-1, C), v.reshape(-1, C)], dim=1).half())
    out = gout(batch * Lq, C)
    desc = hip.AttnDesc(batch, heads, Lq, Lk, d, 3 * C, 2 * C, 2 * C, C, d ** -0.5)
    hip.flash_attn(desc, qd.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, out.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(batch, Lq, C), ref)
    check_all(out, qd, kv)


def test_flash_attn_masked_causal_d104(hiplib):
    from rcdms_amd import hip
    batch, heads, L, d = 2, 2, 85, 104
    g = torch.Generator().manual_seed(5 + L + d)
    C = heads * d
    q, k, v = (h16(torch.randn(batch, L, C, generator=g)) for _ in range(3))
    add = torch.full((L, L), -10000.0).triu_(1)[None].expand(batch, L, L)
    ref = O.attention_core(q, k, v, heads, mask=add)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    out = gout(batch * L, C)
    desc = hip.AttnDesc(batch, heads, L, L, d, C, C, C, C, d ** -0.5)
    hip.flash_attn_masked(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), 0, True, out.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(batch, L, C), ref)
    check_all(out, qd, kd, vd)
