"""GPU parity tests, kernel level: every C-ABI entry point of librcdm_hip.so against the oracle's op
(oracle/unet_oracle.py, CPU fp32) on the same seeded inputs.  Inputs are rounded to f16 first so the
only differences are accumulation order and the single output rounding.

Tolerance (stated once): outputs are f16 -> relative 2^-10 per rounding; we accept
|hip - oracle| <= 4e-3 * max|oracle| + 2e-3 * |oracle| elementwise unless a test says otherwise."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O
from tests.guard import check_all, check_out, check_written, guarded_in, guarded_out, guarded_vec, guarded_w

pytestmark = pytest.mark.gpu

DEV = "cuda"


def close(got, ref, rel=2e-3, abs_frac=4e-3):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite output"
    tol = abs_frac * ref.abs().max() + rel * ref.abs()
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), f"max err {err.max():.4g} (ref max {ref.abs().max():.4g}), {int(bad.sum())} / {bad.numel()} outside tol"


def h16(x):
    return x.half().float()


def gin(t, ld=None, guard_rows=256):
    """A read-only 2-D operand inside poison (tests/guard.py): pad columns and guard rows above and below."""
    return guarded_in(t, ld, device=DEV, guard_rows=guard_rows)[0]


def gout(rows, C, ld=None, dtype=torch.float16, guard_rows=256):
    """A NaN-filled output with pad columns and guard rows above and below."""
    return guarded_out(rows, C, ld, dtype, device=DEV, guard_rows=guard_rows)[0]


def gvec(v):
    """A dense fp32 vector / table operand at a 16-byte-aligned offset inside poison."""
    return guarded_vec(v.float(), device=DEV)[0]


def gw(W):
    """A dense f16 weight matrix W[N][K] with poisoned guard rows around it."""
    return guarded_w(W.half(), device=DEV)[0]


def rows_from_5d(x5, ld=None, dev=DEV):
    """(b,C,f,H,W) fp32 -> f16 rows [b*f*H*W][ld] on the GPU, the pad columns and guard rows around them poisoned."""
    b, c, f, h, w = x5.shape
    r = x5.permute(0, 2, 3, 4, 1).reshape(b * f * h * w, c).half()
    return guarded_in(r, ld or c, device=dev)[0]


def rows_to_5d(rows, b, c, f, h, w):
    return rows[:, :c].float().cpu().reshape(b, f, h, w, c).permute(0, 4, 1, 2, 3)


def ws(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)   # NaN-filled: no kernel may depend on workspace contents


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,epi,split", [
    (256, 128, 64, 0, 1),
    (300, 320, 320, 1 | 4, 1),       # M tail, N tail, bias + residual
    (300, 320, 320, 1 | 2, 1),       # bias + per-sample row vector
    (640, 1280, 1280, 1, 0),         # heuristic split-K
    (130, 72, 200, 1 | 4, 3),        # forced split-K, K tail (200 = 3*64 + 8), N % 128 != 0
    (1024, 960, 320, 0, 1),
    (260, 64, 64, 1 | 2 | 4, 1),     # row vector with fewer rows per sample (100) than a 128-row tile: in-place reads
    (400, 320, 128, 1 | 2 | 4, 1),
])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_gemm(hiplib, M, N, K, epi, split, variant):
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(1234 + M + N + K)
    A = h16(torch.randn(M, K, generator=g))
    W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    rps = 150 if M == 300 else 100   # 150: a 128-row tile straddles two samples (the two-vector prefetch path)
    nsamp = (M + rps - 1) // rps
    rowvec = torch.randn(nsamp, N, generator=g)
    res = h16(torch.randn(M, N, generator=g))
    ref = A @ W.t()
    if epi & 1:
        ref = ref + bias
    if epi & 2:
        ref = ref + rowvec[torch.arange(M) // rps]
    if epi & 4:
        ref = ref + res
    lda, ldc, ldr, ldt = K + 8, N + 16, N + 8, N + 8
    Ad, Rd = gin(A.half(), lda), gin(res.half(), ldr)
    Wd, bd, rvd = gw(W), gvec(bias), gin(rowvec, ldt, guard_rows=8)
    out = gout(M, N, ldc)
    d = hip.GemmDesc(M, N, K, lda, ldc, ldr, epi, rps, ldt, 1.0, split)
    w = ws(hip.gemm_workspace_bytes(d))
    hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), rvd.data_ptr(), Rd.data_ptr(), out.data_ptr(),
             w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    hip.set_igemm_variant(-1)
    close(out[:, :N], ref)
    assert torch.isnan(out[:, N:].float()).all(), "wrote outside the N columns"
    check_all(out, Ad, Rd, Wd, bd, rvd)


def test_gemm_transpose_detecting(hiplib):
    """A = I (padded) with an ASYMMETRIC W catches a row/col swap in the MFMA C layout."""
    from rcdms_amd import hip
    M = N = K = 128
    A = torch.eye(M, K)
    W = (torch.arange(N)[:, None] * 0.01 + torch.arange(K)[None, :] * 0.37) % 3.0
    W = h16(W)
    out = gout(M, N)
    d = hip.GemmDesc(M, N, K, K, N, N, 0, 1, 0, 1.0, 1)
    Ad, Wd = gin(A.half()), gw(W)
    hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), 0, 0, 0, out.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    close(out, W.t(), rel=1e-3, abs_frac=1e-3)
    check_all(out, Ad, Wd)


@pytest.mark.parametrize("variant", [6, 7, 8, 9])
@pytest.mark.parametrize("M,N,K,epi,split", [
    (700, 648, 1000, 1 | 4, 1),      # several tiles both ways, ragged M / N, K tail (15 k-steps + 40), bias + residual
    (1280, 640, 704, 1, 0),          # 11 k-steps (odd), heuristic split
    (512, 512, 64, 0, 1),            # a single k-step: prologue -> epilogue with no steady-state tick
    (512, 512, 128, 1 | 16, 1),      # two k-steps, GELU epilogue
    (2560, 1280, 2560, 1 | 4, 0),    # M = 2560 level: fewer tiles than CUs -> split-K slabs + reduce
    (330, 330 // 8 * 8, 1920, 1 | 2, 1),
])
def test_gemm_pingpong(hiplib, M, N, K, epi, split, variant):
    """The 8-wave ping-pong kernel (igemm8.hip) at shapes that exercise its slot-release schedule: odd / even / tiny
    k-step counts, tiles ragged in M and N, the fused and the split-K (slab) epilogues."""
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(4321 + M + N + K)
    A = h16(torch.randn(M, K, generator=g))
    W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    rps = 150
    rowvec = torch.randn((M + rps - 1) // rps, N, generator=g)
    res = h16(torch.randn(M, N, generator=g))
    ref = A @ W.t()
    if epi & 1:
        ref = ref + bias
    if epi & 2:
        ref = ref + rowvec[torch.arange(M) // rps]
    if epi & 16:
        ref = F.gelu(ref)
    if epi & 4:
        ref = ref + res
    Ad, Wd, Rd = gin(A.half()), gw(W), gin(res.half())
    bd, rvd = gvec(bias), gvec(rowvec)
    out = gout(M, N, N + 8)
    d = hip.GemmDesc(M, N, K, K, N + 8, N, epi, rps, N, 1.0, split)
    w = ws(hip.gemm_workspace_bytes(d))
    for _ in range(2):   # twice: a stale-LDS or missed-wait race rarely shows on a cold first launch only
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), rvd.data_ptr(), Rd.data_ptr(), out.data_ptr(),
                 w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    hip.set_igemm_variant(-1)
    close(out[:, :N], ref)
    assert torch.isnan(out[:, N:].float()).all(), "wrote outside the N columns"
    check_all(out, Ad, Wd, Rd, bd, rvd)


@pytest.mark.parametrize("M,N,K,epi,pe,dup", [
    (40960, 320, 320, 1 | 4, False, 0),     # to_out + residual -> norm2 / norm3 at the 64x64 level
    (20480, 320, 320, 1, True, 20480),      # proj_in -> temporal norm with the positional encoding; shared-prefix dup
    (4100, 320, 1280, 1 | 4, False, 0),     # ragged last tile, long K
    (330, 64, 64, 1 | 4, True, 0),          # tiny-config width: masked chunks in every row group
    (97, 200, 72, 0, False, 0),             # no bias, no residual, 25 chunks per row
])
def test_gemm_ln(hiplib, M, N, K, epi, pe, dup):
    """rcdm_gemm_ln (the LayerNorm of the output rows fused into the 160x320 ping-pong tile's epilogue) against the fp32
    reference, and bit for bit against the two calls it replaces: the same kernel without the LayerNorm + rcdm_layernorm."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(77 + M + N + K)
    A = h16(torch.randn(M, K, generator=g))
    W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    res = h16(torch.randn(M, N, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(N, generator=g), torch.randn(N, generator=g)
    frames, rpf = 5, 64
    table = O.sinusoid_table(N, frames)
    x_ref = A @ W.t()
    if epi & 1:
        x_ref = x_ref + bias
    if epi & 4:
        x_ref = x_ref + res
    y_ref = F.layer_norm(h16(x_ref), (N,), gamma, beta, 1e-5)
    if pe:
        y_ref = y_ref + table[(torch.arange(M) // rpf) % frames]
    Ad, Wd, Rd = gin(A.half()), gw(W), gin(res.half())
    bd, gd, btd, td = gvec(bias), gvec(gamma), gvec(beta), gvec(table)
    rows = M + (dup if dup else 0)
    out = gout(rows, N, N + 8)
    y = gout(M, N, N + 8)
    d = hip.GemmDesc(M, N, K, K, N + 8, N, epi, 1, 0, 1.0, 1, dup)
    ln = hip.LnFuse(gd.data_ptr(), btd.data_ptr(), td.data_ptr() if pe else 0, y.data_ptr(), N + 8, rpf, frames, 1e-5)
    for _ in range(2):
        hip.gemm_ln(d, ln, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), Rd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    close(out[:M, :N], x_ref)
    close(y[:, :N], y_ref)
    assert torch.isnan(out[:, N:].float()).all() and torch.isnan(y[:, N:].float()).all(), "wrote outside the N columns"
    if dup:
        assert torch.equal(out[dup:dup + M, :N], out[:M, :N])
    check_all(out, y, Ad, Wd, Rd, bd, gd, btd, td)
    # the unfused pair: same GEMM kernel (variant 6 = the 160x320 ping-pong tile), then rcdm_layernorm on its output
    hip.set_igemm_variant(6)
    out2 = gout(M, N)
    y2 = gout(M, N)
    d2 = hip.GemmDesc(M, N, K, K, N, N, epi, 1, 0, 1.0, 1, 0)
    w = ws(hip.gemm_workspace_bytes(d2))
    hip.gemm(d2, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, Rd.data_ptr(), out2.data_ptr(), w.data_ptr(), w.numel())
    hip.set_igemm_variant(-1)
    hip.layernorm(hip.LayerNormDesc(M, N, N, N, 1e-5, rpf, frames), out2.data_ptr(), gd.data_ptr(), btd.data_ptr(),
                  td.data_ptr() if pe else 0, y2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out[:M, :N], out2), "fused GEMM output differs from the unfused kernel's"
    dy = (y[:, :N].float() - y2.float()).abs().max().item()
    assert dy <= 2e-3 * y_ref.abs().max().item(), dy          # same inputs, another summation order in the row statistics
    check_all(out2, y2, Ad, Wd, Rd, bd, gd, btd, td)


def test_gemm_ln_rejects(hiplib):
    from rcdms_amd import hip
    x = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    f = torch.zeros(1 << 12, dtype=torch.float32, device=DEV)
    ln = hip.LnFuse(f.data_ptr(), f.data_ptr(), 0, x.data_ptr(), 640, 1, 1, 1e-5)
    for desc in (hip.GemmDesc(64, 640, 64, 64, 640, 640, 1, 1, 0, 1.0, 1, 0),        # row wider than one tile
                 hip.GemmDesc(64, 320, 64, 64, 160, 160, 1 | 8, 1, 0, 1.0, 1, 0),    # GEGLU
                 hip.GemmDesc(64, 320, 64, 64, 320, 320, 1, 1, 0, 1.0, 2, 0)):       # split-K
        with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
            hip.gemm_ln(desc, ln, x.data_ptr(), x.data_ptr(), f.data_ptr(), 0, x.data_ptr())


@pytest.mark.parametrize("variant", [1, 2, 5, 6, 8, 9])
@pytest.mark.parametrize("split", [1, 2])
def test_gemm_dup_rows(hiplib, variant, split):
    """rcdm_gemm_desc.dup_rows: every output row is also stored dup_rows further down (shared CFG prefix)."""
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(5)
    M, N, K = 300, 320, 256
    A = h16(torch.randn(M, K, generator=g)); W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    Ad, Wd, bd = gin(A.half()), gw(W), gvec(bias)
    out = gout(2 * M + 3, N)
    d = hip.GemmDesc(M, N, K, K, N, 0, 1, 1, 0, 1.0, split, M + 3)
    w = ws(hip.gemm_workspace_bytes(d))
    hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    hip.set_igemm_variant(-1)
    close(out[:M], A @ W.t() + bias)
    assert torch.equal(out[:M], out[M + 3:]) and torch.isnan(out[M:M + 3].float()).all()
    check_all(out, Ad, Wd, bd)


@pytest.mark.parametrize("variant", [6, 7, 8])
def test_gemm_pingpong_bitwise_vs_128(hiplib, variant):
    """Same k order inside a tile -> the ping-pong kernel and the 128x128 kernel agree BIT FOR BIT without split-K
    (fp32 accumulation over k in the same 32-deep MFMA steps? no: 16x16x32 vs 32x32x16 group k differently, so only
    near-equality is required) — and repeated launches of the ping-pong kernel are bit-identical (no race)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(77)
    M, N, K = 1600, 960, 1280
    Ad = gin(h16(torch.randn(M, K, generator=g)).half())
    Wd = gw(h16(torch.randn(N, K, generator=g) * K ** -0.5))
    d = hip.GemmDesc(M, N, K, K, N, 0, 0, 1, 0, 1.0, 1)
    outs = []
    for v in (variant, variant, variant, 1):
        hip.set_igemm_variant(v)
        o = gout(M, N)
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), 0, 0, 0, o.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        outs.append(o)
    hip.set_igemm_variant(-1)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "ping-pong kernel is not deterministic"
    close(outs[0], outs[3].float(), rel=2e-3, abs_frac=1e-3)
    check_all(*outs, Ad, Wd)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
@pytest.mark.parametrize("split", [1, 2])
def test_gemm_geglu(hiplib, split, variant):
    _gemm_geglu(split, variant, 8)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
@pytest.mark.parametrize("split", [1, 2])
def test_gemm_geglu_dense(hiplib, split, variant):
    _gemm_geglu(split, variant, 0)


def _gemm_geglu(split, variant, pad):
    """pad: lda = K + pad, ldc = N / 2 + pad (the GEGLU output is half as wide as the GEMM)."""
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(7)
    M, C = 200, 64
    x = h16(torch.randn(M, C, generator=g))
    sd = {"ff.net.0.proj.weight": h16(torch.randn(8 * C, C, generator=g) * C ** -0.5),
          "ff.net.0.proj.bias": torch.randn(8 * C, generator=g) * 0.1}
    hg = F.linear(x, sd["ff.net.0.proj.weight"], sd["ff.net.0.proj.bias"])
    hidden, gate = hg.chunk(2, dim=-1)
    ref = hidden * F.gelu(gate)
    wp = gout(8 * C, C)
    bp = gout(1, 8 * C, dtype=torch.float32, guard_rows=1)
    w32, b32, xd = gin(sd["ff.net.0.proj.weight"]), gvec(sd["ff.net.0.proj.bias"]), gin(x.half(), C + pad)
    hip.pack_geglu_rows(w32.data_ptr(), b32.data_ptr(), 8 * C, C, wp.data_ptr(), bp.data_ptr())
    out = gout(M, 4 * C, 4 * C + pad)
    d = hip.GemmDesc(M, 8 * C, C, C + pad, 4 * C + pad, 0, hip.EPI_BIAS | hip.EPI_GEGLU, 1, 0, 1.0, split)
    w = ws(hip.gemm_workspace_bytes(d))
    hip.gemm(d, xd.data_ptr(), wp.data_ptr(), bp.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    hip.set_igemm_variant(-1)
    close(out[:, :4 * C], ref)
    check_all(out, wp, bp, w32, b32, xd)


@pytest.mark.parametrize("b,f,H,W,cin,cout,stride,up,split", [
    (1, 2, 8, 8, 64, 128, 1, 0, 1),
    (2, 3, 10, 6, 72, 72, 1, 0, 1),     # ragged: c_in tail, N tail, M tail
    (1, 5, 16, 16, 64, 64, 2, 0, 1),    # Downsample3D
    (1, 5, 8, 8, 128, 64, 1, 1, 1),     # Upsample3D folded into the conv
    (2, 1, 8, 8, 320, 320, 1, 0, 4),    # split-K
    (2, 5, 16, 16, 128, 320, 1, 0, 0),  # 2560 pixels: several 160-row tiles, 18 k-steps, heuristic split
])
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_conv3x3(hiplib, b, f, H, W, cin, cout, stride, up, split, variant):
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(99 + cin + cout + stride + up)
    x = h16(torch.randn(b, cin, f, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=g)
    temb = torch.randn(b, cout, generator=g)
    xin = F.interpolate(x, scale_factor=[1.0, 2.0, 2.0], mode="nearest") if up else x
    ref = O.conv_frames(xin, w, bias, stride=stride, padding=1) + temb[:, :, None, None, None]
    Ho, Wo = ref.shape[-2:]
    res = h16(torch.randn(ref.shape, generator=g))
    ref = ref + res
    lda = cin + 8
    xd = rows_from_5d(x, lda)
    rd = rows_from_5d(res)
    wp = gout(cout, 9 * cin)
    w32 = gvec(w)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    out = gout(b * f * Ho * Wo, cout)
    d = hip.ConvDesc(b * f, H, W, cin, cout, stride, up, lda, cout, cout,
                     hip.EPI_BIAS | hip.EPI_ROWVEC | hip.EPI_RESIDUAL, f * Ho * Wo, cout, 1.0, split)
    wsb = ws(hip.conv3x3_workspace_bytes(d))
    bd, td = gvec(bias), gvec(temb)
    hip.conv3x3(d, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(),
                wsb.data_ptr(), wsb.numel())
    torch.cuda.synchronize()
    hip.set_igemm_variant(-1)
    close(rows_to_5d(out, b, cout, f, Ho, Wo), ref)
    check_all(out, wp, xd, rd, w32, bd, td)


@pytest.mark.parametrize("b,f,H,W,cin,cin2,cout,split", [
    (1, 2, 8, 8, 64, 128, 64, 1),        # the second input deeper than one tap
    (2, 3, 10, 6, 128, 64, 72, 1),       # M tail, N tail, a padded second-input row stride
    (2, 1, 8, 8, 320, 640, 320, 4),      # split-K: the second input's k-steps sit in the last slab
    (2, 5, 16, 16, 128, 192, 320, 0),    # 2560 pixels: several tiles, heuristic split
    (2, 5, 8, 8, 1280, 2560, 1280, 0),   # the 8x8-level up-block ResNet (conv2 + shortcut of the 2560-channel concat)
])
@pytest.mark.parametrize("variant", [-1, 1, 3, 5, 6, 7, 8, 9])
def test_conv3x3_add1x1(hiplib, b, f, H, W, cin, cin2, cout, split, variant):
    """rcdm_conv3x3_add1x1: conv3x3(x) + conv1x1(x2) in one implicit GEMM (ResnetBlock3D conv2 + conv_shortcut,
    resnet.py:205-212) against the two fp32 convolutions, on every tile family, with split-K and the fused epilogue."""
    from rcdms_amd import hip
    if variant == -1 and cin < 1280:
        pytest.skip("heuristic pick: production shape only")
    if variant != -1 and cin >= 1280 and variant not in (1, 8, 9):
        pytest.skip("production shape: its own tile families only")
    g = torch.Generator().manual_seed(77 + cin + cin2 + cout)
    x = h16(torch.randn(b, cin, f, H, W, generator=g))
    x2 = h16(torch.randn(b, cin2, f, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    w2 = h16(torch.randn(cout, cin2, generator=g) * cin2 ** -0.5)
    bias = torch.randn(cout, generator=g)
    temb = torch.randn(b, cout, generator=g)
    res = h16(torch.randn(b, cout, f, H, W, generator=g))
    ref = (O.conv_frames(x, w, bias, stride=1, padding=1) + torch.einsum("oc,bcfhw->bofhw", w2, x2)
           + temb[:, :, None, None, None] + res) * 0.5
    lda, lda2 = cin + 8, cin2 + 16
    xd, x2d, rd = rows_from_5d(x, lda), rows_from_5d(x2, lda2), rows_from_5d(res)
    wp = gout(cout, 9 * cin)
    w32 = gvec(w)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    wk = gw(torch.cat([wp, w2.half().to(DEV)], dim=1))
    out = gout(b * f * H * W, cout)
    d = hip.ConvDesc(b * f, H, W, cin, cout, 1, 0, lda, cout, cout, hip.EPI_BIAS | hip.EPI_ROWVEC | hip.EPI_RESIDUAL,
                     f * H * W, cout, 0.5, split, 0, 0, cin2, lda2)
    bd, td = gvec(bias), gvec(temb)
    hip.set_igemm_variant(variant)
    try:
        wsb = ws(hip.conv3x3_workspace_bytes(d))
        hip.conv3x3_add1x1(d, xd.data_ptr(), x2d.data_ptr(), wk.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(),
                           out.data_ptr(), wsb.data_ptr(), wsb.numel())
        torch.cuda.synchronize()
        # the plain entry point refuses a descriptor that names a second input (it has no pointer for it)
        with pytest.raises(hip.RcdmError):
            hip.conv3x3(d, xd.data_ptr(), wk.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(),
                        wsb.data_ptr(), wsb.numel())
    finally:
        hip.set_igemm_variant(-1)
    close(rows_to_5d(out, b, cout, f, H, W), ref)
    check_all(out, wp, xd, x2d, rd, wk, w32, bd, td)


def test_conv3x3_add1x1_refusals(hiplib):
    """The second input needs stride 1, no upsample, whole 64-channel k-steps on both inputs and a pointer."""
    from rcdms_amd import hip
    x = torch.zeros(64, dtype=torch.float16, device=DEV)
    p = x.data_ptr()
    for bad in (hip.ConvDesc(2, 8, 8, 64, 64, 2, 0, 64, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 64, 64),      # stride 2
                hip.ConvDesc(2, 8, 8, 64, 64, 1, 1, 64, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 64, 64),      # upsample
                hip.ConvDesc(2, 8, 8, 72, 64, 1, 0, 72, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 64, 64),      # c_in % 64
                hip.ConvDesc(2, 8, 8, 64, 64, 1, 0, 64, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 72, 72),      # c_in2 % 64
                hip.ConvDesc(2, 8, 8, 64, 64, 1, 0, 64, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 64, 32)):     # lda2 < c_in2
        with pytest.raises(hip.RcdmError):
            hip.conv3x3_add1x1(bad, p, p, p, 0, 0, 0, p, 0, 0)
    ok = hip.ConvDesc(2, 8, 8, 64, 64, 1, 0, 64, 64, 0, 0, 1, 0, 1.0, 0, 0, 0, 64, 64)
    with pytest.raises(hip.RcdmError):
        hip.conv3x3_add1x1(ok, p, 0, p, 0, 0, 0, p, 0, 0)     # no second input


@pytest.mark.parametrize("n_img,H,W,cin,cout,variant,split", [
    (5, 16, 16, 64, 96, 6, 0),       # 1280 source pixels = 8 tiles of 160 rows per phase; N tail (96 of a 320-wide tile)
    (5, 16, 16, 128, 256, 7, 0),     # 160x256 tiles
    (5, 16, 16, 64, 520, 8, 0),      # 256x256 tiles, three column tiles, the last one 8 columns wide
    (10, 8, 8, 192, 64, 6, 0),       # 8x8 images: 2.5 images per 160-row tile (image borders inside a tile)
    (10, 8, 8, 192, 64, 6, 3),       # ... split-K: fp32 slabs + the reduce pass store the remapped rows
    (10, 16, 16, 1280, 1280, -1, 0), # the 16x16 -> 32x32 upsampler of the UNet, heuristic tile
    (10, 8, 8, 1280, 1280, -1, 0),   # the 8x8 -> 16x16 upsampler: 64 tiles, heuristic split-K
])
def test_conv3x3_upsample_phase_form(hiplib, n_img, H, W, cin, cout, variant, split):
    """rcdm_conv3x3 with upsample = 2 (four 2x2 phase convolutions over the source grid, weights from
    rcdm_pack_conv3x3_up2) against nearest-2x upsample + conv3x3 in fp32 (resnet.py:60-79), and against the library's own
    upsample = 1 form on the same operands."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(500 + cin + cout + H)
    x = h16(torch.randn(1, cin, n_img, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=g)
    ref = O.conv_frames(F.interpolate(x, scale_factor=[1.0, 2.0, 2.0], mode="nearest"), w, bias, stride=1, padding=1)
    lda = cin + 8
    xd = rows_from_5d(x, lda)
    w32, bd = gvec(w), gvec(bias)
    wp2_h = gout(4 * cout, 4 * cin)
    wp2 = wp2_h.view(4, cout, 4 * cin)
    hip.pack_conv3x3_up2(w32.data_ptr(), cout, cin, wp2.data_ptr())
    # the packed image against the definition: phase (a, b), source tap (r, c) = sum of the 3x3 taps that land on it
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    for a in (0, 1):
        for b in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    want = w[:, :, rows[a][r]][:, :, :, rows[b][c]].sum(dim=(2, 3))
                    got = wp2[2 * a + b].view(cout, 4, cin)[:, 2 * r + c].float().cpu()
                    assert (got - want).abs().max() <= 1e-3 * want.abs().max() + 1e-6
    out = gout(n_img * 4 * H * W, cout)
    d2 = hip.ConvDesc(n_img, H, W, cin, cout, 1, 2, lda, cout, 0, hip.EPI_BIAS, 1, 0, 1.0, split)
    hip.set_igemm_variant(variant)
    try:
        assert hip.conv3x3_up2_supported(d2)
        w2 = ws(hip.conv3x3_workspace_bytes(d2))
        assert (hip.conv3x3_workspace_bytes(d2) > 0) == (split > 1 or (n_img, H, cin) == (10, 8, 1280))
        hip.conv3x3(d2, xd.data_ptr(), wp2.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w2.data_ptr(), w2.numel())
        torch.cuda.synchronize()
    finally:
        hip.set_igemm_variant(-1)
    close(rows_to_5d(out, 1, cout, n_img, 2 * H, 2 * W), ref)
    wp = gout(cout, 9 * cin)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    out1 = gout(n_img * 4 * H * W, cout)
    d1 = hip.ConvDesc(n_img, H, W, cin, cout, 1, 1, lda, cout, 0, hip.EPI_BIAS, 1, 0, 1.0, 0)
    wsb = ws(hip.conv3x3_workspace_bytes(d1))
    hip.conv3x3(d1, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), 0, 0, out1.data_ptr(), wsb.data_ptr(), wsb.numel())
    torch.cuda.synchronize()
    diff = (out.float() - out1.float()).abs().max().item()
    assert diff <= 4e-3 * ref.abs().max().item(), diff
    check_all(out, out1, wp, xd, w32, bd)
    check_out(wp2_h)


def test_shape_rules_override_the_tile_choice(hiplib):
    """rcdm_set_shape_rules: a rule changes the tile variant / split-K plan of exactly its shape (seen through the workspace
    query), the result stays right, "off" and NULL restore the library's own behaviour, malformed text is ignored."""
    from rcdms_amd import hip
    M, N, K = 640, 1280, 1280
    g = torch.Generator().manual_seed(3)
    A = h16(torch.randn(M, K, generator=g))
    W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
    ref = A @ W.t()
    Ad, Wd = gin(A.half()), gw(W)
    d = hip.GemmDesc(M, N, K, K, N, 0, 0, 1, 0, 1.0, 0)
    other = hip.GemmDesc(M, N, 4096, 4096, N, 0, 0, 1, 0, 1.0, 0)   # (a shape the library's own table has no rule for)

    def run():
        w = ws(hip.gemm_workspace_bytes(d))
        out = gout(M, N)
        hip.gemm(d, Ad.data_ptr(), Wd.data_ptr(), 0, 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
        close(out, ref)
        check_all(out, Ad, Wd)
    try:
        hip.set_shape_rules("off")
        base, base_other = hip.gemm_workspace_bytes(d), hip.gemm_workspace_bytes(other)
        run()
        hip.set_shape_rules(f"1,{M},{N},{K},3,4")          # 64x64 tiles, K cut four ways: four fp32 slabs
        assert hip.gemm_workspace_bytes(d) == 4 * M * N * 4
        assert hip.gemm_workspace_bytes(other) == base_other   # another shape is not touched
        run()
        hip.set_shape_rules(f"1,{M},{N},{K},9,1")          # 160x160 tiles, unsplit
        assert hip.gemm_workspace_bytes(d) == 0
        run()
        hip.set_shape_rules("nonsense;1,2,3")
        assert hip.gemm_workspace_bytes(d) in (base, hip.gemm_workspace_bytes(d))
        run()
        hip.set_shape_rules("off")
        assert hip.gemm_workspace_bytes(d) == base
    finally:
        hip.set_shape_rules(None)
    run()


@pytest.mark.parametrize("n,k,m", [(640, 2560, 640), (33, 70, 1), (5, 1, 97), (1280, 1280, 5120)])
def test_matmul_f32_pack_kernel(hiplib, n, k, m):
    """rcdm_matmul_f32 (weight composition at pack time) against a float64 product; ragged sizes, a vector right side."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(n + k + m)
    a = torch.randn(n, k, generator=g)
    b = torch.randn(k, generator=g) if m == 1 else torch.randn(k, m, generator=g)
    got = hip.matmul_f32(a.to(DEV), b.to(DEV)).cpu()
    ref = (a.double() @ b.double()).float()
    assert got.shape == ref.shape
    assert (got - ref).abs().max() <= 2e-5 * (k ** 0.5) * max(ref.abs().max().item(), 1.0)


def test_conv3x3_upsample_phase_form_refusals(hiplib):
    """Shapes and epilogues the phase form does not take are refused by rcdm_conv3x3 and reported by the query."""
    from rcdms_amd import hip
    ok = hip.ConvDesc(10, 16, 16, 1280, 1280, 1, 2, 1280, 1280, 0, hip.EPI_BIAS, 1, 0, 1.0, 0)
    assert hip.conv3x3_up2_supported(ok)
    for bad in (hip.ConvDesc(10, 16, 16, 1280, 1280, 1, 2, 1280, 1280, 1280, hip.EPI_BIAS | hip.EPI_RESIDUAL, 1, 0, 1.0, 0),
                hip.ConvDesc(10, 16, 16, 1272, 1280, 1, 2, 1272, 1280, 0, hip.EPI_BIAS, 1, 0, 1.0, 0),     # c_in % 64
                hip.ConvDesc(1, 8, 8, 64, 64, 1, 2, 64, 64, 0, hip.EPI_BIAS, 1, 0, 1.0, 0),                # does not fill the chip
                hip.ConvDesc(10, 16, 16, 1280, 1280, 2, 2, 1280, 1280, 0, hip.EPI_BIAS, 1, 0, 1.0, 0)):    # stride 2
        assert not hip.conv3x3_up2_supported(bad)
        x = torch.zeros(16, dtype=torch.float16, device=DEV)
        with pytest.raises(hip.RcdmError):
            hip.conv3x3(bad, x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), x.data_ptr(), 0, 0)


@pytest.mark.parametrize("b,f,H,W,C,cross,silu", [
    (2, 5, 8, 8, 320, True, True),      # resnet norm: statistics across the 5 frames
    (2, 5, 8, 8, 320, False, False),    # transformer / motion-module norm: per frame, eps 1e-6
    (1, 5, 16, 16, 64, True, True),     # cg = 2 (tiny config)
    (2, 3, 4, 4, 2560, True, True),     # widest concat input
    (1, 2, 6, 10, 960, False, True),
    # production shapes of the 8x8 / 16x16 / 32x32 levels: the single-launch form (one block per sample x group bundle)
    (2, 5, 8, 8, 1280, True, True),     # cg = 40: one group per block
    (2, 5, 16, 16, 1280, False, False), # 10 samples x 32 blocks
    (2, 5, 32, 32, 640, False, False),  # cg = 20: two groups per block
    (2, 5, 16, 16, 2560, True, True),   # cg = 80, 1280 rows per sample
    (2, 5, 16, 16, 1920, True, True),   # cg = 60: too few blocks for the single-launch form, three-launch path
    (2, 5, 7, 9, 1280, True, True),     # ragged row count (315 rows per sample)
])
def test_groupnorm(hiplib, b, f, H, W, C, cross, silu):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(5 + C)
    x = h16(torch.randn(b, C, f, H, W, generator=g) * 2.0 + 0.7)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5 if cross else 1e-6
    if cross:
        ref = O.group_norm_cross_frame(x, gamma, beta, 32, eps)
    else:
        x4 = x.permute(0, 2, 1, 3, 4).reshape(b * f, C, H, W)
        ref = O.group_norm_per_frame(x4, gamma, beta, 32, eps).reshape(b, f, C, H, W).permute(0, 2, 1, 3, 4)
    if silu:
        ref = F.silu(ref)
    ldx = C + 8
    xd = rows_from_5d(x, ldx)
    y = gout(b * f * H * W, C)
    samples, rps = (b, f * H * W) if cross else (b * f, H * W)
    d = hip.GroupNormDesc(samples, rps, C, 32, ldx, C, eps, int(silu))
    w = ws(hip.groupnorm_workspace_bytes(d))
    gd, bd = gvec(gamma), gvec(beta)
    hip.groupnorm_silu(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    close(rows_to_5d(y, b, C, f, H, W), ref)
    check_all(y, xd, gd, bd)


@pytest.mark.parametrize("kind,b,f,H,W,cin,cout,cross,split,variant", [
    ("conv", 2, 5, 32, 32, 128, 640, True, 2, -1),     # conv1 -> norm2 of a 32x32-level ResNet block (cross-frame statistics)
    ("conv", 2, 5, 32, 32, 128, 640, False, 3, -1),    # conv2 (+ residual) -> the per-frame norm in front of a transformer
    ("conv", 2, 5, 16, 16, 128, 320, True, 4, 9),      # 160x160 tiles, cg = 10 (groups straddle 16-byte chunks)
    ("conv", 1, 5, 24, 24, 64, 960, False, 2, 1),      # one sample per image, 576 rows each
    ("gemm", 2, 5, 32, 32, 1280, 640, False, 4, -1),   # the proj_out-composed feed-forward GEMM -> a motion module's norm
    ("gemm", 2, 5, 16, 16, 640, 640, True, 2, 5),
    ("conv+1x1", 2, 5, 32, 32, 128, 640, False, 2, -1),   # conv2 + conv_shortcut (rcdm_conv3x3_add1x1_gnstat) -> a transformer's norm
    ("conv+1x1", 2, 5, 16, 16, 128, 320, True, 4, 9),     # ... on 160x160 tiles (cross-frame norm): the second input's k-steps in the last slab
])
def test_splitk_gnstat_is_bit_identical(hiplib, kind, b, f, H, W, cin, cout, cross, split, variant):
    """rcdm_conv3x3_gnstat / rcdm_gemm_gnstat + rcdm_groupnorm_silu_prestat (the split-K reduce pass leaves the partial
    statistics of the GroupNorm that reads its output next: resnet.py:185-202 conv1 -> norm2, attention.py:328 /
    motion_module.py:162 behind conv2 or the feed-forward) against the separate launches rcdm_conv3x3 / rcdm_gemm +
    rcdm_groupnorm_silu: the producer's rows AND the norm's output must be bit-identical (statistics from the stored halfs,
    same order of additions), and the norm matches the oracle."""
    from rcdms_amd import hip
    hip.set_igemm_variant(variant)
    g = torch.Generator().manual_seed(31 + cin + cout + split)
    n_img, M = b * f, b * f * H * W
    bias = gvec(torch.randn(cout, generator=g))
    rv = gvec(torch.randn(b, cout, generator=g))                         # per-sample row vector (time_emb_proj rows)
    res = gin(h16(torch.randn(M, cout, generator=g)).half())
    gamma, beta = gvec(torch.randn(cout, generator=g)), gvec(torch.randn(cout, generator=g))
    samples, rps = (b, f * H * W) if cross else (n_img, H * W)
    ldc = cout + 8
    gnd = hip.GroupNormDesc(samples, rps, cout, 32, ldc, cout, 1e-5 if cross else 1e-6, int(cross))
    epi = 1 | 2 | 4
    if kind == "conv+1x1":
        cin2 = 192
        x = gin(h16(torch.randn(M, cin, generator=g)).half())
        x2 = gin(h16(torch.randn(M, cin2, generator=g)).half())
        w = gw(h16(torch.randn(cout, 9 * cin + cin2, generator=g) * (9 * cin) ** -0.5))
        d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin, ldc, cout, epi, f * H * W, cout, 1.0, split, 0, 0, cin2, cin2)
        wsb = hip.conv3x3_workspace_bytes(d)
        ok = hip.conv3x3_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.conv3x3_add1x1(d, x.data_ptr(), x2.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(),
                                                o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.conv3x3_add1x1_gnstat(d, gnd, x.data_ptr(), x2.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(),
                                                          res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
    elif kind == "conv":
        x = gin(h16(torch.randn(M, cin, generator=g)).half())
        w = gw(h16(torch.randn(cout, 9 * cin, generator=g) * (9 * cin) ** -0.5))
        d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin, ldc, cout, epi, f * H * W, cout, 1.0, split, 0, 0)
        wsb = hip.conv3x3_workspace_bytes(d)
        ok = hip.conv3x3_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.conv3x3(d, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.conv3x3_gnstat(d, gnd, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(),
                                                   k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
    else:
        x = gin(h16(torch.randn(M, cin, generator=g)).half())
        w = gw(h16(torch.randn(cout, cin, generator=g) * cin ** -0.5))
        d = hip.GemmDesc(M, cout, cin, cin, ldc, cout, epi, f * H * W, cout, 1.0, split, 0)
        wsb = hip.gemm_workspace_bytes(d)
        ok = hip.gemm_gnstat_ok(d, gnd)
        plain = lambda o, k: hip.gemm(d, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(), k.data_ptr(), k.numel())
        fused = lambda o, k, gk: hip.gemm_gnstat(d, gnd, x.data_ptr(), w.data_ptr(), bias.data_ptr(), rv.data_ptr(), res.data_ptr(), o.data_ptr(),
                                                k.data_ptr(), k.numel(), gk.data_ptr(), gk.numel())
    assert wsb > 0 and ok and hip.groupnorm_prestat_ok(gnd)
    outs = []
    for mode in ("separate", "fused"):
        o = gout(M, cout, ldc)
        y = gout(M, cout)
        k, gk = ws(wsb), ws(hip.groupnorm_workspace_bytes(gnd))
        if mode == "separate":
            plain(o, k)
            hip.groupnorm_silu(gnd, o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), gk.data_ptr(), gk.numel())
        else:
            fused(o, k, gk)
            hip.groupnorm_silu_prestat(gnd, o.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), gk.data_ptr(), gk.numel())
        torch.cuda.synchronize()
        outs.append((o[:, :cout].clone(), y.clone()))
        assert torch.isnan(o[:, cout:].float()).all(), "wrote outside the output columns"
        check_all(o, y, x, w, bias, rv, res, gamma, beta)
        check_written(o), check_written(y)       # names the rows a skipped tile or slab left unwritten
    hip.set_igemm_variant(-1)
    assert torch.equal(outs[0][0], outs[1][0]), "the producer's rows differ"
    assert torch.equal(outs[0][1], outs[1][1]), "the norm's output differs"
    # ... and the norm is the reference's GroupNorm of those rows
    o32 = outs[1][0].float().cpu().reshape(b, f, H, W, cout).permute(0, 4, 1, 2, 3)
    if cross:
        ref = F.silu(O.group_norm_cross_frame(o32, gamma.cpu(), beta.cpu(), 32, 1e-5))
    else:
        x4 = o32.permute(0, 2, 1, 3, 4).reshape(n_img, cout, H, W)
        ref = O.group_norm_per_frame(x4, gamma.cpu(), beta.cpu(), 32, 1e-6).reshape(b, f, cout, H, W).permute(0, 2, 1, 3, 4)
    close(rows_to_5d(outs[1][1], b, cout, f, H, W), ref)


def test_gnstat_refusals(hiplib):
    """Loud refusals: a launch that is not split-K has no reduce pass to carry the statistics; a norm that runs as one launch has
    no statistics pass to replace; mismatched rows."""
    from rcdms_amd import hip
    M, C = 10240, 640
    d1 = hip.GemmDesc(M, C, 640, 640, C, 0, 1, 1, 0, 1.0, 1, 0)          # split_k = 1: no slabs
    gnd = hip.GroupNormDesc(10, 1024, C, 32, C, C, 1e-6, 0)
    assert not hip.gemm_gnstat_ok(d1, gnd)
    d2 = hip.GemmDesc(M, C, 640, 640, C, 0, 1, 1, 0, 1.0, 2, 0)
    assert hip.gemm_gnstat_ok(d2, gnd)
    assert not hip.gemm_gnstat_ok(d2, hip.GroupNormDesc(10, 512, C, 32, C, C, 1e-6, 0))       # other row count
    assert not hip.gemm_gnstat_ok(d2, hip.GroupNormDesc(10, 1024, C, 32, C + 8, C, 1e-6, 0))  # other row stride
    small = hip.GroupNormDesc(10, 64, 1280, 32, 1280, 1280, 1e-6, 0)                         # single-launch norm (8x8 level)
    assert not hip.groupnorm_prestat_ok(small)
    x = torch.zeros(M, C, dtype=torch.float16, device=DEV)
    k = ws(hip.gemm_workspace_bytes(d1) + 16)
    with pytest.raises(hip.RcdmError):
        hip.gemm_gnstat(d1, gnd, x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 0, x.data_ptr(), k.data_ptr(), k.numel(), k.data_ptr(), k.numel())
    with pytest.raises(hip.RcdmError):
        hip.groupnorm_silu_prestat(small, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), k.data_ptr(), k.numel())
    torch.cuda.synchronize()


@pytest.mark.parametrize("b,f,H,W,C", [(2, 5, 32, 32, 640), (2, 5, 64, 64, 320), (1, 4, 24, 24, 960), (2, 5, 32, 32, 64)])
def test_groupnorm_fold_is_bit_identical(hiplib, b, f, H, W, C):
    """Per-frame norms with many samples run as statistics + an apply kernel that finalises the groups itself (round 4); the
    result must be bit-identical to the three-launch form (same Chan combination in the same order)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(21 + C)
    x = h16(torch.randn(b * f * H * W, C, generator=g) * 3.0 + 1.5)
    gamma, beta = gvec(torch.randn(C, generator=g)), gvec(torch.randn(C, generator=g))
    xd = gin(x.half())
    d = hip.GroupNormDesc(b * f, H * W, C, 32, C, C, 1e-6, 0)
    w = ws(hip.groupnorm_workspace_bytes(d))
    outs = []
    for mode in (0, 1):
        hip.set_groupnorm_fold(mode)
        y = gout(b * f * H * W, C)
        hip.groupnorm_silu(d, xd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
        outs.append(y)
    hip.set_groupnorm_fold(-1)
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
    check_all(*outs, xd, gamma, beta)
    check_written(outs[0]), check_written(outs[1])


@pytest.mark.parametrize("M,C,pe", [(50, 320, False), (40, 640, True), (7, 1280, True), (33, 64, False),
                                    # production-sized row counts, ragged last wave
                                    (2051, 320, False), (2400, 320, True), (2049, 640, True), (2050, 1280, False),
                                    (2400, 1280, True), (2048, 960, False),
                                    # widths that do not fill the row-group kernel's lanes evenly (masked chunks), the
                                    # widest it takes (stage-1 prior), one row, and a few thousand rows of a narrow matrix
                                    (97, 768, False), (970, 2048, False), (1, 200, False), (5000, 72, False), (20, 1000, True)])
def test_layernorm(hiplib, M, C, pe):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(11 + C)
    frames, rpf = 5, 4
    if pe and M < 2048:
        M = 2 * frames * rpf
    if pe and M >= 2048:
        rpf = 240                       # 2400 rows = 2 samples x 5 frames x 240 rows
    x = h16(torch.randn(M, C, generator=g) * 3 + 1)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    table = O.sinusoid_table(C, frames)
    if pe:
        ref = ref + table[(torch.arange(M) // rpf) % frames]
    xd = gin(x.half())
    y = gout(M, C)
    d = hip.LayerNormDesc(M, C, C, C, 1e-5, rpf, frames)
    gd, bd, td = gvec(gamma), gvec(beta), gvec(table)
    hip.layernorm(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), td.data_ptr() if pe else 0, y.data_ptr())
    torch.cuda.synchronize()
    close(y, ref)
    check_all(y, xd, gd, bd, td)


@pytest.mark.parametrize("batch,heads,Lq,Lk,d", [
    (2, 8, 256, 256, 40),    # self-attention, 64x64-latent head dim
    (2, 8, 200, 85, 40),     # cross-attention over 85 context rows (ragged key tile, ragged query tile)
    (3, 8, 64, 91, 80),
    (1, 8, 130, 130, 160),
    (2, 8, 16, 16, 160),     # 256x256 image mid block: 4x4 latent patches
    (2, 4, 96, 85, 8),       # tiny-config head dims
    (1, 2, 70, 64, 16),
    (1, 2, 64, 70, 32),
])
def test_flash_attn(hiplib, batch, heads, Lq, Lk, d):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(3 + Lq + Lk + d)
    C = heads * d
    q = h16(torch.randn(batch, Lq, C, generator=g))
    k = h16(torch.randn(batch, Lk, C, generator=g))
    v = h16(torch.randn(batch, Lk, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    # q inside a fused [q|k|v]-style wider buffer, k/v interleaved in one [k|v] buffer
    qd = gin(q.reshape(-1, C).half(), 3 * C)
    kv = gin(torch.cat([k.reshape(-1, C), v.reshape(-1, C)], dim=1).half())
    out = gout(batch * Lq, C)
    desc = hip.AttnDesc(batch, heads, Lq, Lk, d, 3 * C, 2 * C, 2 * C, C, d ** -0.5)
    hip.flash_attn(desc, qd.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, out.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(batch, Lq, C), ref)
    check_all(out, qd, kv)


@pytest.mark.parametrize("batch,heads,Lq,Lk,d", [
    (2, 8, 4096, 85, 40),    # the stage-2 cross-attention sites at 64x64 / 32x32 / 16x16 / 8x8 latents
    (10, 8, 1024, 85, 80),
    (2, 8, 256, 91, 160),    # FlintstonesSV context length
    (10, 8, 64, 85, 160),
    (1, 8, 100, 96, 40),     # ragged query count, full key capacity
    (3, 4, 33, 1, 40),       # a single key: softmax == 1, output == V row
    (2, 2, 70, 13, 32),      # tiny-config shapes (no spare dim row at d = 32: VALU row sum)
    (1, 1, 5, 50, 8),
])
def test_xattn_short_keys(hiplib, batch, heads, Lq, Lk, d):
    """rcdm_xattn_pack_kv + rcdm_xattn (cross-attention with Lk <= 96, scores held in registers) vs the oracle attention
    and vs rcdm_flash_attn on the same buffers."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(11 + Lq + Lk + d)
    C = heads * d
    q = h16(torch.randn(batch, Lq, C, generator=g))
    k = h16(torch.randn(batch, Lk, C, generator=g))
    v = h16(torch.randn(batch, Lk, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    qd = gin(q.reshape(-1, C).half())
    kv = gin(torch.cat([k.reshape(-1, C), v.reshape(-1, C)], dim=1).half())        # [K | V] rows, as the context GEMM writes
    img = gout(1, hip.xattn_image_bytes(batch, heads, d), dtype=torch.uint8, guard_rows=1)
    out = gout(batch * Lq, C)
    out_f = gout(batch * Lq, C)
    desc = hip.AttnDesc(batch, heads, Lq, Lk, d, C, 2 * C, 2 * C, C, d ** -0.5)
    hip.xattn_pack_kv(kv.data_ptr(), kv.data_ptr() + 2 * C, batch, Lk, heads, d, 2 * C, 2 * C, img.data_ptr())
    hip.xattn(desc, qd.data_ptr(), img.data_ptr(), out.data_ptr())
    hip.flash_attn(desc, qd.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, out_f.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(batch, Lq, C), ref)
    assert (out.float() - out_f.float()).abs().max().item() <= 2e-3 * ref.abs().max().item() + 1e-3
    check_all(out, out_f, img, qd, kv)


def test_xattn_rejects_long_keys(hiplib):
    from rcdms_amd import hip
    desc = hip.AttnDesc(1, 8, 64, 97, 40, 320, 640, 640, 320, 40 ** -0.5)
    x = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
        hip.xattn(desc, x.data_ptr(), x.data_ptr(), x.data_ptr())
    assert hip.xattn_image_bytes(2, 8, 40) == 2 * 8 * (9 + 12) * 1024 and hip.xattn_image_bytes(1, 8, 160) == 8 * (30 + 30) * 1024


@pytest.mark.parametrize("batch,heads,L,d,causal,pad", [
    (2, 4, 97, 64, True, True),      # the stage-1 prior's shape: 91 text + 6 extra tokens, causal + text padding
    (2, 4, 97, 64, True, False),
    (3, 2, 150, 40, False, True),    # padding only, three key tiles
    (1, 2, 64, 160, True, True),     # un-pipelined (d > 80) variant
])
def test_flash_attn_masked(hiplib, batch, heads, L, d, causal, pad):
    """rcdm_flash_attn_masked vs the reference's ADDITIVE mask (0 / -10000, myprior_transformer.py:389-393)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(5 + L + d)
    C = heads * d
    q, k, v = (h16(torch.randn(batch, L, C, generator=g)) for _ in range(3))
    valid = torch.ones(batch, L, dtype=torch.uint8)
    if pad:
        for b in range(batch):
            valid[b, 20 + 7 * b:L - 6] = 0          # padded text tokens; the trailing extra tokens stay visible
    add = (1.0 - valid.float())[:, None, :] * -10000.0
    if causal:
        add = add + torch.full((L, L), -10000.0).triu_(1)[None]
    else:
        add = add.expand(batch, L, L)
    ref = O.attention_core(q, k, v, heads, mask=add)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    vm = valid.to(DEV)
    out = gout(batch * L, C)
    desc = hip.AttnDesc(batch, heads, L, L, d, C, C, C, C, d ** -0.5)
    hip.flash_attn_masked(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), vm.data_ptr() if pad else 0, causal,
                          out.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(batch, L, C), ref)
    check_all(out, qd, kd, vd)


def test_gemm_gelu(hiplib):
    """Linear -> exact GELU epilogue (the prior's FeedForward(activation_fn="gelu")), plain and split-K paths."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(23)
    for M, N, K, split in [(970, 512, 256, 1), (130, 72, 200, 3)]:
        A = h16(torch.randn(M, K, generator=g))
        W = h16(torch.randn(N, K, generator=g) * K ** -0.5)
        bias = torch.randn(N, generator=g)
        ref = F.gelu(F.linear(A, W, bias))
        Ad, Wd, bd = gin(A.half()), gw(W), gvec(bias)
        out = gout(M, N)
        dsc = hip.GemmDesc(M, N, K, K, N, 0, hip.EPI_BIAS | hip.EPI_GELU, 1, 0, 1.0, split)
        w = ws(hip.gemm_workspace_bytes(dsc))
        hip.gemm(dsc, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), w.data_ptr(), w.numel())
        torch.cuda.synchronize()
        close(out, ref)
        check_all(out, Ad, Wd, bd)


def test_flash_attn_forced_rescale(hiplib):
    """A key in a LATE tile that dominates one query's scores forces the online-softmax rescale branch."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(21)
    heads, d, L = 2, 40, 256
    C = heads * d
    q = h16(torch.randn(1, L, C, generator=g))
    k = h16(torch.randn(1, L, C, generator=g))
    v = h16(torch.randn(1, L, C, generator=g))
    k[0, 200, :d] = h16(q[0, 17, :d] * 4.0)      # spike in the 4th key tile for query 17 / head 0
    ref = O.attention_core(q, k, v, heads)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    out = gout(L, C)
    desc = hip.AttnDesc(1, heads, L, L, d, C, C, C, C, d ** -0.5)
    hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    close(out.reshape(1, L, C), ref)
    check_all(out, qd, kd, vd)


@pytest.mark.parametrize("L,boost", [(1024, (1.3, 1.8, 2.5, 4.0)), (4096, (1.5, 3.0)), (512, ())])
def test_flash_attn_deferred_max_long_keys(hiplib, L, boost):
    """The d = 40 kernel with the softmax argument out of the matrix pipe (MSUB: Q pre-scaled, running max in a spare
    QK^T column, the max only raised when a tile exceeds it by 2^6): long key loops where the max (a) never moves after the
    first tile, (b) creeps up by less than the threshold (P > 1 in later tiles), (c) jumps by more in several late tiles —
    every case against the full fp32 oracle, and bit-identical on a second run."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(31 + L)
    heads, d = 2, 40
    C = heads * d
    q = h16(torch.randn(1, L, C, generator=g))
    k = h16(torch.randn(1, L, C, generator=g))
    v = h16(torch.randn(1, L, C, generator=g))
    for i, f in enumerate(boost):            # growing spikes in later and later key tiles, for a few queries each
        key = (i + 1) * L // (len(boost) + 1) + 3
        for qi in (5 + 64 * i, 40 + 64 * i):
            k[0, key + (qi & 7), :d] = h16(q[0, qi, :d] * f)
    ref = O.attention_core(q, k, v, heads)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    desc = hip.AttnDesc(1, heads, L, L, d, C, C, C, C, d ** -0.5)
    outs = []
    for _ in range(2):
        out = gout(L, C)
        hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        outs.append(out)
    close(outs[0].reshape(1, L, C), ref)
    assert torch.equal(outs[0], outs[1])
    check_all(*outs, qd, kd, vd)


@pytest.mark.parametrize("gain", [6.0, 30.0])
def test_flash_attn_msub_large_logits(hiplib, gain):
    """Large scaled scores through the d = 40 MSUB kernel (running max held as f16 inside the Q fragment, Q pre-scaled and
    re-rounded to f16): q, k scaled so that |scale * log2(e) * q.k| reaches ~50 (gain 6) and ~1300 (gain 30, softmax nearly
    one-hot).  Documented range of the kernel: |scaled score| < 2^15 (rcdm.h).  No inf / NaN, and the output stays within
    the stated tolerance of the fp32 oracle on the same f16 inputs; the fma-path kernel (RCDM_ATTN_MSUB=0) has no such
    re-rounding, so the measured difference between the two is printed."""
    from rcdms_amd import hip
    L, heads, d = 1024, 2, 40
    C = heads * d
    g = torch.Generator().manual_seed(77)
    q = h16(torch.randn(1, L, C, generator=g) * gain ** 0.5)
    k = h16(torch.randn(1, L, C, generator=g) * gain ** 0.5)
    v = h16(torch.randn(1, L, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    out = gout(L, C)
    desc = hip.AttnDesc(1, heads, L, L, d, C, C, C, C, d ** -0.5)
    hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, qd, kd, vd)
    got = out.float().cpu().reshape(1, L, C)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    smax = (torch.einsum("blhd,bmhd->bhlm", q.view(1, L, heads, d), k.view(1, L, heads, d)).abs().max() * d ** -0.5 * 1.4427).item()
    print(f"gain {gain}: max |scaled score| {smax:.0f}, max abs err {err:.3e} (|ref| max {ref.abs().max():.2f})")
    # P carries a relative error of ~ln2 * 2^-12 * |scaled score| from the f16 rounding of Q * c: ~1 % at 50, ~20 % at 1300 on the
    # (few) keys that share the top of a nearly one-hot row
    close(got, ref, rel=2e-3, abs_frac=4e-3 if gain <= 6 else 4e-2)


def test_flash_attn_wide_range_flag(hiplib):
    """RCDM_ATTN_WIDE_RANGE (what rcdms_amd.engine sets when its weight-norm bound of a site's scores reaches 2^15): the
    d = 40 launch takes the fp32-argument softmax kernel, whose error does not grow with the score magnitude.  Scores of
    ~1300 here: with the flag the result is at the ordinary tolerance, where the matrix-pipe-softmax kernel needs 10x that
    (test_flash_attn_msub_large_logits)."""
    from rcdms_amd import hip
    L, heads, d, gain = 1024, 2, 40, 30.0
    C = heads * d
    g = torch.Generator().manual_seed(77)
    q = h16(torch.randn(1, L, C, generator=g) * gain ** 0.5)
    k = h16(torch.randn(1, L, C, generator=g) * gain ** 0.5)
    v = h16(torch.randn(1, L, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    qd, kd, vd = (gin(t.reshape(-1, C).half()) for t in (q, k, v))
    errs = []
    for flags in (0, hip.ATTN_WIDE_RANGE):
        out = gout(L, C)
        desc = hip.AttnDesc(1, heads, L, L, d, C, C, C, C, d ** -0.5, flags)
        hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        got = out.float().cpu().reshape(1, L, C)
        assert torch.isfinite(got).all()
        errs.append((got - ref).abs().max().item())
        if flags:
            close(got, ref, rel=2e-3, abs_frac=4e-3)
        check_all(out, qd, kd, vd)
    print(f"|scaled score| ~1300: max abs err {errs[0]:.3e} (matrix-pipe softmax argument) vs {errs[1]:.3e} (RCDM_ATTN_WIDE_RANGE)")
    assert errs[1] < errs[0]


@pytest.mark.parametrize("b,frames,pixels,heads,d", [(2, 5, 64, 8, 40), (1, 5, 16, 8, 160), (2, 5, 33, 8, 8), (1, 3, 20, 4, 16)])
def test_temporal_attn(hiplib, b, frames, pixels, heads, d):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(17 + pixels + d)
    C = heads * d
    qkv = h16(torch.randn(b * frames * pixels, 3 * C, generator=g))
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]

    def regroup(x):  # "(b f) d c -> (b d) f c"  motion_module.py:299
        return x.reshape(b, frames, pixels, C).permute(0, 2, 1, 3).reshape(b * pixels, frames, C)

    o = O.attention_core(regroup(q), regroup(k), regroup(v), heads)
    ref = o.reshape(b, pixels, frames, C).permute(0, 2, 1, 3).reshape(b * frames * pixels, C)
    out = gout(b * frames * pixels, C)
    desc = hip.TemporalAttnDesc(b, frames, pixels, heads, d, 3 * C, C, d ** -0.5)
    qkv_d = gin(qkv.half())
    hip.temporal_attn(desc, qkv_d.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    close(out, ref)
    check_all(out, qkv_d)


def test_timestep_embed_and_small_linear(hiplib):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(2)
    t = torch.tensor([981.0, 981.0, 1.0])
    ref = O.timestep_embedding(t, 320)
    out = gout(3, 320, dtype=torch.float32)
    t_d = gvec(t)
    hip.timestep_embed(t_d.data_ptr(), 3, 320, out.data_ptr())
    torch.cuda.synchronize()
    assert (out.cpu() - ref).abs().max() < 2e-4
    W1 = h16(torch.randn(1280, 320, generator=g) * 0.05)
    b1 = torch.randn(1280, generator=g)
    ref2 = F.silu(F.linear(ref, W1, b1))
    o2 = gout(3, 1280, dtype=torch.float32)
    W1d, b1d = gw(W1), gvec(b1)
    hip.small_linear(out.data_ptr(), 3, 320, W1d.data_ptr(), b1d.data_ptr(), 1280, 0, 1, o2.data_ptr())
    W2 = h16(torch.randn(200, 1280, generator=g) * 0.03)
    ref3 = F.linear(F.silu(ref2), W2)
    o3 = gout(3, 200, dtype=torch.float32)
    W2d = gw(W2)
    hip.small_linear(o2.data_ptr(), 3, 1280, W2d.data_ptr(), 0, 200, 1, 0, o3.data_ptr())
    torch.cuda.synchronize()
    close(o2, ref2, rel=1e-3, abs_frac=1e-3)
    close(o3, ref3, rel=1e-3, abs_frac=1e-3)
    check_all(out, o2, o3, t_d, W1d, b1d, W2d)


def test_layout_and_ddim(hiplib):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(8)
    S, f, H, W = 2, 5, 8, 8
    lat = torch.randn(S, 4, f, H, W, generator=g)
    mask = (torch.rand(2 * S, 1, f, H, W, generator=g) > 0.5).float()
    masked = torch.randn(2 * S, 4, f, H, W, generator=g)
    ref_in = torch.cat([torch.cat([lat] * 2), mask, masked], dim=1)       # RCDMs_pipeline.py:482-486
    rows = gout(2 * S * f * H * W, 64)
    lat0, mask_d, masked_d = gvec(lat), gvec(mask), gvec(masked)
    hip.assemble_input(lat0.data_ptr(), mask_d.data_ptr(), masked_d.data_ptr(), S, 2, f, H, W, rows.data_ptr(), 64, 64)
    torch.cuda.synchronize()
    close(rows_to_5d(rows, 2 * S, 9, f, H, W), ref_in, rel=1e-3, abs_frac=1e-3)
    assert (rows[:, 9:] == 0).all()
    check_all(rows, lat0, mask_d, masked_d)
    # generic converters round-trip
    x = torch.randn(3, 9, f, H, W, generator=g)
    r2 = gout(3 * f * H * W, 16)
    x_d = gvec(x)
    hip.ncfhw_to_rows(x_d.data_ptr(), 3, 9, f, H, W, r2.data_ptr(), 16, 16)
    back_h = gout(1, 3 * 9 * f * H * W, dtype=torch.float32, guard_rows=1)
    back = back_h.view(3, 9, f, H, W)
    hip.rows_to_ncfhw(r2.data_ptr(), 16, 3, 9, f, H, W, back.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(back.cpu(), x.half().float())
    check_all(r2, back_h, x_d)
    # CFG + DDIM step against the oracle scheduler
    sched = O.DDIMOracle(); sched.set_timesteps(20)
    eps = h16(torch.randn(2 * S, 4, f, H, W, generator=g))
    eps_rows = rows_from_5d(eps, 32)
    gs = 2.0
    coef = []
    for t in sched.timesteps:
        pt = int(t) - 1000 // 20
        a_t = sched.alphas_cumprod[int(t)]; a_p = sched.alphas_cumprod[pt] if pt >= 0 else torch.tensor(1.0)
        coef.append([a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()])
    coef = gvec(torch.tensor(coef, dtype=torch.float32))
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    lat_h = gout(1, lat.numel(), dtype=torch.float32, guard_rows=1)     # in place: the state sits between NaN guard bands
    lat_h[0].copy_(lat.reshape(-1))
    lat_d = lat_h.view(lat.shape)
    hip.cfg_ddim_step(eps_rows.data_ptr(), 32, lat_d.data_ptr(), S, 2, f, H, W, gs, coef.data_ptr(), step.data_ptr())
    hip.advance_step(step.data_ptr())
    torch.cuda.synchronize()
    e_u, e_c = eps.chunk(2)
    ref = sched.step(e_u + gs * (e_c - e_u), sched.timesteps[3], lat)
    assert (lat_d.cpu() - ref).abs().max() < 1e-5
    assert int(step.item()) == 4
    check_all(lat_h, eps_rows, coef)


def test_cfg_pndm_step_vs_scheduler(hiplib):
    """rcdm_cfg_pndm_step replayed over a whole PLMS schedule (device step counter, prediction ring, saved first sample)
    against the host-visible PNDMScheduler.step (diffusers 0.24.0 arithmetic restated; parity unpinned) and against the
    oracle's independent PNDMOracle."""
    from rcdms_amd import hip
    from rcdms_amd.scheduler import PNDMScheduler
    S, f, H, W, gs, n = 2, 5, 8, 8, 2.0, 9
    g = torch.Generator().manual_seed(11)
    sched = PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, skip_prk_steps=True)
    sched.set_timesteps(n)
    orc = O.PNDMOracle(beta_schedule="scaled_linear"); orc.set_timesteps(n)
    assert torch.equal(sched.timesteps, orc.timesteps)
    tab = gvec(sched.plms_table())
    lat = torch.randn(S, 4, f, H, W, generator=g)
    lat_h = gout(1, lat.numel(), dtype=torch.float32, guard_rows=1)     # in place: the state sits between NaN guard bands
    lat_h[0].copy_(lat.reshape(-1))
    lat_d = lat_h.view(lat.shape)
    hist = gout(5, S * 4 * f * H * W, dtype=torch.float32, guard_rows=1)  # (no initialisation needed: NaN-filled)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    x, xo = lat.clone(), lat.clone()
    for i, t in enumerate(sched.timesteps.tolist()):
        eps = h16(torch.randn(2 * S, 4, f, H, W, generator=g))
        rows = rows_from_5d(eps, 32)
        hip.cfg_pndm_step(rows.data_ptr(), 32, lat_d.data_ptr(), hist.data_ptr(), S, 2, f, H, W, gs, tab.data_ptr(), step.data_ptr())
        hip.advance_step(step.data_ptr())
        torch.cuda.synchronize()
        e_u, e_c = eps.chunk(2)
        e = e_u + gs * (e_c - e_u)
        x = sched.step(e, t, x).prev_sample
        xo = orc.step(e, t, xo)
        assert (lat_d.cpu() - x).abs().max() < 2e-5 * max(1.0, x.abs().max().item()), i
        assert (x - xo).abs().max() < 2e-5 * max(1.0, x.abs().max().item()), i
        check_all(lat_h, hist, rows, tab)
    assert int(step.item()) == n + 1


def test_graph_capture_replay(hiplib):
    from rcdms_amd import hip
    M = N = K = 128
    A = torch.randn(M, K).half().to(DEV)
    W = torch.randn(N, K).half().to(DEV)
    out = torch.zeros(M, N, dtype=torch.float16, device=DEV)
    d = hip.GemmDesc(M, N, K, K, N, N, 0, 1, 0, 1.0, 1)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gr = hip.Graph()
        gr.begin()
        hip.gemm(d, A.data_ptr(), W.data_ptr(), 0, 0, 0, out.data_ptr(), 0, 0)
        gr.end()
        assert float(out.abs().sum()) == 0.0, "capture must not execute"
        gr.launch()
        s.synchronize()
    close(out, A.float().cpu() @ W.float().cpu().t())


# ------------------------------------------------------------------------------------------------
# Layouts the engine uses and no test above runs: every row stride wider than its operand, all of them at once, the pad
# columns poisoned (inputs) or NaN (outputs).  lda = c_in + 8, lda2 = c_in2 + 16, ldc = c_out + 24, ldr = c_out + 16,
# ldt = c_out + 8: all different, so a stride taken from the wrong field shows too.
def _gn_rows(x2d, samples, rps, C, groups, eps, dtype=torch.float64):
    """(mean, rstd) [samples][groups] of rows [samples * rps][C] in `dtype` (biased variance, torch.nn.GroupNorm)."""
    v = x2d.to(dtype).reshape(samples, rps, groups, C // groups)
    mean = v.mean(dim=(1, 3))
    var = v.var(dim=(1, 3), unbiased=False)
    return mean, (var + eps).rsqrt()


PADDED_CONVS = [
    # form, b, f, H, W, cin, cin2, cout, split, variant   (per form: a ragged case, then a production-shaped one)
    ("plain", 2, 3, 10, 6, 72, 0, 72, 1, 1),
    ("plain", 2, 5, 16, 16, 320, 0, 320, 0, -1),
    ("stride2", 1, 3, 9, 7, 72, 0, 40, 1, 2),           # odd sides: h_out = 5, w_out = 4
    ("stride2", 2, 5, 16, 16, 320, 0, 320, 0, -1),      # Downsample3D
    ("up1", 1, 3, 5, 3, 72, 0, 72, 1, 1),
    ("up1", 2, 5, 8, 8, 640, 0, 640, 0, -1),            # Upsample3D folded into the conv
    ("up2", 1, 5, 16, 16, 64, 0, 96, 0, 6),             # phase form: N tail of a 320-wide tile
    ("up2", 1, 10, 8, 8, 640, 0, 640, 0, 6),
    ("add1x1", 2, 3, 10, 6, 128, 64, 72, 1, 1),
    ("add1x1", 2, 5, 8, 8, 640, 1280, 640, 0, -1),      # conv2 + conv_shortcut of an up-block ResNet
    ("gnstat", 1, 5, 12, 10, 64, 0, 192, 2, 1),         # 600 rows: M tail on every tile height
    ("gnstat", 2, 5, 16, 16, 128, 0, 320, 4, 9),
    ("add1x1_gnstat", 1, 5, 12, 10, 64, 64, 192, 2, 1),
    ("add1x1_gnstat", 2, 5, 16, 16, 128, 192, 320, 4, 9),
    ("wino", 3, 2, 6, 10, 64, 128, 72, 3, -1),          # N tail, second input, forced split-K
    ("wino", 2, 5, 16, 16, 320, 0, 320, 0, -1),
    ("wino_gn", 1, 5, 12, 10, 64, 0, 192, 0, -1),       # the norm in the input transform + the next norm's partials
    ("wino_gn", 2, 5, 16, 16, 640, 0, 640, 0, -1),
]


@pytest.mark.parametrize("form,b,f,H,W,cin,cin2,cout,split,variant", PADDED_CONVS)
def test_conv_padded_strides(hiplib, form, b, f, H, W, cin, cin2, cout, split, variant):
    """Every convolution form with lda > c_in, lda2 > c_in2, ldc > c_out, ldr > c_out and ldt > c_out together (an up-block
    reads a concat buffer and writes into one): against the fp32 convolution of the f16-rounded operands."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(4000 + cin + cin2 + cout + H)
    up2, wino = form == "up2", form.startswith("wino")
    stride = 2 if form == "stride2" else 1
    up = 1 if form == "up1" else 2 if up2 else 0
    gn_in = form == "wino_gn"
    x = h16(torch.randn(b, cin, f, H, W, generator=g) * 1.5 + 0.3)
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias, temb = torch.randn(cout, generator=g), torch.randn(b, cout, generator=g)
    gamma, beta = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    xin = F.silu(O.group_norm_cross_frame(x, gamma, beta, 32, 1e-5)) if gn_in else x
    xin = F.interpolate(xin, scale_factor=[1.0, 2.0, 2.0], mode="nearest") if up else xin
    ref = O.conv_frames(xin, w, bias, stride=stride, padding=1)
    Ho, Wo = ref.shape[-2:]
    M = b * f * Ho * Wo
    epi = hip.EPI_BIAS if up2 else hip.EPI_BIAS | hip.EPI_ROWVEC | hip.EPI_RESIDUAL     # the phase form takes a bias only
    lda, lda2, ldc, ldr, ldt = cin + 8, cin2 + 16, cout + 24, cout + 16, cout + 8
    x2d = w2 = None
    if cin2:
        x2 = h16(torch.randn(b, cin2, f, H, W, generator=g))
        w2 = h16(torch.randn(cout, cin2, generator=g) * cin2 ** -0.5)
        ref = ref + torch.einsum("oc,bcfhw->bofhw", w2, x2)
        x2d = rows_from_5d(x2, lda2)
    res = h16(torch.randn(ref.shape, generator=g))
    if not up2:
        ref = ref + temb[:, :, None, None, None] + res
    xd, rd = rows_from_5d(x, lda), rows_from_5d(res, ldr)
    w32, bd, td = gvec(w), gvec(bias), gin(temb, ldt, guard_rows=8)
    out = gout(M, cout, ldc)
    d = hip.ConvDesc(b * f, H, W, cin, cout, stride, up, lda, ldc, 0 if up2 else ldr, epi, 1 if up2 else f * Ho * Wo,
                     0 if up2 else ldt, 1.0, split, 0, 0, cin2, lda2 if cin2 else 0)
    ptrs = (0, 0) if up2 else (td.data_ptr(), rd.data_ptr())
    ins = [xd, w32, bd] + ([] if up2 else [td, rd]) + ([x2d] if cin2 else [])
    outs = [out]
    if wino:
        U = gout(16 * cout, cin)
        hip.pack_conv3x3_wino(w32.data_ptr(), cout, cin, U.data_ptr())
        w2d = gw(w2) if cin2 else None
        gd, bed = gvec(gamma), gvec(beta)
        assert hip.conv3x3_wino_supported(d)
        gnd = god = stat = part = None
        if gn_in:
            gnd = hip.GroupNormDesc(b, f * H * W, cin, 32, lda, lda, 1e-5, 1)
            stat = gout(1, b * 32 * 2, dtype=torch.float32, guard_rows=1)
            gws = ws(hip.groupnorm_workspace_bytes(gnd))
            hip.groupnorm_stats(gnd, xd.data_ptr(), stat.data_ptr(), gws.data_ptr(), gws.numel())
            god = hip.GroupNormDesc(b, f * H * W, cout, 32, ldc, ldc, 1e-5, 0)
            part = ws(b * 32 * (f * H * W // 4) * 3 * 4)
            outs.append(stat)
        wsb = ws(hip.conv3x3_wino_workspace_bytes(d))
        hip.conv3x3_wino(d, xd.data_ptr(), U.data_ptr(), bd.data_ptr(), td.data_ptr(), rd.data_ptr(), out.data_ptr(),
                         wsb.data_ptr(), wsb.numel(), x2=x2d.data_ptr() if cin2 else 0, W2=w2d.data_ptr() if cin2 else 0,
                         gn=gnd, gn_stat=stat.data_ptr() if gn_in else 0, gn_gamma=gd.data_ptr() if gn_in else 0,
                         gn_beta=bed.data_ptr() if gn_in else 0, gn_out=god, gn_out_partial=part.data_ptr() if gn_in else 0)
        torch.cuda.synchronize()
        outs.append(U)
        ins += [gd, bed] + ([w2d] if cin2 else [])
        if gn_in:   # the partial statistics the output transform left: finalized, they are the statistics of the stored rows
            st = gout(1, b * 32 * 2, dtype=torch.float32, guard_rows=1)
            hip.groupnorm_finalize(b, 32, f * H * W // 4, 1e-5, part.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            mean, rstd = _gn_rows(out[:, :cout].cpu(), b, f * H * W, cout, 32, 1e-5)
            got = st.cpu().double().reshape(b, 32, 2)
            assert torch.allclose(got[..., 0], mean, rtol=2e-5, atol=1e-6) and torch.allclose(got[..., 1], rstd, rtol=2e-5, atol=1e-6)
            outs.append(st)
    else:
        if up2:
            wp = gout(4 * cout, 4 * cin)
            hip.pack_conv3x3_up2(w32.data_ptr(), cout, cin, wp.data_ptr())
        else:
            wp = gout(cout, 9 * cin)
            hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
        outs.append(wp)
        wk = gw(torch.cat([wp, w2.half().to(DEV)], dim=1)) if cin2 else wp
        gnstat = form.endswith("gnstat")
        hip.set_igemm_variant(variant)
        try:
            if up2:
                assert hip.conv3x3_up2_supported(d)
            wsb = ws(hip.conv3x3_workspace_bytes(d))
            tail = (bd.data_ptr(), *ptrs, out.data_ptr(), wsb.data_ptr(), wsb.numel())
            if gnstat:   # the split-K reduce pass also leaves the statistics of the norm that reads `out` (row stride ldc) next
                gnd = hip.GroupNormDesc(b, f * H * W, cout, 32, ldc, cout + 8, 1e-5, 1)
                assert hip.conv3x3_gnstat_ok(d, gnd) and hip.groupnorm_prestat_ok(gnd)
                gk = ws(hip.groupnorm_workspace_bytes(gnd))
                if cin2:
                    hip.conv3x3_add1x1_gnstat(d, gnd, xd.data_ptr(), x2d.data_ptr(), wk.data_ptr(), *tail, gk.data_ptr(), gk.numel())
                else:
                    hip.conv3x3_gnstat(d, gnd, xd.data_ptr(), wk.data_ptr(), *tail, gk.data_ptr(), gk.numel())
                g2, b2 = torch.randn(cout, generator=g), torch.randn(cout, generator=g)
                g2d, b2d = gvec(g2), gvec(b2)
                y = gout(M, cout, cout + 8)
                hip.groupnorm_silu_prestat(gnd, out.data_ptr(), g2d.data_ptr(), b2d.data_ptr(), y.data_ptr(), gk.data_ptr(), gk.numel())
                torch.cuda.synchronize()
                yref = F.silu(O.group_norm_cross_frame(rows_to_5d(out, b, cout, f, H, W), g2, b2, 32, 1e-5))
                close(rows_to_5d(y, b, cout, f, H, W), yref)
                outs.append(y)
                ins += [g2d, b2d]
            elif cin2:
                hip.conv3x3_add1x1(d, xd.data_ptr(), x2d.data_ptr(), wk.data_ptr(), *tail)
            else:
                hip.conv3x3(d, xd.data_ptr(), wk.data_ptr(), *tail)
            torch.cuda.synchronize()
        finally:
            hip.set_igemm_variant(-1)
        if cin2:
            ins.append(wk)
    close(rows_to_5d(out, b, cout, f, Ho, Wo), ref)
    check_all(*outs, *ins)


@pytest.mark.parametrize("variant", [1, 2, 5, 6, 8, 9])
@pytest.mark.parametrize("split", [1, 2])
def test_conv3x3_dup_rows(hiplib, variant, split):
    """rcdm_conv3x3_desc.dup_rows (the shared CFG prefix): the copy dup_rows = M + 3 further down is bit-identical and the
    three rows between the two images of the output stay untouched."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(6)
    n_img, H, W, cin, cout = 3, 10, 10, 64, 320
    M = n_img * H * W
    x = h16(torch.randn(1, cin, n_img, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=g)
    ref = O.conv_frames(x, w, bias, stride=1, padding=1)
    lda, ldc = cin + 8, cout + 8
    xd, w32, bd = rows_from_5d(x, lda), gvec(w), gvec(bias)
    wp = gout(cout, 9 * cin)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    out = gout(2 * M + 3, cout, ldc)
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, lda, ldc, 0, hip.EPI_BIAS, 1, 0, 1.0, split, 0, M + 3)
    hip.set_igemm_variant(variant)
    try:
        wsb = ws(hip.conv3x3_workspace_bytes(d))
        hip.conv3x3(d, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), wsb.data_ptr(), wsb.numel())
        torch.cuda.synchronize()
    finally:
        hip.set_igemm_variant(-1)
    close(rows_to_5d(out[:M], 1, cout, n_img, H, W), ref)
    assert torch.equal(out[:M, :cout], out[M + 3:, :cout]), "the duplicate rows differ"
    assert torch.isnan(out[M:M + 3].float()).all(), "the rows between the two copies were written"
    check_all(out, wp, xd, w32, bd)


@pytest.mark.parametrize("n_img,H,W,cin,cout", [(3, 6, 10, 72, 40), (2, 16, 16, 128, 128)])
def test_conv3x3_pad_after_only(hiplib, n_img, H, W, cin, cout):
    """pad_after_only = 1 (F.pad(x, (0, 1, 0, 1)) + a stride-2 conv without padding, the VAE encoder's downsampler) with padded
    row strides; an odd side is refused (rcdm.h: even h_in and w_in)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(60 + cin)
    x = h16(torch.randn(1, cin, n_img, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=g)
    ref = O.conv_frames(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2, padding=0)
    Ho, Wo = ref.shape[-2:]
    assert (Ho, Wo) == (H // 2, W // 2)
    lda, ldc = cin + 8, cout + 24
    xd, w32, bd = rows_from_5d(x, lda), gvec(w), gvec(bias)
    wp = gout(cout, 9 * cin)
    hip.pack_conv3x3(w32.data_ptr(), cout, cin, cin, wp.data_ptr())
    out = gout(n_img * Ho * Wo, cout, ldc)
    d = hip.ConvDesc(n_img, H, W, cin, cout, 2, 0, lda, ldc, 0, hip.EPI_BIAS, 1, 0, 1.0, 1, 1)
    wsb = ws(hip.conv3x3_workspace_bytes(d))
    hip.conv3x3(d, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), wsb.data_ptr(), wsb.numel())
    torch.cuda.synchronize()
    close(rows_to_5d(out, 1, cout, n_img, Ho, Wo), ref)
    check_all(out, wp, xd, w32, bd)
    for h_odd, w_odd in ((H + 1, W), (H, W + 1)):
        bad = hip.ConvDesc(n_img, h_odd, w_odd, cin, cout, 2, 0, lda, ldc, 0, hip.EPI_BIAS, 1, 0, 1.0, 1, 1)
        with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
            hip.conv3x3(bad, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), 0, 0, out.data_ptr(), wsb.data_ptr(), wsb.numel())
    check_all(out, xd)


@pytest.mark.parametrize("n_img,H,W,cin,cout,up,with_bias", [
    (10, 64, 64, 320, 4, 0, True),      # conv_out: 320 -> 4 channels padded to 8, ten 64x64 latent images
    (3, 5, 7, 320, 4, 0, True),         # a small ragged image
    (3, 5, 7, 72, 4, 0, False),
    (3, 4, 6, 64, 64, 1, True),         # the upsampling gather into a wider buffer
])
def test_conv_taps_gather(hiplib, n_img, H, W, cin, cout, up, with_bias):
    """rcdm_gemm over nine stacked tap planes + rcdm_conv_taps_gather against the fp32 conv3x3: upsample = 0 at conv_out's
    geometry (the output channels zero-padded to 8 as the UNet program does) and upsample = 1, both with ldc > c_out."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(80 + cin + H + up)
    cp = (cout + 7) // 8 * 8
    x = h16(torch.randn(1, cin, n_img, H, W, generator=g))
    w = h16(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=g)
    xin = F.interpolate(x, scale_factor=[1.0, 2.0, 2.0], mode="nearest") if up else x
    ref = O.conv_frames(xin, w, bias if with_bias else None, stride=1, padding=1)
    wpad = torch.cat([w, torch.zeros(cp - cout, cin, 3, 3)])
    bpad = torch.cat([bias, torch.zeros(cp - cout)])
    M, lda, ldp, ldc = n_img * H * W, cin + 8, 9 * cp + 8, cp + 8
    xd, W9, bd = rows_from_5d(x, lda), gw(wpad.permute(2, 3, 0, 1).reshape(9 * cp, cin)), gvec(bpad)
    P = gout(M, 9 * cp, ldp)
    d = hip.GemmDesc(M, 9 * cp, cin, lda, ldp, 0, 0, 1, 0, 1.0, 0, 0)
    wsb = ws(hip.gemm_workspace_bytes(d))
    hip.gemm(d, xd.data_ptr(), W9.data_ptr(), 0, 0, 0, P.data_ptr(), wsb.data_ptr(), wsb.numel())
    out = gout(M << (2 * up), cp, ldc)
    hip.conv_taps_gather(P.data_ptr(), ldp, n_img, H, W, cp, up, bd.data_ptr() if with_bias else 0, out.data_ptr(), ldc)
    torch.cuda.synchronize()
    got = rows_to_5d(out, 1, cp, n_img, H << up, W << up)
    close(got[:, :cout], ref)
    if cp > cout:
        assert (got[:, cout:] == 0).all(), "the zero-padded output channels are not zero"
    check_all(out, P, xd, W9, bd)


@pytest.mark.parametrize("b,f,H,W,C,cross,silu", [
    (2, 5, 8, 8, 320, True, True),       # 320 rows per sample: the single-launch form
    (2, 3, 7, 9, 192, False, False),     # 63 rows per sample (ragged), per frame
    (1, 5, 16, 16, 64, True, True),      # 1280 rows per sample: statistics / finalize / apply
    (2, 5, 16, 16, 1920, True, True),    # cg = 60: the three-launch path at a production width
])
def test_groupnorm_padded_strides(hiplib, b, f, H, W, C, cross, silu):
    """rcdm_groupnorm_silu with poisoned ldx > C and ldy > C on the single-launch and the three-launch form."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(50 + C)
    x = h16(torch.randn(b, C, f, H, W, generator=g) * 2.0 + 0.7)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5 if cross else 1e-6
    if cross:
        ref = O.group_norm_cross_frame(x, gamma, beta, 32, eps)
    else:
        x4 = x.permute(0, 2, 1, 3, 4).reshape(b * f, C, H, W)
        ref = O.group_norm_per_frame(x4, gamma, beta, 32, eps).reshape(b, f, C, H, W).permute(0, 2, 1, 3, 4)
    if silu:
        ref = F.silu(ref)
    ldx, ldy = C + 8, C + 24
    xd = rows_from_5d(x, ldx)
    y = gout(b * f * H * W, C, ldy)
    samples, rps = (b, f * H * W) if cross else (b * f, H * W)
    d = hip.GroupNormDesc(samples, rps, C, 32, ldx, ldy, eps, int(silu))
    w = ws(hip.groupnorm_workspace_bytes(d))
    gd, bd = gvec(gamma), gvec(beta)
    hip.groupnorm_silu(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    close(rows_to_5d(y, b, C, f, H, W), ref)
    check_all(y, xd, gd, bd)


GN_PARTS = [
    # samples, rows per sample, C, groups
    (3, 315, 72, 4),        # ragged rows, cg = 18
    (2, 640, 320, 32),      # cross-frame norm of an 8x8-level ResNet block (5 frames x 128 ... rows), cg = 10
    (10, 256, 1280, 32),    # per-frame norm at the 16x16 level, cg = 40
    (1, 4100, 64, 32),      # one long sample, cg = 2
]


def _stat_bound(got, ref64, ref32, what, case):
    """|kernel - fp64| against eight times the error of the plain torch fp32 evaluation of the same statistic (the factor: the
    kernel's different but fixed order of additions)."""
    err = (got.double() - ref64).abs().max().item()
    yard = (ref32.double() - ref64).abs().max().item()
    print(f"groupnorm {what} {case}: kernel max abs err {err:.3e}, torch fp32 yardstick {yard:.3e}, bound {8 * yard:.3e}")
    assert err <= 8 * yard, f"{what}: {err:.3e} > 8 x {yard:.3e}"


@pytest.mark.parametrize("samples,rps,C,groups", GN_PARTS)
def test_groupnorm_stats_alone(hiplib, samples, rps, C, groups):
    """rcdm_groupnorm_stats on its own against fp64, rows at a poisoned ldx > C; (mean, rstd) within 8x the error of torch's
    fp32 evaluation of the same statistics."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(70 + C + rps)
    x = (torch.randn(samples * rps, C, generator=g) * 2.0 + 0.7).half()
    eps, ldx = 1e-5, C + 8
    xd = gin(x, ldx)
    stat = gout(1, samples * groups * 2, dtype=torch.float32, guard_rows=1)
    d = hip.GroupNormDesc(samples, rps, C, groups, ldx, C, eps, 0)
    w = ws(hip.groupnorm_workspace_bytes(d))
    hip.groupnorm_stats(d, xd.data_ptr(), stat.data_ptr(), w.data_ptr(), w.numel())
    torch.cuda.synchronize()
    got = stat.cpu().reshape(samples, groups, 2)
    assert torch.isfinite(got).all()
    m64, r64 = _gn_rows(x, samples, rps, C, groups, eps)
    m32, r32 = _gn_rows(x, samples, rps, C, groups, eps, torch.float32)
    check_all(stat, xd)
    _stat_bound(got[..., 0], m64, m32, "stats mean", (samples, rps, C, groups))
    _stat_bound(got[..., 1], r64, r32, "stats rstd", (samples, rps, C, groups))


@pytest.mark.parametrize("samples,rps,C,groups", GN_PARTS)
@pytest.mark.parametrize("splits", [3, 7])
def test_groupnorm_finalize_alone(hiplib, samples, rps, C, groups, splits):
    """rcdm_groupnorm_finalize on its own: (count, mean, M2) partials of uneven row slices, formed in fp64 and rounded to fp32,
    against the fp64 combination of those fp32 values; the yardstick is the same combination evaluated by torch in fp32."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(71 + C + rps)
    x = (torch.randn(samples, rps, groups, C // groups, generator=g) * 2.0 + 0.7).half().double()
    eps = 1e-5
    cuts = [0] + [min(rps, (i + 1) * (rps // splits) + (3 if i % 2 == 0 and splits > 1 else 0)) for i in range(splits - 1)] + [rps]
    part = torch.empty(samples, groups, splits, 3, dtype=torch.float64)
    for i in range(splits):
        v = x[:, cuts[i]:cuts[i + 1]]
        mu = v.mean(dim=(1, 3))
        part[:, :, i, 0] = v.shape[1] * v.shape[3]
        part[:, :, i, 1] = mu
        part[:, :, i, 2] = (v - mu[:, None, :, None]).pow(2).sum(dim=(1, 3))
    part = part.float()

    def combine(p):
        n, mu, m2 = p[..., 0], p[..., 1], p[..., 2]
        tot = n.sum(-1)
        mean = (n * mu).sum(-1) / tot
        var = (m2 + n * (mu - mean[..., None]).pow(2)).sum(-1) / tot
        return mean, (var + eps).rsqrt()

    (m64, r64), (m32, r32) = combine(part.double()), combine(part)
    pd = gvec(part)
    stat = gout(1, samples * groups * 2, dtype=torch.float32, guard_rows=1)
    hip.groupnorm_finalize(samples, groups, splits, eps, pd.data_ptr(), stat.data_ptr())
    torch.cuda.synchronize()
    got = stat.cpu().reshape(samples, groups, 2)
    assert torch.isfinite(got).all()
    check_all(stat, pd)
    _stat_bound(got[..., 0], m64, m32, "finalize mean", (samples, rps, C, groups, splits))
    _stat_bound(got[..., 1], r64, r32, "finalize rstd", (samples, rps, C, groups, splits))


@pytest.mark.parametrize("samples,rps,C,groups", GN_PARTS)
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_apply_alone(hiplib, samples, rps, C, groups, silu):
    """rcdm_groupnorm_apply on its own: final (mean, rstd) pairs handed in, rows at poisoned ldx > C, output at ldy > C, against
    the fp64 normalisation with those pairs."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(72 + C + rps)
    x = (torch.randn(samples * rps, C, generator=g) * 2.0 + 0.7).half()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps, ldx, ldy = 1e-5, C + 8, C + 24
    m64, r64 = _gn_rows(x, samples, rps, C, groups, eps)
    st = torch.stack([m64, r64], dim=-1).float()
    v = x.double().reshape(samples, rps, groups, C // groups)
    ref = (v - st[..., 0].double()[:, None, :, None]) * st[..., 1].double()[:, None, :, None]
    ref = ref.reshape(samples * rps, C) * gamma.double() + beta.double()
    if silu:
        ref = F.silu(ref)
    xd, sd, gd, bd = gin(x, ldx), gvec(st), gvec(gamma), gvec(beta)
    y = gout(samples * rps, C, ldy)
    d = hip.GroupNormDesc(samples, rps, C, groups, ldx, ldy, eps, silu)
    hip.groupnorm_apply(d, xd.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    close(y[:, :C], ref)
    check_all(y, xd, sd, gd, bd)


@pytest.mark.parametrize("M,C,pe", [(33, 64, False), (97, 768, False), (10, 1280, True), (2051, 320, False), (1, 200, False),
                                    (20, 1000, True), (970, 2048, False)])
def test_layernorm_padded_strides(hiplib, M, C, pe):
    """rcdm_layernorm with poisoned ldx > C and ldy > C: a row statistic that runs into the pad columns shows."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(12 + C)
    frames, rpf = 5, 2
    x = h16(torch.randn(M, C, generator=g) * 3 + 1)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    table = O.sinusoid_table(C, frames)
    if pe:
        ref = ref + table[(torch.arange(M) // rpf) % frames]
    ldx, ldy = C + 8, C + 24
    xd = gin(x.half(), ldx)
    y = gout(M, C, ldy)
    d = hip.LayerNormDesc(M, C, ldx, ldy, 1e-5, rpf, frames)
    gd, bd, td = gvec(gamma), gvec(beta), gvec(table)
    hip.layernorm(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), td.data_ptr() if pe else 0, y.data_ptr())
    torch.cuda.synchronize()
    close(y[:, :C], ref)
    check_all(y, xd, gd, bd, td)


@pytest.mark.parametrize("batch,heads,Lq,Lk,d", [
    (2, 8, 200, 85, 40),     # ragged query and key tiles
    (3, 8, 64, 91, 80),
    (1, 8, 130, 130, 160),
    (2, 4, 96, 85, 8),
    (1, 2, 70, 77, 16),
    (1, 2, 67, 70, 32),
])
def test_flash_attn_padded_strides(hiplib, batch, heads, Lq, Lk, d):
    """rcdm_flash_attn with q, k, v and the output each in a buffer of its own wider than heads * d: beside the LAST head lies
    poison (NaN in the output), not the next head."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(4 + Lq + Lk + d)
    C = heads * d
    q = h16(torch.randn(batch, Lq, C, generator=g))
    k = h16(torch.randn(batch, Lk, C, generator=g))
    v = h16(torch.randn(batch, Lk, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    ldq, ldk, ldv, ldo = C + 8, C + 16, C + 24, C + 32
    qd, kd, vd = gin(q.reshape(-1, C).half(), ldq), gin(k.reshape(-1, C).half(), ldk), gin(v.reshape(-1, C).half(), ldv)
    out = gout(batch * Lq, C, ldo)
    desc = hip.AttnDesc(batch, heads, Lq, Lk, d, ldq, ldk, ldv, ldo, d ** -0.5)
    hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    close(out[:, :C].reshape(batch, Lq, C), ref)
    check_all(out, qd, kd, vd)


@pytest.mark.parametrize("batch,heads,L,d,causal,pad", [
    (2, 4, 97, 64, True, True),
    (3, 2, 150, 40, False, True),
    (1, 2, 70, 160, True, False),
])
def test_flash_attn_masked_padded_strides(hiplib, batch, heads, L, d, causal, pad):
    """rcdm_flash_attn_masked with every row stride wider than heads * d, the pad columns poisoned."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(6 + L + d)
    C = heads * d
    q, k, v = (h16(torch.randn(batch, L, C, generator=g)) for _ in range(3))
    valid = torch.ones(batch, L, dtype=torch.uint8)
    if pad:
        for b in range(batch):
            valid[b, 20 + 7 * b:L - 6] = 0
    add = (1.0 - valid.float())[:, None, :] * -10000.0
    add = add + torch.full((L, L), -10000.0).triu_(1)[None] if causal else add.expand(batch, L, L)
    ref = O.attention_core(q, k, v, heads, mask=add)
    ldq, ldk, ldv, ldo = C + 8, C + 16, C + 24, C + 32
    qd, kd, vd = gin(q.reshape(-1, C).half(), ldq), gin(k.reshape(-1, C).half(), ldk), gin(v.reshape(-1, C).half(), ldv)
    vm = valid.to(DEV)
    out = gout(batch * L, C, ldo)
    desc = hip.AttnDesc(batch, heads, L, L, d, ldq, ldk, ldv, ldo, d ** -0.5)
    hip.flash_attn_masked(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), vm.data_ptr() if pad else 0, causal, out.data_ptr())
    torch.cuda.synchronize()
    close(out[:, :C].reshape(batch, L, C), ref)
    check_all(out, qd, kd, vd)


@pytest.mark.parametrize("b,frames,pixels,heads,d", [(2, 5, 64, 8, 40), (1, 5, 16, 8, 160), (2, 5, 33, 8, 8), (1, 3, 20, 4, 16)])
def test_temporal_attn_padded_strides(hiplib, b, frames, pixels, heads, d):
    """rcdm_temporal_attn with ldqkv > 3 C and ldo > C: beside v's last head lies poison."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(18 + pixels + d)
    C = heads * d
    qkv = h16(torch.randn(b * frames * pixels, 3 * C, generator=g))
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]

    def regroup(x):
        return x.reshape(b, frames, pixels, C).permute(0, 2, 1, 3).reshape(b * pixels, frames, C)

    o = O.attention_core(regroup(q), regroup(k), regroup(v), heads)
    ref = o.reshape(b, pixels, frames, C).permute(0, 2, 1, 3).reshape(b * frames * pixels, C)
    ldqkv, ldo = 3 * C + 8, C + 24
    out = gout(b * frames * pixels, C, ldo)
    desc = hip.TemporalAttnDesc(b, frames, pixels, heads, d, ldqkv, ldo, d ** -0.5)
    qkv_d = gin(qkv.half(), ldqkv)
    hip.temporal_attn(desc, qkv_d.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    close(out[:, :C], ref)
    check_all(out, qkv_d)


@pytest.mark.parametrize("N", [8, 72, 1000, 4096])
@pytest.mark.parametrize("M", [1, 130])
@pytest.mark.parametrize("scale", [0.25, 1.0])
def test_softmax_rows_padded(hiplib, M, N, scale):
    """rcdm_softmax_rows against fp64 on the f16-rounded logits, ldx > N (poisoned) and ldy > N; row 0 has a single
    dominant logit.  Tolerance of tests/test_vae.py test_softmax_rows."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(9 + M + N)
    x = (torch.randn(M, N, generator=g) * 3).half()
    x[0, N // 3] = 60.0
    want = torch.softmax(x.double() * scale, dim=-1)
    ldx, ldy = N + 8, N + 16
    xd = gin(x, ldx)
    y = gout(M, N, ldy)
    hip.softmax_rows(M, N, ldx, ldy, scale, xd.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    got = y[:, :N].float().cpu()
    assert torch.isfinite(got).all(), "non-finite output"
    assert torch.allclose(got.double(), want, rtol=2e-3, atol=1e-6), (got.double() - want).abs().max()
    check_all(y, xd)


@pytest.mark.parametrize("rows", [1, 8])
def test_timestep_embed_and_small_linear_rows(hiplib, rows):
    """rcdm_timestep_embed and rcdm_small_linear at 1 and 8 rows, guarded outputs (fp32 against fp64 of the f16 weights)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(3 + rows)
    t = torch.linspace(1.0, 981.0, rows)
    ref = O.timestep_embedding(t, 320)
    out = gout(rows, 320, dtype=torch.float32)
    t_d = gvec(t)
    hip.timestep_embed(t_d.data_ptr(), rows, 320, out.data_ptr())
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and (out.cpu() - ref).abs().max() < 2e-4
    W1 = h16(torch.randn(200, 320, generator=g) * 0.05)
    b1 = torch.randn(200, generator=g)
    ref2 = F.silu(F.linear(F.silu(out.cpu().double()), W1.double(), b1.double()))
    o2 = gout(rows, 200, dtype=torch.float32)
    W1d, b1d = gw(W1), gvec(b1)
    hip.small_linear(out.data_ptr(), rows, 320, W1d.data_ptr(), b1d.data_ptr(), 200, 1, 1, o2.data_ptr())
    torch.cuda.synchronize()
    close(o2, ref2, rel=1e-3, abs_frac=1e-3)
    check_all(out, o2, t_d, W1d, b1d)


def test_converters_into_wider_rows(hiplib):
    """rcdm_assemble_input / rcdm_ncfhw_to_rows into rows with ld > c_pad: the columns C..c_pad are zero, the columns
    c_pad..ld untouched; rcdm_rows_to_ncfhw reads such rows back."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(9)
    S, f, H, W = 2, 3, 5, 7
    lat = torch.randn(S, 4, f, H, W, generator=g)
    mask = (torch.rand(2 * S, 1, f, H, W, generator=g) > 0.5).float()
    masked = torch.randn(2 * S, 4, f, H, W, generator=g)
    ref_in = torch.cat([torch.cat([lat] * 2), mask, masked], dim=1)
    rows = gout(2 * S * f * H * W, 16, 40)
    lat0, mask_d, masked_d = gvec(lat), gvec(mask), gvec(masked)
    hip.assemble_input(lat0.data_ptr(), mask_d.data_ptr(), masked_d.data_ptr(), S, 2, f, H, W, rows.data_ptr(), 40, 16)
    torch.cuda.synchronize()
    close(rows_to_5d(rows, 2 * S, 9, f, H, W), ref_in, rel=1e-3, abs_frac=1e-3)
    assert (rows[:, 9:16] == 0).all()
    check_all(rows, lat0, mask_d, masked_d)
    x = torch.randn(3, 9, f, H, W, generator=g)
    r2 = gout(3 * f * H * W, 16, 32)
    x_d = gvec(x)
    hip.ncfhw_to_rows(x_d.data_ptr(), 3, 9, f, H, W, r2.data_ptr(), 32, 16)
    torch.cuda.synchronize()
    assert torch.equal(rows_to_5d(r2, 3, 9, f, H, W), x.half().float()) and (r2[:, 9:16] == 0).all()
    check_all(r2, x_d)
    src = rows_from_5d(x, 32)           # poison beyond the 9 channels
    back_h = gout(1, x.numel(), dtype=torch.float32, guard_rows=1)
    hip.rows_to_ncfhw(src.data_ptr(), 32, 3, 9, f, H, W, back_h.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(back_h.view(x.shape).cpu(), x.half().float())
    check_all(back_h, src)


@pytest.mark.parametrize("reps,with_noise,clip", [(2, True, 10.0), (1, False, 0.0)])
def test_cfg_unclip_step_padded_rows(hiplib, reps, with_noise, clip):
    """rcdm_cfg_unclip_step reading f16 prediction rows with ld > E, poison beyond the E used columns, against the formula
    of rcdm.h in fp64; the state sits between guard bands."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(14 + reps)
    n, E, ld, gs, steps, st = 3, 72, 88, 4.0, 4, 2
    pred = (torch.randn(reps * n, E, generator=g) * 6).half()
    lat = torch.randn(n, E, generator=g)
    coef = torch.rand(steps, 3, generator=g) + 0.1
    noise = torch.randn(steps, n, E, generator=g)
    p = pred.double()
    x0 = p[:n] + gs * (p[n:] - p[:n]) if reps == 2 else p
    if clip > 0:
        x0 = x0.clamp(-clip, clip)
    c = coef.double()[st]
    ref = c[0] * x0 + c[1] * lat.double() + (c[2] * noise[st].double() if with_noise else 0.0)
    pd, cd, nd = gin(pred, ld), gvec(coef), gvec(noise)
    lat_h = gout(1, n * E, dtype=torch.float32, guard_rows=1)
    lat_h[0].copy_(lat.reshape(-1))
    step = torch.tensor([st], dtype=torch.int32, device=DEV)
    hip.cfg_unclip_step(pd.data_ptr(), ld, lat_h.data_ptr(), n, reps, E, gs, clip, cd.data_ptr(), nd.data_ptr() if with_noise else 0,
                        step.data_ptr())
    torch.cuda.synchronize()
    got = lat_h[0].cpu().double().reshape(n, E)
    assert (got - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    check_all(lat_h, pd, cd, nd)
