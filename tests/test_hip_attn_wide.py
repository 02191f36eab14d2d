"""rcdm_flash_attn at head dims 160 < d <= 512 (csrc/attn_wide.hip: the one 512-channel head of the SD-1.5 VAE mid block)
against oracle.unet_oracle.attention_core in fp32 on the same f16-rounded inputs, at the tolerance of every other head dim
(`close` of tests/test_hip_kernels.py, unchanged)."""
import pytest
import torch

from oracle import unet_oracle as O
from tests.guard import check_all
from tests.test_hip_kernels import DEV, close, gin, gout, h16

pytestmark = pytest.mark.gpu


def _run(hip, q, k, v, heads, d, flags=0):
    """q inside a 3C-wide [q|k|v]-style buffer, k | v interleaved in one 2C-wide buffer (as test_flash_attn lays them out)."""
    batch, Lq, C = q.shape
    Lk = k.shape[1]
    qd = gin(q.reshape(-1, C).half(), 3 * C)
    kv = gin(torch.cat([k.reshape(-1, C), v.reshape(-1, C)], dim=1).half(), 2 * C + 8)
    out = gout(batch * Lq, C, C + 8)
    desc = hip.AttnDesc(batch, heads, Lq, Lk, d, 3 * C, 2 * C + 8, 2 * C + 8, C + 8, d ** -0.5, flags)
    hip.flash_attn(desc, qd.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, qd, kv)
    return out[:, :C].reshape(batch, Lq, C)


@pytest.mark.parametrize("batch,heads,Lq,Lk,d", [
    (1, 1, 4096, 4096, 512),   # the VAE mid block of a 512 x 512 image
    (2, 1, 6144, 6144, 512),   # 512 x 768: past the score-buffer form's limit
    (1, 1, 1000, 777, 512),    # ragged last query block and key tile
    (1, 1, 16, 16, 512),       # half a key tile
    (1, 1, 1, 1, 512),         # a single key: output == V row
    (3, 2, 130, 200, 256),
    (1, 1, 300, 300, 320),
])
def test_flash_attn_wide(hiplib, batch, heads, Lq, Lk, d):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(7 + Lq + Lk + d)
    C = heads * d
    q = h16(torch.randn(batch, Lq, C, generator=g))
    k = h16(torch.randn(batch, Lk, C, generator=g))
    v = h16(torch.randn(batch, Lk, C, generator=g))
    ref = O.attention_core(q, k, v, heads)
    got = _run(hip, q, k, v, heads, d)
    print(f"d = {d} Lq = {Lq} Lk = {Lk}: max abs err {(got.float().cpu() - ref).abs().max().item():.3e} (ref max {ref.abs().max().item():.3f})")
    close(got, ref)          # measured max abs err 4e-4 .. 7e-4 of max|ref| (8.5e-5 of 0.17 at 4096 x 4096 x 512; 0 at a single key)


@pytest.mark.parametrize("d", [512, 256])
def test_flash_attn_wide_forced_rescale(hiplib, d):
    """A key in a LATE tile dominates one query: its softmax reference (the first key tile's max) is off by far more than
    the f16 range of P, which the kernel must notice and repair (modelled on test_flash_attn_forced_rescale)."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(21)
    L = 256
    q = h16(torch.randn(1, L, d, generator=g))
    k = h16(torch.randn(1, L, d, generator=g))
    v = h16(torch.randn(1, L, d, generator=g))
    k[0, 200] = h16(q[0, 17] * 4.0)      # spike in the 7th key tile for query 17: scaled score ~ 4 |q|^2 / sqrt(d) ~ 90
    k[0, 77] = h16(q[0, 140] * 1.5)      # a second, smaller one (~ 34) in another wave's queries and another tile
    ref = O.attention_core(q, k, v, 1)
    got = _run(hip, q, k, v, 1, d)
    close(got, ref)
    # the spiked queries reproduce (nearly) the V row of their dominant key: the late tile was weighted in, not lost
    assert (got[0, 17].float().cpu() - v[0, 200]).abs().max() < 2e-2


@pytest.mark.parametrize("d,L", [(512, 256), (320, 200), (192, 96)])
def test_flash_attn_wide_large_logits(hiplib, d, L):
    """|scale log2(e) q.k| in the several hundreds (a nearly one-hot softmax): finite output at the ordinary tolerance, with
    and without RCDM_ATTN_WIDE_RANGE (modelled on test_flash_attn_large_logits_all_head_dims)."""
    from rcdms_amd import hip
    gain = 48.0
    gq = torch.Generator().manual_seed(5 + d)
    q = h16(torch.randn(2, L, d, generator=gq) * gain ** 0.5)
    k = h16(torch.randn(2, L, d, generator=gq) * gain ** 0.5)
    v = h16(torch.randn(2, L, d, generator=gq))
    ref = O.attention_core(q, k, v, 1)
    smax = (torch.einsum("bld,bmd->blm", q, k).abs().max() * d ** -0.5 * 1.4427).item()
    assert smax >= 200.0, smax
    for flags in (hip.ATTN_WIDE_RANGE, 0):
        got = _run(hip, q, k, v, 1, d, flags).float().cpu()
        assert torch.isfinite(got).all()
        print(f"d = {d}, flags {flags}: max |scaled score| {smax:.0f}, max abs err {(got - ref).abs().max().item():.3e}")
        close(got, ref, rel=2e-3, abs_frac=4e-3)


def test_flash_attn_wide_shape_errors(hiplib):
    """Still RCDM_ESHAPE: a masked or causal call above d = 160, d > 512, d % 64 != 0 above 160."""
    from rcdms_amd import hip
    L = 64
    buf = gin(torch.randn(L, 3 * 576, generator=torch.Generator().manual_seed(1)).half())
    out = gout(L, 512)                           # the one real launch below writes exactly these rows
    scratch = gout(L, 576)                       # handed to the refused calls only: must stay untouched
    valid = torch.ones(1, L, dtype=torch.uint8, device=DEV)

    def desc(d):
        return hip.AttnDesc(1, 1, L, L, d, 3 * d, 3 * d, 3 * d, d, d ** -0.5)

    def ptrs(d):
        return buf.data_ptr(), buf.data_ptr() + 2 * d, buf.data_ptr() + 4 * d

    with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
        hip.flash_attn_masked(desc(512), *ptrs(512), valid.data_ptr(), False, scratch.data_ptr())
    with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
        hip.flash_attn_masked(desc(512), *ptrs(512), 0, True, scratch.data_ptr())
    for d in (576, 200):
        with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
            hip.flash_attn(desc(d), *ptrs(d), scratch.data_ptr())
    # ... and the unmasked entry of the masked symbol is the same call as rcdm_flash_attn
    hip.flash_attn_masked(desc(512), *ptrs(512), 0, False, out.data_ptr())
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    check_all(out, scratch, buf)
    assert torch.isnan(scratch.float()).all(), "a refused call wrote its output"


def test_flash_attn_wide_graph_capture(hiplib):
    """Capturable on the caller's stream: a replayed graph writes the bits of the eager call."""
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(11)
    L, d = 384, 512
    qkv = gin((torch.randn(L, 3 * d, generator=g)).half())
    out_e = gout(L, d)
    out_g = gout(L, d)
    desc = hip.AttnDesc(1, 1, L, L, d, 3 * d, 3 * d, 3 * d, d, d ** -0.5)
    hip.flash_attn(desc, qkv.data_ptr(), qkv.data_ptr() + 2 * d, qkv.data_ptr() + 4 * d, out_e.data_ptr())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.flash_attn(desc, qkv.data_ptr(), qkv.data_ptr() + 2 * d, qkv.data_ptr() + 4 * d, out_g.data_ptr())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_e, out_g) and out_e.float().abs().max() > 0
    check_all(out_e, out_g, qkv)
