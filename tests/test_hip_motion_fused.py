"""GPU: the temporal attention as the tail of the q | k | v row chain (rcdm_rowchain tail 4, rowff.hip) against the two-launch
form it replaces (rcdm_rowchain tail 3 -> rcdm_temporal_attn) on the same inputs and weights, and both against the fp32
arithmetic of the reference (tests/test_hip_rowff.py _chain_reference for proj_in / to_out -> LayerNorm (+ pe) -> q | k | v,
oracle.unet_oracle.attention_core over the five frames of every pixel, motion_module.py:299-302).

What differs between the two forms, by construction: q, k and v are the same f16 bits (the tail-3 chain's roundings), the
softmax is the arithmetic of temporal_attn_kernel, p v is accumulated over the frames in the same order and rounded to f16
once — but the 40 products of a score are summed per 8-channel piece and then across four lanes instead of in one chain of 40
fmas.  That moves a score by a few fp32 ulps (relative 1e-6 of the largest |q k| term), i.e. an output by far less than
an f16 ulp of the largest output: it can flip the final f16 rounding of an element, nothing more.  So the forms are not
bit-identical (measured on MI355X: 34 - 80 of 51 200 - 153 600 outputs differ, each by one f16 ulp; rel-RMS against the
fp32 reference 3.35e-4 ... 3.64e-4 for BOTH forms, 5.0e-4 / 5.1e-4 with the +-30 scores), and the
test asserts

  * rel-RMS(fused, oracle) <= rel-RMS(two-launch, oracle) + MARGIN, the two-launch figure measured here on the same inputs.
    MARGIN = 2^-11 / sqrt(3) = 2.8e-4 is the rel-RMS of ONE f16 rounding of ao (uniform error of at most half an ulp,
    2^-11 relative): the most a set of flipped final roundings can add.  Where a head's scores are pushed to +-30 both forms
    sit far from the fp32 oracle for the same reason (q and k are f16: 30 * 2^-11 of score error is 1.5 % of a probability),
    which is why the bound is relative to the two-launch form and not a figure of its own;
  * |fused - two-launch| <= 2^-10 * max|two-launch| + 2^-10 * |two-launch| elementwise: one f16 ulp at the element's or
    the tensor's scale (the absolute error of an element is a sum over five frames of v);
  * at ordinary scores, both forms within the kernel suite's tolerance of the oracle (tests/test_hip_kernels.py close());
  * the token rows bit-identical to the two-launch form's (stage A and its stores are the same code, the row map differs).
Buffers are guarded (tests/guard.py): row strides above C, poisoned pad columns and guard rows on the way in, NaN on the way
out, all asserted untouched."""
import pytest
import torch

from oracle import unet_oracle as O
from tests.guard import check_all, check_out, check_written
from tests.test_hip_kernels import DEV, close, gin, gout, gvec, h16
from tests.test_hip_rowff import _chain_reference, _chain_weights, _dev

pytestmark = pytest.mark.gpu

C, F, HEADS, D, G = 320, 5, 8, 40, 32
MARGIN = 2.0 ** -11 / 3.0 ** 0.5


def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _oracle_attention(qkv, b, hw):
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]

    def regroup(x):  # "(b f) d c -> (b d) f c"  motion_module.py:299
        return x.reshape(b, F, hw, C).permute(0, 2, 1, 3).reshape(b * hw, F, C)

    o = O.attention_core(regroup(q), regroup(k), regroup(v), HEADS)
    return o.reshape(b, hw, F, C).permute(0, 2, 1, 3).reshape(b * F * hw, C)


def _group_norm_rows(x, gn_g, gn_b, n_img, hw):
    xs = x.view(n_img, hw, G, C // G)
    mean = xs.mean(dim=(1, 3), keepdim=True)
    var = xs.var(dim=(1, 3), unbiased=False, keepdim=True)
    return h16(((xs - mean) / torch.sqrt(var + 1e-6)).reshape(-1, C) * gn_g + gn_b)


def _launch(tail, a16, res16, tok, out, dev, ws, M, hw, gn=None):
    from rcdms_amd import hip
    d = hip.RowChainDesc(M, C, a16.stride(0), res16.stride(0) if res16 is not None else 0, tok.stride(0), out.stride(0), tail,
                         hw, F, 1e-5, G if gn else 0, hw if gn else 0)
    hip.rowchain(d, a16.data_ptr(), res16.data_ptr() if res16 is not None else 0, tok.data_ptr(), dev["ba"].data_ptr(),
                 dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(), dev["pe"].data_ptr() if dev["pe"] is not None else 0,
                 ws.data_ptr(), 0, 0, out.data_ptr(),
                 gn_stat=gn[0].data_ptr() if gn else 0, gn_g=gn[1].data_ptr() if gn else 0, gn_b=gn[2].data_ptr() if gn else 0)


def _packed(dev, tail):
    from rcdms_amd import hip
    ws = gout(1, hip.rowchain_stream_bytes(C, tail), dtype=torch.uint8, guard_rows=1)
    hip.pack_rowchain(dev["wa"].data_ptr(), C, tail, dev["wt"].data_ptr(), 0, 0, 0, ws.data_ptr(), 0)
    return ws


def _case(b, hw, site, pe, big=False):
    """site 0: chains[0] of a motion module (GroupNorm prologue on the raw rows, no residual, tok and out on their own);
    site 1: chains[1] (a_in = the previous attention's output, residual = tok written in place, out over a_in).  big: head 3's
    scores scaled to +-30, head 5's keys equal in every frame (zero to_k rows: a uniform softmax)."""
    from rcdms_amd import hip
    M = b * F * hw
    assert hip.rowchain_config_supported(C, 4, F if pe else 0)
    w, g = _chain_weights(C, 3, F if pe else 0, 4000 + 10 * hw + b + 100 * site + (1000 if big else 0))
    if big:
        w["wt"][3 * D:4 * D] *= 25.0                    # q of head 3: scores ~ N(0, 1.2) * 25
        w["wt"][C + 5 * D:C + 6 * D] = 0.0              # k of head 5
        w["wt"] = h16(w["wt"])
    x = h16(torch.randn(M, C, generator=g) * (2.0 if site == 0 else 1.0) + (0.5 if site == 0 else 0.0))
    res = h16(torch.randn(M, C, generator=g) * 1.5) if site == 1 else None
    dev = _dev(w)
    lda, ldt, ldq = C + 24, C + 32, 3 * C + 16

    # ---- fp32 reference
    if site == 0:
        gn_g, gn_b = (1.0 + 0.2 * torch.randn(C, generator=g)).float(), (0.3 * torch.randn(C, generator=g)).float()
        a_ref = _group_norm_rows(x, gn_g, gn_b, b * F, hw)
    else:
        a_ref = x
    tok_ref, qkv_ref = _chain_reference(a_ref, res, w, 3, hw)
    ao_ref = _oracle_attention(qkv_ref, b, hw)

    # ---- two launches: tail 3 (on normalised rows: the prologue form of tail 3 needs 160 rows per sample and is shown
    # bit-identical to this in tests/test_hip_rowff.py), then rcdm_temporal_attn
    x16 = gin(x.half(), lda)
    gn = None
    if site == 0:
        gd = hip.GroupNormDesc(b * F, hw, C, G, lda, lda, 1e-6, 0)
        gws = torch.full((max(hip.groupnorm_workspace_bytes(gd), 16),), 0xFF, dtype=torch.uint8, device=DEV)
        gg, gb = gvec(gn_g), gvec(gn_b)
        a16 = gout(M, C, lda)
        hip.groupnorm_silu(gd, x16.data_ptr(), gg.data_ptr(), gb.data_ptr(), a16.data_ptr(), gws.data_ptr(), gws.numel())
        stat = gout(1, b * F * G * 2, dtype=torch.float32, guard_rows=1)
        hip.groupnorm_stats(gd, x16.data_ptr(), stat.data_ptr(), gws.data_ptr(), gws.numel())
        gn = (stat, gg, gb)
    else:
        a16 = x16
    res16 = gin(res.half(), ldt) if site == 1 else None
    ws3, ws4 = _packed(dev, 3), _packed(dev, 4)
    tok1, qkv1, ao1 = gout(M, C, ldt), gout(M, 3 * C, ldq), gout(M, C, lda)
    _launch(3, a16, res16, tok1, qkv1, dev, ws3, M, hw)
    hip.temporal_attn(hip.TemporalAttnDesc(b, F, hw, HEADS, D, ldq, lda, D ** -0.5), qkv1.data_ptr(), ao1.data_ptr())

    # ---- one launch
    if site == 0:
        tok2, ao2 = gout(M, C, ldt), gout(M, C, lda)
        _launch(4, x16, None, tok2, ao2, dev, ws4, M, hw, gn=gn)
    else:   # as the plan calls it: tok over the residual rows, the output over the input rows
        tok2, ao2 = gout(M, C, ldt), gout(M, C, lda)
        tok2[:, :C] = res.half().to(DEV)
        ao2[:, :C] = x.half().to(DEV)
        _launch(4, ao2, tok2, tok2, ao2, dev, ws4, M, hw)
    torch.cuda.synchronize()

    for t in (tok1, qkv1, ao1, tok2, ao2):
        check_out(t)
        check_written(t)
    check_all(ws3, ws4, x16, *([res16] if res16 is not None else []), *([a16, stat, gg, gb] if site == 0 else []),
              *(v for v in dev.values() if v is not None))
    assert torch.equal(tok1[:, :C], tok2[:, :C]), "token rows differ from the two-launch form"
    u, f = ao1[:, :C].float().cpu(), ao2[:, :C].float().cpu()
    ru, rf = rel_rms(u, ao_ref), rel_rms(f, ao_ref)
    diff = (f - u).abs()
    print(f"b={b} hw={hw} site={site} pe={int(pe)} big={int(big)}: rel-RMS vs fp32 two-launch {ru:.3e}  fused {rf:.3e}  "
          f"(margin {MARGIN:.2e});  fused vs two-launch: {int((diff > 0).sum())} / {diff.numel()} elements differ, max {diff.max():.3e} "
          f"(max|ao| {u.abs().max():.3e})")
    assert torch.isfinite(f).all()
    assert rf <= ru + MARGIN, f"fused rel-RMS {rf:.3e} vs two-launch {ru:.3e} + {MARGIN:.2e}"
    ulp = 2.0 ** -10
    bad = diff > ulp * u.abs().max() + ulp * u.abs()
    assert not bad.any(), f"{int(bad.sum())} elements further than an f16 ulp from the two-launch form, max {diff.max():.3e}"
    if not big:
        close(ao1[:, :C], ao_ref)
        close(ao2[:, :C], ao_ref)
        close(tok2[:, :C], tok_ref)


@pytest.mark.parametrize("b,hw,site,pe", [
    (1, 32, 1, True),    # exactly one full block: two pixel groups
    (1, 48, 0, True),    # three groups: the second block has one dead group of five waves
    (2, 32, 0, True),    # two blocks, one per sample: positional row and GroupNorm sample per wave
    (2, 48, 1, True),    # a block whose two groups lie in different samples
    (2, 32, 1, False),   # without the positional rows
    (1, 48, 0, False),
])
def test_fused_vs_two_launches(hiplib, b, hw, site, pe):
    _case(b, hw, site, pe)


@pytest.mark.parametrize("site", [0, 1])
def test_fused_scores_far_from_zero(hiplib, site):
    """Head 3 with scaled scores of +-30 (softmax rows that are one-hot to fp32 precision next to flat ones), head 5 with the
    same key in every frame (all five scores equal: the output is the mean of v over the frames)."""
    _case(1, 48, site, True, big=True)


def test_fused_rejects(hiplib):
    """Shapes the frame-major blocks cannot take are refused, not run: another frame count, images that are not whole
    16-pixel groups, a row count that is not whole samples, a GroupNorm sample that is not the image."""
    from rcdms_amd import hip
    assert not hip.rowchain_config_supported(C, 4, 3) and not hip.rowchain_config_supported(640, 4, 5)
    assert hip.rowchain_stream_bytes(C, 4) == hip.rowchain_stream_bytes(C, 3)
    w, g = _chain_weights(C, 3, F, 5)
    dev = _dev(w)
    ws4 = _packed(dev, 4)
    M = F * 32
    x16 = gin(h16(torch.randn(M, C, generator=g)).half())
    tok, out = gout(M, C), gout(M, C)

    def call(M_, hw, frames, gn_rows=0):
        d = hip.RowChainDesc(M_, C, C, 0, C, C, 4, hw, frames, 1e-5, G if gn_rows else 0, gn_rows)
        st = dev["ln_g"].data_ptr() if gn_rows else 0
        hip.rowchain(d, x16.data_ptr(), 0, tok.data_ptr(), dev["ba"].data_ptr(), dev["ln_g"].data_ptr(), dev["ln_b"].data_ptr(),
                     dev["pe"].data_ptr(), ws4.data_ptr(), 0, 0, out.data_ptr(), gn_stat=st, gn_g=st, gn_b=st)

    for args in ((M, 32, 4), (M, 40, 5), (M - 32, 32, 5), (M, 32, 5, 64)):
        with pytest.raises(hip.RcdmError):
            call(*args)
    torch.cuda.synchronize()
    check_all(tok, out, x16)
