"""GPU: the kernels of csrc/conv2d.hip on the guarded buffers of tests/guard.py.

  rcdm_conv2d   against a float64 convolution of the same f16 operands, per output
                    |err| <= 2^-11 |y| + K 2^-24 sum|a||w|,  K = kh kw c_in
                (one rounding to f16 of a sum of K products accumulated in fp32), through every kernel form the Inception
                network uses, with tiles that hold rows of two images, M / N / K tails, lda > c_in, a column window of a wider
                output, stride 2 on even and odd sides; small-integer operands come back bit for bit; the ReLU epilogue.
  rcdm_pool2d, rcdm_global_avgpool, rcdm_image_bilinear_rows   as include/rcdm.h defines them."""
import pytest
import torch
import torch.nn.functional as F

from tests import guard as G
from tests import inception_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

FORMS = [((3, 3), 2, (0, 0)), ((3, 3), 1, (0, 0)), ((3, 3), 1, (1, 1)), ((1, 1), 1, (0, 0)), ((5, 5), 1, (2, 2)),
         ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0)), ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))]
FORM_IDS = ["3x3s2", "3x3", "3x3p1", "1x1", "5x5p2", "1x7", "7x1", "1x3", "3x1"]
# (n_img, h, w, c_in, c_out): 3 images of 9 x 11 put rows of two images into one 64-row tile and leave an M tail, K = kh kw c_in
# is no multiple of the 32-deep k-step for any of these c_in; 1 image of 4 x 5 is less than one tile
SHAPES = [(3, 9, 11, ci, co) for ci in (8, 48, 80) for co in (8, 48, 80, 192)] + [(1, 4, 5, 8, 8), (1, 4, 5, 80, 48)]


def side(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def run_conv(hip, x, w, bias, stride, pad, epi, lda=None, ldc=None, off=0):
    """x (n, h, w, c_in) f16, w (c_out, c_in, kh, kw) f16, bias fp32 or None -> (guarded output view, its rows M, handles)."""
    n, h, wd, ci = x.shape
    co, _, kh, kw = w.shape
    ho, wo = side(h, kh, stride, pad[0]), side(wd, kw, stride, pad[1])
    M = n * ho * wo
    xv, hx = G.guarded_in(x.reshape(-1, ci), lda, device=DEV)
    wv, hw_ = G.guarded_w(w.permute(0, 2, 3, 1).reshape(co, -1).contiguous(), device=DEV)
    ldc = co + 8 if ldc is None else ldc
    ov, hout = G.guarded_out(M, ldc if off else co, ldc, device=DEV)
    handles = [hx, hw_, hout]
    bptr = 0
    if bias is not None:
        bv, hb = G.guarded_vec(bias, device=DEV)
        bptr = bv.data_ptr()
        handles.append(hb)
    d = hip.Conv2dDesc(n, h, wd, ci, co, kh, kw, stride, stride, pad[0], pad[1], xv.shape[1], ldc, epi)
    hip.conv2d(d, xv.data_ptr(), wv.data_ptr(), bptr, ov.data_ptr() + 2 * off)
    torch.cuda.synchronize()
    return ov, (n, ho, wo), handles


def reference(x, w, bias, stride, pad):
    """float64 conv of the f16 operands -> (y, sum |a||w| (+ |bias|)) as rows [M][c_out]."""
    xd, wd = x.permute(0, 3, 1, 2).double(), w.double()
    b = None if bias is None else bias.double()
    y = F.conv2d(xd, wd, b, stride=stride, padding=pad)
    s = F.conv2d(xd.abs(), wd.abs(), None if b is None else b.abs(), stride=stride, padding=pad)
    co = w.shape[0]
    return y.permute(0, 2, 3, 1).reshape(-1, co), s.permute(0, 2, 3, 1).reshape(-1, co)


def check_conv(hip, shape, form, seed, relu=True, lda_pad=8, **kw):
    n, h, wd, ci, co = shape
    (kh, kwid), stride, pad = form
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, wd, ci, generator=g).half()
    w = (torch.randn(co, ci, kh, kwid, generator=g) / (kh * kwid * ci) ** 0.5).half()
    bias = torch.randn(co, generator=g)
    epi = hip.EPI_BIAS | (hip.EPI_RELU if relu else 0)
    ov, _, handles = run_conv(hip, x, w, bias, stride, pad, epi, lda=ci + lda_pad, **kw)
    y, s = reference(x, w, bias, stride, pad)
    if relu:
        y = y.clamp_min(0.0)
    K = kh * kwid * ci
    tol = 2.0 ** -11 * y.abs() + K * 2.0 ** -24 * s
    off = kw.get("off", 0)
    got = ov[:, off:off + co].double().cpu()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} outputs never stored"
    bad = (got - y).abs() > tol
    assert not bad.any(), (shape, form, int(bad.sum()), float(((got - y).abs() / tol).max()))
    return ov, handles, float(((got - y).abs() / tol).max())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_conv2d_forms_against_float64(hiplib, form):
    from rcdms_amd import hip
    worst = 0.0
    for i, shape in enumerate(SHAPES):
        ov, handles, r = check_conv(hip, shape, form, 100 + i)
        worst = max(worst, r)
        G.check_all(*handles)
    print(f"conv2d {form}: worst |err| / bound over {len(SHAPES)} shapes {worst:.3f}")


@pytest.mark.parametrize("hw", [(10, 9), (17, 10), (9, 17)])
def test_conv2d_stride2_even_and_odd_sides(hiplib, hw):
    from rcdms_amd import hip
    assert {side(10, 3, 2, 0), side(9, 3, 2, 0)} == {4} and side(17, 3, 2, 0) == 8
    _, handles, _ = check_conv(hip, (2, hw[0], hw[1], 48, 80), ((3, 3), 2, (0, 0)), 7)
    G.check_all(*handles)


def test_conv2d_writes_only_its_column_window(hiplib):
    from rcdms_amd import hip
    for form in (FORMS[2], FORMS[3], FORMS[5]):
        ov, handles, _ = check_conv(hip, (3, 9, 11, 48, 96), form, 11, ldc=288, off=64)
        bits = ov.view(torch.int16)
        fill = handles[2].fill
        assert bool((bits[:, :64] == fill).all()) and bool((bits[:, 160:] == fill).all()), "columns outside the window changed"
        G.check_all(*handles)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_conv2d_small_integers_come_back_exactly(hiplib, form):
    """Operands in {-1, 0, 1}, integer bias: every product and partial sum is an integer below 2^11 (K <= 1200), exact in
    fp32 and in f16, so the result is the float64 convolution bit for bit — any misplaced tap, fragment or tile changes it."""
    from rcdms_amd import hip
    (kh, kwid), stride, pad = form
    g = torch.Generator().manual_seed(3)
    for n, h, wd, ci, co in ((3, 9, 11, 48, 80), (1, 4, 5, 8, 8)):
        x = torch.randint(-1, 2, (n, h, wd, ci), generator=g).half()
        w = torch.randint(-1, 2, (co, ci, kh, kwid), generator=g).half()
        bias = torch.randint(-3, 4, (co,), generator=g).float()
        for epi in (hip.EPI_BIAS, hip.EPI_BIAS | hip.EPI_RELU, 0):
            ov, _, handles = run_conv(hip, x, w, bias if epi & hip.EPI_BIAS else None, stride, pad, epi, lda=ci + 8)
            y, _ = reference(x, w, bias if epi & hip.EPI_BIAS else None, stride, pad)
            if epi & hip.EPI_RELU:
                y = y.clamp_min(0.0)
            assert float(y.abs().max()) < 2048
            want = y.half()
            got = ov[:, :co].cpu()
            assert torch.equal(got.view(torch.int16), (want + 0.0).view(torch.int16)), (form, n, epi, int((got != want).sum()))
            G.check_all(*handles)


def test_conv2d_rows_beyond_two_gib(hiplib):
    """2 images of 6000 x 6000 rows of 16 halves: 2.3 GB of input and of output, so most of image 1 lies past byte 2^31 of
    both buffers — where a 32-bit byte offset wraps.  1 x 1, small integers: every output is exact, compared bit for bit with
    a product made on the device.  (No guard bands at this size: the pad columns 8..16 must keep their NaN.)"""
    from rcdms_amd import hip
    n, side_, ci, co, ld = 2, 6000, 8, 8, 16
    M = n * side_ * side_
    assert M * ld * 2 > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randint(-2, 3, (M, ld), generator=g, device=DEV, dtype=torch.int8).half()
    w = torch.randint(-1, 2, (co, ci), generator=g, device=DEV, dtype=torch.int8).half()
    bias = torch.randint(-3, 4, (co,), generator=g, device=DEV, dtype=torch.int8).float()
    out = torch.full((M, ld), float("nan"), dtype=torch.float16, device=DEV)
    d = hip.Conv2dDesc(n, side_, side_, ci, co, 1, 1, 1, 1, 0, 0, ld, ld, hip.EPI_BIAS)
    hip.conv2d(d, x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    want = torch.addmm(bias, x[:, :ci].float(), w.float().T).half()          # integers below 20: exact in fp32 and in f16
    assert bool((want.abs() <= 19).all())
    same = out[:, :co] == want
    assert bool(same.all()), f"{int((~same).sum())} outputs differ, first at row {int((~same).any(dim=1).nonzero()[0])} of {M}"
    assert bool(torch.isnan(out[:, co:]).all()), "the pad columns changed"
    # an unsupported row count is refused, not wrapped
    big = hip.Conv2dDesc(40, 8192, 8192, ci, co, 1, 1, 1, 1, 0, 0, ld, ld, hip.EPI_BIAS)
    assert hiplib.rcdm_conv2d(big, x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), 0) == -2


def test_conv2d_relu_epilogue(hiplib):
    """1 x 1 conv with a diagonal weight: output row = input row times the diagonal.  NaN passes, negatives and values that
    round to -0.0 give +0.0 under ReLU, and the bias-only epilogue stores what it stored without the new bit."""
    from rcdms_amd import hip
    vals = [1.5, -1.5, 2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0, 0.0, -0.25, 3.0, -3.0]
    x = torch.zeros(1, 4, 5, 8)
    for i, v in enumerate(vals):
        x[0, i // 5, i % 5, i % 8] = v
        x[0, 2 + i // 5, i % 5, 1] = v            # column 1 carries the factor 2^-14: -2^-28 rounds to -0.0 in f16
    x[0, 3, 4, :] = float("nan")
    x = x.half()
    diag = torch.ones(8)
    diag[1] = 2.0 ** -14
    w = torch.diag(diag).reshape(8, 8, 1, 1).half()
    bias = torch.zeros(8)
    bias[3] = 0.25
    y, _ = reference(x, w, bias, 1, (0, 0))
    plain, _, h0 = run_conv(hip, x, w, bias, 1, (0, 0), hip.EPI_BIAS)
    relu, _, h1 = run_conv(hip, x, w, bias, 1, (0, 0), hip.EPI_BIAS | hip.EPI_RELU)
    plain, relu = plain[:, :8].cpu(), relu[:, :8].cpu()
    nan = torch.isnan(y)
    assert nan[19].all() and int(nan.sum()) == 8
    assert torch.equal(torch.isnan(plain), nan) and torch.equal(torch.isnan(relu), nan)
    want_plain = y.half()
    ok = ~nan
    assert torch.equal(plain.view(torch.int16)[ok], want_plain.view(torch.int16)[ok])
    assert bool((plain.view(torch.int16)[ok] == -32768).any()), "the test lost its -0.0 case"
    want_relu = torch.where(y > 0, y, torch.zeros_like(y)).half()
    assert torch.equal(relu.view(torch.int16)[ok], want_relu.view(torch.int16)[ok])
    assert not bool((relu.view(torch.int16)[ok] < 0).any()), "a sign bit survived the ReLU"
    G.check_all(*h0, *h1)


# ---- pools ---------------------------------------------------------------------------------------------------------------

def run_pool(hip, x, k, s, p, mode, ld_pad=8):
    n, h, w, c = x.shape
    ho, wo = side(h, k, s, p), side(w, k, s, p)
    xv, hx = G.guarded_in(x.reshape(-1, c), c + ld_pad, device=DEV)
    ov, hout = G.guarded_out(n * ho * wo, c, c + 16, device=DEV)
    d = hip.Pool2dDesc(n, h, w, c, k, k, s, s, p, p, xv.shape[1], ov.shape[1], mode)
    hip.pool2d(d, xv.data_ptr(), ov.data_ptr())
    torch.cuda.synchronize()
    G.check_all(hx, hout)
    return ov[:, :c].cpu().reshape(n, ho, wo, c)


@pytest.mark.parametrize("c", [8, 776])
def test_pool2d_max(hiplib, c):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(c)
    for h, w in ((9, 11), (10, 10)):
        x = torch.randn(2, h, w, c, generator=g).half()
        got = run_pool(hip, x, 3, 2, 0, hip.POOL_MAX)
        want = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, stride=2).permute(0, 2, 3, 1).half()
        assert torch.equal(got, want)
    # all-negative input, 3 s1 p1: a zero from the padding would win every border window
    x = (-1.0 - torch.rand(2, 5, 6, c, generator=g)).half()
    got = run_pool(hip, x, 3, 1, 1, hip.POOL_MAX)
    want = F.max_pool2d(x.permute(0, 3, 1, 2).float(), 3, stride=1, padding=1).permute(0, 2, 3, 1).half()
    assert torch.equal(got, want) and bool((got < 0).all())


@pytest.mark.parametrize("c", [8, 776])
def test_pool2d_average_modes(hiplib, c):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(c + 1)
    x = (torch.randn(2, 5, 6, c, generator=g) + 1.0).half()
    xd = x.permute(0, 3, 1, 2).double()
    for mode, include in ((hip.POOL_AVG_INCLUDE_PAD, True), (hip.POOL_AVG_EXCLUDE_PAD, False)):
        got = run_pool(hip, x, 3, 1, 1, mode)
        want = F.avg_pool2d(xd, 3, stride=1, padding=1, count_include_pad=include).permute(0, 2, 3, 1)
        # within one f16 step of the float64 average: the spacing of f16 at the value (2^-10 relative, 2^-24 below 2^-14)
        step = torch.maximum(2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(2.0 ** -24).double())
        assert bool(((got.double() - want).abs() <= step).all()), float(((got.double() - want).abs() / step).max())
    # a window of ones makes the divisors visible: corner 4, edge 6, interior 9 taps in the image
    ones = torch.ones(1, 5, 6, c).half()
    inc = run_pool(hip, ones, 3, 1, 1, hip.POOL_AVG_INCLUDE_PAD)
    exc = run_pool(hip, ones, 3, 1, 1, hip.POOL_AVG_EXCLUDE_PAD)
    assert bool((exc == 1.0).all())
    for (yy, xx), taps in (((0, 0), 4), ((0, 2), 6), ((2, 0), 6), ((2, 3), 9), ((4, 5), 4)):
        assert bool((inc[0, yy, xx] == torch.tensor(taps / 9.0).half()).all()), (yy, xx)


@pytest.mark.parametrize("rows,c", [(64, 8), (64, 2048), (35, 8), (35, 2048)])
def test_global_avgpool_is_the_ordered_sum(hiplib, rows, c):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(rows + c)
    x = (torch.randn(3, rows, c, generator=g) * 2.0 + 0.5).half()
    xv, hx = G.guarded_in(x.reshape(-1, c), c + 8, device=DEV)
    outs = []
    for _ in range(2):
        ov, hout = G.guarded_out(3, c, c + 4, dtype=torch.float32, device=DEV, guard_rows=8)
        hip.global_avgpool(3, rows, c, xv.data_ptr(), xv.shape[1], ov.data_ptr(), ov.shape[1])
        torch.cuda.synchronize()
        G.check_all(hx, hout)
        outs.append(ov[:, :c].cpu())
    want = O.ordered_mean(x)
    assert torch.equal(outs[0].view(torch.int32), want.view(torch.int32)), float((outs[0] - want).abs().max())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# ---- bilinear frames -----------------------------------------------------------------------------------------------------

def run_bilinear(hip, frames, flip=False, c_pad=8, ld=16):
    """frames: device uint8 (n, H, W, 3) view of any pitch."""
    n, H, W, _ = frames.shape
    ov, hout = G.guarded_out(n * 299 * 299, c_pad, ld, device=DEV, guard_rows=64)
    d = hip.BilinearDesc(frames.stride(1), frames.stride(0) if n > 1 else 0, n, 3, H, W, 299, 299, int(flip), ld, c_pad,
                         (2.0, 2.0, 2.0), (-1.0, -1.0, -1.0))
    hip.image_bilinear_rows(d, frames.data_ptr(), ov.data_ptr())
    torch.cuda.synchronize()
    G.check_out(hout)
    return ov[:, :c_pad].cpu().reshape(n, 299, 299, c_pad)


def torch_resize_f16(frames_cpu):
    x = frames_cpu.permute(0, 3, 1, 2).float() / 255
    y = F.interpolate(x, (299, 299), mode="bilinear", align_corners=False) * 2 - 1
    return y.permute(0, 2, 3, 1).half()


def f16_step(v):
    """One f16 step at |v| (2^-11 just below 1, 2^-24 in the subnormal range): the bound wherever |v| >= 2^-9.  Below that
    (2 v - 1 cancels near an output of 0) the f16 spacing, 2^-19 and finer, approaches what two fp32 evaluations of the same
    formula may differ by before they are rounded — four products and three sums of values in [0, 1], then * 2 - 1, each
    rounded to 2^-24 relative: 16 * 2^-24 — and torch's own contraction pattern is not known, so only there that term is
    added.  The kernel is also held bit for bit to the written-out resize of tests/inception_oracle.py, which
    tests/test_inception_host.py ties to interpolate."""
    a = v.abs().double()
    step = 2.0 ** (torch.floor(torch.log2(a.clamp_min(2.0 ** -14))) - 10)
    return torch.where(a >= 2.0 ** -9, step, step + 16 * 2.0 ** -24)


def oracle_resize_f16(frames_cpu):
    return O.resize(frames_cpu).permute(0, 2, 3, 1).half()


def guarded_frames(frames_cpu, border=8):
    """The frames in the middle of a larger uint8 allocation of 0xA5 bytes -> (pitched device view, whole buffer, its snapshot)."""
    n, H, W, _ = frames_cpu.shape
    big = torch.full((n, H + 2 * border, W + 2 * border, 3), 0xA5, dtype=torch.uint8, device=DEV)
    big[:, border:border + H, border:border + W] = frames_cpu.to(DEV)
    return big[:, border:border + H, border:border + W], big, big.clone()


@pytest.mark.parametrize("hw", [(48, 64), (512, 512), (299, 299)], ids=["up", "down", "identity"])
def test_bilinear_rows_match_torch(hiplib, hw):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(hw[1])
    fr = torch.randint(0, 256, (2, *hw, 3), generator=g, dtype=torch.uint8)
    view, big, snap = guarded_frames(fr)
    got = run_bilinear(hip, view)
    assert torch.equal(big, snap), "the kernel wrote into its source"
    want = torch_resize_f16(fr)
    assert torch.equal(got[..., :3].view(torch.int16), oracle_resize_f16(fr).view(torch.int16)), "not the written-out resize, bit for bit"
    assert bool((got[..., 3:] == 0).all()) and not bool((got[..., 3:].view(torch.int16) != 0).any()), "pad channels are not +0"
    if hw == (299, 299):
        assert torch.equal(got[..., :3].view(torch.int16), want.view(torch.int16))
    else:
        diff = (got[..., :3].double() - want.double()).abs()
        assert bool((diff <= f16_step(want)).all()), float((diff / f16_step(want)).max())


def test_bilinear_rows_read_a_pitched_slice_and_flip_channels(hiplib):
    from rcdms_amd import hip
    g = torch.Generator().manual_seed(9)
    strip = torch.randint(0, 256, (2, 40, 3 * 56, 3), generator=g, dtype=torch.uint8)      # three 56-wide cells side by side
    cell = strip[:, 4:36, 56:112]                                                           # the middle cell, rows 4..35
    dev = strip.to(DEV)[:, 4:36, 56:112]
    assert not dev.is_contiguous()
    whole = dev._base.clone() if dev._base is not None else None
    got = run_bilinear(hip, dev, c_pad=16, ld=24)
    assert whole is not None and torch.equal(dev._base, whole), "the kernel wrote into the strip"
    want = torch_resize_f16(cell.contiguous())
    assert torch.equal(got[..., :3].view(torch.int16), oracle_resize_f16(cell.contiguous()).view(torch.int16))
    diff = (got[..., :3].double() - want.double()).abs()
    assert bool((diff <= f16_step(want)).all()), float((diff / f16_step(want)).max())
    assert not bool((got[..., 3:].view(torch.int16) != 0).any())
    flipped = run_bilinear(hip, dev, flip=True)
    assert torch.equal(flipped[..., :3].view(torch.int16), got[..., :3].flip(-1).contiguous().view(torch.int16))
