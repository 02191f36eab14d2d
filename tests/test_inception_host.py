"""CPU: the Inception-v3 restatement (tests/inception_oracle.py), the host side of rcdms_amd/inception.py, and the argument
checks of the four entry points of csrc/conv2d.hip, all without a device.  torchvision is compared against only where it
imports (it is not a dependency of this repository): the parity status of the oracle is "restated, unpinned"."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import inception_oracle as O

EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def sd():
    return O.synthetic_state_dict(0)


@pytest.fixture(scope="module")
def frames():
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, 256, (2, 48, 64, 3), generator=g, dtype=torch.uint8)


@pytest.fixture(scope="module")
def taps(sd, frames):
    out = {}
    for v in ("fid", "torchvision"):
        t = {}
        f = O.features(sd, frames, v, taps=t)
        out[v] = (f, t)
    return out


def test_oracle_shapes_and_channel_sums(taps):
    for v, (f, t) in taps.items():
        assert tuple(f.shape) == (2, 2048) and f.dtype == torch.float32
        assert list(t) == list(O.BLOCKS)
        for name, y in t.items():
            side = O.BLOCK_SIDES[name]
            assert tuple(y.shape) == (2, O.BLOCK_CHANNELS[name], side, side), (v, name, tuple(y.shape))
    # the concat of every block is the sum of its branches
    s = O.conv_shapes()
    assert 64 + 64 + 96 + s["Mixed_5b.branch_pool"][0] == 256 and 64 + 64 + 96 + s["Mixed_5d.branch_pool"][0] == 288
    assert s["Mixed_6a.branch3x3"][0] + s["Mixed_6a.branch3x3dbl_3"][0] + 288 == 768
    for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        assert sum(s[f"{b}.{k}"][0] for k in ("branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool")) == 768
    assert s["Mixed_7a.branch3x3_2"][0] + s["Mixed_7a.branch7x7x3_4"][0] + 768 == 1280
    for b in ("Mixed_7b", "Mixed_7c"):
        assert s[f"{b}.branch1x1"][0] + 2 * 384 + 2 * 384 + s[f"{b}.branch_pool"][0] == 2048


def test_synthetic_activations_stay_order_one(taps):
    for v, (f, t) in taps.items():
        rms = {k: float(y.pow(2).mean().sqrt()) for k, y in t.items()}
        print(v, {k: round(r, 3) for k, r in rms.items()})
        assert all(0.2 <= r <= 6.0 for r in rms.values()), rms
        assert torch.isfinite(f).all()


def test_variants_differ_where_the_pools_differ(taps):
    fid, tv = taps["fid"][1], taps["torchvision"][1]
    assert torch.equal(fid["maxpool2"], tv["maxpool2"])
    assert not torch.equal(fid["Mixed_5b"], tv["Mixed_5b"])
    # the four corners see 4 of 9 taps: exclude-pad and include-pad differ there; the other three branches are the same
    assert torch.equal(fid["Mixed_5b"][:, :224], tv["Mixed_5b"][:, :224])


def test_bn_fold_matches_unfolded_evaluation_in_float64(sd):
    g = torch.Generator().manual_seed(5)
    for name, stride, pad in (("Mixed_5b.branch5x5_2", 1, 2), ("Mixed_6b.branch7x7_2", 1, (0, 3)), ("Mixed_6a.branch3x3", 2, 0)):
        co, ci, kh, kw = O.conv_shapes()[name]
        x = torch.randn(2, ci, 9, 11, generator=g, dtype=torch.float64)
        ref = O.Net(sd, dtype=torch.float64).conv(name, x, stride=stride, padding=pad)
        w, b = O.fold_bn(sd, name)
        got = F.relu(F.conv2d(x, w.double(), b.double(), stride=stride, padding=pad))
        # the fold is done in fp32: 2^-24 relative on the weights and the bias, summed over K products
        tol = 4 * 2.0 ** -24 * (F.conv2d(x.abs(), w.double().abs(), b.double().abs(), stride=stride, padding=pad))
        assert bool(((got - ref).abs() <= tol + 1e-12).all()), float((got - ref).abs().max())
        # and the extractor's own fold: the same numbers, permuted to (c_out, kh, kw, c_in) and rounded to f16
        from rcdms_amd import inception as I
        W16, b32 = I.fold_conv(sd, name)
        assert torch.equal(W16, w.permute(0, 2, 3, 1).reshape(co, -1).to(torch.float16)) and torch.equal(b32, b)
    W16, _ = I.fold_conv(sd, "Conv2d_1a_3x3")
    assert tuple(W16.shape) == (32, 3 * 3 * 8) and bool((W16.view(32, 9, 8)[:, :, 3:] == 0).all())


def test_state_dict_keys_and_refusals(sd):
    from rcdms_amd import inception as I
    want = O.state_dict_shapes(1000)
    keys = I.expected_keys()
    assert list(keys) == list(want)
    for k, shape in want.items():
        assert tuple(1000 if v is None else v for v in keys[k]) == shape, k
    assert I.check_state_dict(sd) == 1000
    extra = dict(sd)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    assert I.check_state_dict(extra) == 1000
    for nc in (7, 9, 1008):
        d = dict(sd)
        d["fc.weight"], d["fc.bias"] = torch.zeros(nc, 2048), torch.zeros(nc)
        assert I.check_state_dict(d) == nc
    d = dict(sd)
    del d["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(ValueError, match="Mixed_6c.branch7x7dbl_3.bn.running_var"):
        I.check_state_dict(d)
    d = dict(sd)
    d["Mixed_7a.branch7x7x3_2.conv.weight"] = torch.zeros(192, 192, 7, 1)     # (1, 7) and (7, 1) swapped
    with pytest.raises(ValueError, match="Mixed_7a.branch7x7x3_2.conv.weight"):
        I.check_state_dict(d)
    d = dict(sd)
    d["fc.bias"] = torch.zeros(1001)
    with pytest.raises(ValueError, match="fc.bias"):
        I.check_state_dict(d)
    # the constructor refuses before it needs a device
    with pytest.raises(ValueError, match="lacks"):
        I.InceptionV3Features({}, device="cuda:0")
    with pytest.raises(ValueError, match="variant"):
        I.InceptionV3Features(sd, variant="tf", device="cuda:0")
    from rcdms_amd import hip
    with pytest.raises(hip.RcdmError, match="no CPU path"):
        I.InceptionV3Features(sd, device="cpu")


@pytest.mark.parametrize("hw", [(48, 64), (512, 512), (299, 299)], ids=["up", "down", "identity"])
def test_resize_restatement_against_interpolate(hw):
    g = torch.Generator().manual_seed(hw[0])
    fr = torch.randint(0, 256, (2, *hw, 3), generator=g, dtype=torch.uint8)
    x = fr.permute(0, 3, 1, 2).float() / 255
    want = F.interpolate(x, (299, 299), mode="bilinear", align_corners=False) * 2 - 1
    got = O.resize(fr)
    assert tuple(got.shape) == (2, 3, 299, 299)
    if hw == (299, 299):
        assert torch.equal(got, want) and torch.equal(got, x * 2 - 1)
    else:
        # the same coordinates and weights; four products and three sums of values in [0, 1] in fp32, contracted or not, then
        # * 2 - 1: a few fp32 roundings of numbers below 2
        tol = 16 * 2.0 ** -24
        diff = float((got - want).abs().max())
        print(f"resize {hw} -> 299: worst |restatement - interpolate| {diff:.2e}, allowed {tol:.2e}")
        assert diff <= tol


def test_ordered_mean_is_a_sequential_fp32_sum():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 35, 8, generator=g).half()
    got = O.ordered_mean(x)
    s = torch.zeros(2, 8)
    for r in range(35):
        s += x[:, r].float()
    assert torch.equal(got, s / 35.0) and got.dtype == torch.float32
    assert float((got - x.double().mean(dim=1)).abs().max()) <= 35 * 2.0 ** -24 * float(x.abs().max())


def test_new_entry_points_validate_without_gpu():
    """Every refusal comes back before the device is touched: the pointers below are not device memory."""
    from rcdms_amd import hip
    lib = hip.load()
    P = 4096                                                              # a non-null, 16-byte aligned, never dereferenced "pointer"

    def conv(**kw):
        a = dict(n_img=1, h_in=9, w_in=11, c_in=8, c_out=8, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=0, pad_w=0, lda=8, ldc=8,
                 epilogue=hip.EPI_BIAS | hip.EPI_RELU)
        a.update(kw)
        return lib.rcdm_conv2d(ctypes.byref(hip.Conv2dDesc(**a)), P, P, P, P, 0)
    assert conv(c_in=12, lda=12) == ESHAPE                                # c_in % 8 != 0
    assert conv(c_out=12, ldc=16) == ESHAPE
    assert conv(kh=9, h_in=20) == ESHAPE
    assert conv(stride_h=3) == ESHAPE and conv(stride_w=0) == ESHAPE
    assert conv(h_in=2) == ESHAPE                                         # h_out < 1
    assert conv(w_in=4, kw=7) == ESHAPE                                   # w_out < 1
    assert conv(epilogue=hip.EPI_RESIDUAL) == ESHAPE and conv(epilogue=128) == ESHAPE
    assert conv(epilogue=hip.EPI_RELU | hip.EPI_GELU) == ESHAPE
    assert conv(lda=4) == EINVAL and conv(n_img=0) == EINVAL
    assert lib.rcdm_conv2d(None, P, P, P, P, 0) == EINVAL
    d = hip.Conv2dDesc(1, 9, 11, 8, 8, 3, 3, 1, 1, 0, 0, 8, 8, hip.EPI_BIAS)
    assert lib.rcdm_conv2d(ctypes.byref(d), 0, P, P, P, 0) == EINVAL
    assert lib.rcdm_conv2d(ctypes.byref(d), P, P, 0, P, 0) == EINVAL      # the bias the epilogue asks for
    assert lib.rcdm_conv2d(ctypes.byref(d), P, P + 2, P, P, 0) == EINVAL  # alignment

    # RCDM_EPI_RELU is rcdm_conv2d's: the GEMM and the 3x3 conv refuse it, as they refuse a bit nobody defines
    g = hip.GemmDesc(16, 16, 64, 64, 16, 0, hip.EPI_RELU, 1, 0, 1.0, 1)
    assert lib.rcdm_gemm(ctypes.byref(g), P, P, 0, 0, 0, P, 0, 0, 0) == ESHAPE
    g = hip.GemmDesc(16, 16, 64, 64, 16, 0, hip.EPI_BIAS | hip.EPI_RELU, 1, 0, 1.0, 1)
    assert lib.rcdm_gemm(ctypes.byref(g), P, P, P, 0, 0, P, 0, 0, 0) == ESHAPE
    c = hip.ConvDesc(n_img=1, h_in=8, w_in=8, c_in=8, c_out=8, stride=1, upsample=1, lda=8, ldc=8, epilogue=hip.EPI_RELU,
                     rows_per_sample=1, out_scale=1.0, split_k=1)
    assert lib.rcdm_conv3x3(ctypes.byref(c), P, P, 0, 0, 0, P, 0, 0, 0) == ESHAPE

    def pool(**kw):
        a = dict(n_img=1, h_in=9, w_in=11, c=8, kh=3, kw=3, stride_h=2, stride_w=2, pad_h=0, pad_w=0, ld_in=8, ld_out=8,
                 mode=hip.POOL_MAX)
        a.update(kw)
        return lib.rcdm_pool2d(ctypes.byref(hip.Pool2dDesc(**a)), P, P, 0)
    assert pool(c=12, ld_in=16, ld_out=16) == ESHAPE and pool(kh=4) == ESHAPE and pool(stride_h=3) == ESHAPE
    assert pool(pad_h=2) == ESHAPE and pool(h_in=2) == ESHAPE
    assert pool(mode=3) == EINVAL and pool(ld_out=4) == EINVAL
    assert lib.rcdm_pool2d(None, P, P, 0) == EINVAL
    assert lib.rcdm_pool2d(ctypes.byref(hip.Pool2dDesc(1, 9, 11, 8, 3, 3, 2, 2, 0, 0, 8, 8, 0)), P, 0, 0) == EINVAL

    gap = lib.rcdm_global_avgpool
    assert gap(1, 64, 12, P, 16, P, 16, 0) == ESHAPE and gap(1, 64, 8, P, 12, P, 8, 0) == ESHAPE
    assert gap(0, 64, 8, P, 8, P, 8, 0) == EINVAL and gap(1, 64, 8, 0, 8, P, 8, 0) == EINVAL and gap(1, 64, 8, P, 8, 0, 8, 0) == EINVAL
    assert gap(1, 64, 16, P, 8, P, 16, 0) == EINVAL                       # ld below c

    def bil(src=P, dst=P, **kw):
        a = dict(src_pitch=3 * 64, src_stride=3 * 64 * 48, n=2, channels=3, in_h=48, in_w=64, out_h=299, out_w=299, flip_channels=0,
                 ld=8, c_pad=8, scale=(2.0, 2.0, 2.0), shift=(-1.0, -1.0, -1.0))
        a.update(kw)
        return lib.rcdm_image_bilinear_rows(ctypes.byref(hip.BilinearDesc(**a)), src, dst, 0)
    assert bil(channels=4) == ESHAPE and bil(out_h=10000) == ESHAPE
    assert bil(src_pitch=100) == EINVAL and bil(c_pad=4) == EINVAL and bil(ld=12) == EINVAL and bil(n=0) == EINVAL
    assert bil(src=0) == EINVAL and bil(dst=0) == EINVAL and bil(dst=P + 8) == EINVAL
    assert lib.rcdm_image_bilinear_rows(None, P, P, 0) == EINVAL


class _NoPipe:
    device = torch.device("cpu")


def test_story_runner_feature_source_argument_errors():
    from rcdms_amd.story import StoryRunner
    frames = torch.zeros(1, 5, 8, 8, 3, dtype=torch.uint8)
    caps = [["a", "b", "c", "d", "e"]]
    r = StoryRunner(_NoPipe(), _NoPipe(), None, clip_processor=object(), frame_transform=object())
    with pytest.raises(ValueError, match="feature_source"):
        r(frames, caps, feature_source="fid")
    with pytest.raises(ValueError, match="extractor"):
        r(frames, caps, feature_source="inception", output_type="uint8")
    r = StoryRunner(_NoPipe(), _NoPipe(), None, clip_processor=object(), frame_transform=object(), inception=lambda x: x)
    with pytest.raises(ValueError, match="uint8"):
        r(frames, caps, feature_source="inception", output_type="tensor")
    with pytest.raises(ValueError, match="uint8"):
        r(frames, caps, feature_source="inception", output_type="pil")
    with pytest.raises(ValueError, match="feature_source"):
        r.story_metrics(frames, frames, None, (), feature_source="both")


def test_oracle_against_torchvision_where_it_imports(sd, frames):
    tv = pytest.importorskip("torchvision")
    m = tv.models.inception_v3(weights=None, aux_logits=True, init_weights=False, transform_input=False)
    full = m.state_dict()
    for k, v in sd.items():
        assert k in full and tuple(full[k].shape) == tuple(v.shape), k
        full[k] = v
    m.load_state_dict(full)
    m.eval()
    x = O.resize(frames)
    with torch.no_grad():
        want = m(x)
    net = O.Net(sd, "torchvision")
    f = net.features(x)
    got = net.logits(f)
    assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max())
