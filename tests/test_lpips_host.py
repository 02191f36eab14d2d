"""CPU: the LPIPS path before a GPU runs it.  The numpy model of csrc/lpips_core.h (tests/lpips_oracle.py) against the float64
head within the a-priori bound, the exact cases, the shared core compiled into tools/lpips_host.cpp — it must give the model's
bits —, AlexNet's stem as a 3 x 3 conv over space-to-depth rows against the direct 11 x 11 stride-4 conv bit for bit, the input
rows' table, and the key, shape and argument checks, which need no device.  Where the lpips package imports, the oracle is
compared with the package itself; it is not a dependency."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rcdms_amd import lpips as L
from tests import lpips_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_lpips_head_workspace_bytes", "rcdm_lpips_head", "rcdm_lpips_input_sides", "rcdm_lpips_input_rows")
# (P, hw, C): every lane count 1 .. 64, a lane group with dead lanes (192, 384), pixel counts around a tile and one pixel
HEAD_SHAPES = [(1, 1, 8), (3, 63, 64), (1, 64, 192), (3, 65, 512), (1, 257, 64), (3, 257, 8), (1, 65, 384), (2, 700, 16), (1, 5, 256),
               (1, 9, 32)]


def head_case(P, hw, c, magnitude=1.0):
    seed = 1000 * P + 10 * hw + c
    return O.features(P, hw, c, seed, magnitude), O.features(P, hw, c, seed + 1, magnitude), O.lin_weights(c, seed + 2)


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("P,hw,c", HEAD_SHAPES)
def test_model_within_the_bound_of_the_float64_head(P, hw, c):
    for magnitude in (1.0, 2.0 ** -14):
        a, b, lin = head_case(P, hw, c, magnitude)
        model, want, B = O.head_model(a, b, lin), O.head_f64(a, b, lin), O.head_bound(a, b, lin)
        err = np.abs(model - want)
        print(f"P {P} hw {hw} C {c} magnitude {magnitude:g}: value {want[0]:.6e}, |model - f64| {err.max():.3e}, bound {B.min():.3e}")
        assert (err <= B).all() and (B <= 2e-5 * want + 1e-30).all()          # and the bound itself is tight: ~1e-6 relative


def test_plausible_mistakes_lie_outside_the_bound():
    a, b, lin = head_case(3, 65, 64, 2.0 ** -14)
    want, B = O.head_f64(a, b, lin), O.head_bound(a, b, lin)
    inside = O.head_f64(a, b, lin, eps_inside_root=True)
    print(f"epsilon inside the root at magnitude 2^-14, C = 64: moves the result by {np.abs(inside / want - 1).max():.2e}, "
          f"the bound is {(B / want).max():.2e} of it")
    assert (np.abs(inside - want) > 100 * B).all()
    assert (np.abs(O.head_f64(a, b, np.ones_like(lin)) - want) > 100 * B).all()           # a missing lin
    pa, pb = np.concatenate([a, np.full_like(a[..., :8], 3e4)], -1), np.concatenate([b, np.full_like(b[..., :8], -3e4)], -1)
    over_ld = O.head_f64(pa, pb, np.concatenate([lin, np.zeros(8, np.float32)]))          # the norm taken over ld, not C
    assert (np.abs(over_ld - want) > 100 * B).all()


def test_exact_cases():
    c, hw = 64, 70
    lin = (np.arange(c) % 7 + 1).astype(np.float32) / 8.0                       # dyadic
    a = O.features(2, hw, c, 5)
    assert O.same_bits(O.head_model(a, a, lin), np.zeros(2))                     # identical inputs
    rng = np.random.RandomState(3)
    s = (2.0 ** -9 * (1 + rng.randint(0, 1 << 10, hw) / 1024.0) * 2.0 ** rng.randint(0, 20, hw)).astype(np.float16)
    t = (2.0 ** -9 * (1 + rng.randint(0, 1 << 10, hw) / 1024.0) * 2.0 ** rng.randint(0, 20, hw)).astype(np.float16)
    i, j = rng.randint(0, c, hw), rng.randint(0, c, hw)
    j = np.where(i == j, (j + 1) % c, j)
    a, b = np.zeros((1, hw, c), np.float16), np.zeros((1, hw, c), np.float16)
    a[0, np.arange(hw), i], b[0, np.arange(hw), j] = s, t
    want = (lin[i].astype(np.float64) + lin[j].astype(np.float64)).sum() / hw    # exact: multiples of 1 / 8 below 2^53
    assert O.same_bits(O.head_model(a, b, lin), [want])
    assert O.same_bits(O.pixel_values_model(a[0], b[0], lin).astype(np.float64), lin[i].astype(np.float64) + lin[j])
    b2 = np.zeros_like(b)
    b2[0, np.arange(hw), i] = t                                                  # i == j: both normalise to e_i
    assert O.same_bits(O.head_model(a, b2, lin), [0.0])
    z = np.zeros_like(a)
    assert O.same_bits(O.head_model(z, z, lin), [0.0])                           # 0 / 1e-10 - 0 / 1e-10
    one = O.head_model(a, z, lin)                                                # one side zero: lin_i per pixel
    assert np.isfinite(one).all() and O.same_bits(one, [lin[i].astype(np.float64).sum() / hw])


def test_counts():
    assert [O.lanes(c) for c in (8, 16, 24, 64, 192, 256, 384, 512)] == [1, 2, 4, 8, 32, 32, 64, 64]
    assert O.tiles(1) == 1 and O.tiles(64) == 1 and O.tiles(65) == 2 and O.tiles(257) == 5
    assert O.chain(1) == 15 and O.chain(64 * 256) == 15 and O.chain(64 * 256 + 1) == 16


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/lpips_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("lpips") / "lpips_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "lpips_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_host(host_tool, tmp_path, a, b, lin, lda=None, ldb=None):
    P, hw, c = a.shape
    lda, ldb = lda or c, ldb or c
    paths = []
    for key, arr, ld in (("a", a, lda), ("b", b, ldb)):
        rows = np.full((P * hw, ld), 3.0e4, np.float16)                          # pad columns hold poison: never read
        rows[:, :c] = arr.reshape(P * hw, c)
        paths.append(str(tmp_path / f"{key}.raw"))
        rows.view(np.uint16).tofile(paths[-1])
    paths.append(str(tmp_path / "lin.raw"))
    np.ascontiguousarray(lin, np.float32).tofile(paths[-1])
    r = subprocess.run([host_tool, str(P), str(hw), str(c), str(lda), str(ldb)] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([float(v) for v in r.stdout.decode().split()])


@pytest.mark.parametrize("P,hw,c", HEAD_SHAPES)
def test_host_tool_gives_the_models_bits(host_tool, tmp_path, P, hw, c):
    for magnitude, lda, ldb in ((1.0, None, None), (2.0 ** -14, c + 8, c + 24)):
        a, b, lin = head_case(P, hw, c, magnitude)
        got, model = run_host(host_tool, tmp_path, a, b, lin, lda, ldb), O.head_model(a, b, lin)
        assert O.same_bits(got, model), (got, model)


def test_host_tool_on_subnormal_halves_and_zeros(host_tool, tmp_path):
    a, b, lin = head_case(1, 40, 24, 2.0 ** -22)                                 # f16 subnormals: the widening's last branch
    a[0, :5], b[0, 3:9] = 0, 0
    assert O.same_bits(run_host(host_tool, tmp_path, a, b, lin), O.head_model(a, b, lin))


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(3, np.uint16).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("1", "2", "8", "8", "8", p, p, p)
    assert r.returncode == 2 and b"exactly" in r.stderr
    assert run("1", "2", "12", "16", "16", p, p, p).returncode == 2              # C no multiple of 8
    assert run("1", "2", "520", "520", "520", p, p, p).returncode == 2           # C above 512
    assert run("1", "2", "16", "8", "16", p, p, p).returncode == 2               # lda below C
    r = run("1")
    assert r.returncode == 2 and b"usage" in r.stderr


# ------------------------------------------------------------------------------------------------ AlexNet's stem, the input rows
@pytest.mark.parametrize("H,W", [(31, 34), (32, 33), (33, 32), (67, 95)])
def test_space_to_depth_stem_equals_the_direct_conv_bit_for_bit(H, W):
    rng = np.random.RandomState(H * 100 + W)
    x = rng.randint(-3, 4, (2, H, W, 3)).astype(np.float32)                      # small integers: every sum is exact in fp32
    w = torch.from_numpy(rng.randint(-2, 3, (64, 3, 11, 11)).astype(np.float32))
    bias = torch.from_numpy(rng.randint(-4, 5, 64).astype(np.float32))
    direct = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), w, bias, stride=4, padding=2)
    q = O.space_to_depth(x)
    ho, wo = O.alex_out_side(H), O.alex_out_side(W)
    assert q.shape == (2, ho + 2, wo + 2, 48) and tuple(direct.shape[2:]) == (ho, wo)
    rows = L.alex_stem_rows(w)
    assert rows.dtype == torch.float16 and tuple(rows.shape) == (64, 432)
    w3 = rows.to(torch.float32).view(64, 3, 3, 48).permute(0, 3, 1, 2).contiguous()
    got = F.conv2d(torch.from_numpy(q).permute(0, 3, 1, 2).contiguous(), w3, bias)
    assert got.shape == direct.shape and torch.equal(got, direct)
    assert float(direct.abs().max()) < 2 ** 24 and float(direct.abs().max()) > 0
    # the twelfth row and column of the 12 x 12 kernel are zeros
    w12 = rows.view(64, 3, 3, 4, 4, 3)
    assert not w12[:, 2, :, 3].any() and not w12[:, :, 2, :, 3].any()


def test_input_table_and_rows():
    mul, add = L.input_constants()
    assert np.float32(mul[0]) == np.float32(2.0 / 0.458) and np.float32(add[2]) == np.float32((-1.0 + 0.188) / 0.450)
    table = O.input_table(mul, add)
    u = np.arange(256, dtype=np.float64)[:, None]
    exact = (2.0 * u / 255.0 - 1.0 - np.array(L.SHIFT)) / np.array(L.SCALE)
    # one division, one fma and one f16 rounding from the real value: half an f16 ulp (2^-11 relative, 2^-25 absolute) and a bit
    assert (np.abs(table.astype(np.float64) - exact) <= 2.0 ** -11 * np.abs(exact) * (1 + 2.0 ** -10) + 2.0 ** -25).all()
    frames = np.random.RandomState(0).randint(0, 256, (2, 9, 11, 3)).astype(np.uint8)
    plain = O.input_rows(frames, 1, mul, add)
    assert plain.shape == (2, 9, 11, 8) and not plain[..., 3:].any() and plain[1, 4, 5, 2] == table[frames[1, 4, 5, 2], 2]
    q = O.input_rows(frames, 4, mul, add)
    assert q.shape == (2, 3, 4, 48) and not q[:, 0, :, :24].any() and not q[:, :, 0].reshape(2, 3, 4, 4, 3)[:, :, :, :2].any()
    assert q[0, 1, 1, (1 * 4 + 2) * 3 + 1] == table[frames[0, 3, 4, 1], 1]       # (Y, X, dy, dx) = (1, 1, 1, 2) -> source (3, 4)


# ------------------------------------------------------------------------------------------------ keys, shapes, arguments
def test_state_dict_checks():
    for net in L.NETS:
        for prefix in ("lpips", "features"):
            sd = O.synthetic_state_dict(net, 0, prefix)
            keys = L.check_state_dict(sd, net)
            assert len(keys) == len(L.CONVS[net]) + 5 + 2 and keys["shift"] is None
    sd = O.synthetic_state_dict("alex", 0)
    sd["scaling_layer.shift"], sd["scaling_layer.scale"] = torch.tensor(L.SHIFT).view(1, 3, 1, 1), torch.tensor(L.SCALE).view(1, 3, 1, 1)
    assert L.check_state_dict(sd, "alex")["scale"] == "scaling_layer.scale"
    with pytest.raises(ValueError, match="one of"):
        L.check_state_dict(sd, "squeeze")
    for drop in ("net.slice2.3.weight", "net.slice5.10.bias", "lin3.model.1.weight"):
        bad = {k: v for k, v in sd.items() if k != drop}
        with pytest.raises(ValueError, match="lacks"):
            L.LpipsNet(bad, "alex")                                              # before any device is touched
    for key, shape in (("net.slice1.0.weight", (64, 3, 11, 10)), ("net.slice3.6.bias", (383,)), ("lin1.model.1.weight", (1, 64, 1, 1)),
                       ("lin0.model.1.weight", (64,))):
        bad = dict(sd)
        bad[key] = torch.zeros(shape)
        with pytest.raises(ValueError, match="got"):
            L.LpipsNet(bad, "alex")
    bad = dict(sd)
    bad["lin4.model.1.weight"] = sd["lin4.model.1.weight"].clone()
    bad["lin4.model.1.weight"][0, 7] = -1e-3
    with pytest.raises(ValueError, match="negative"):
        L.LpipsNet(bad, "alex")
    bad = dict(sd)
    bad["scaling_layer.scale"] = torch.tensor([0.458, 0.0, 0.45])
    with pytest.raises(ValueError, match="scale"):
        L.LpipsNet(bad, "alex")
    with pytest.raises(ValueError, match="got"):
        L.LpipsNet(sd, "vgg")                                                    # AlexNet's keys are not VGG's


def test_python_layer_refuses_before_any_device_access():
    from rcdms_amd import hip
    sd = O.synthetic_state_dict("alex", 0)
    with pytest.raises(hip.RcdmError):
        L.LpipsNet(sd, "alex", device="cpu")
    for bad in ({"batch": 0}, {"plans": 0}):
        with pytest.raises(ValueError):
            L.LpipsNet(sd, "alex", **bad)
    L.check_sides("vgg", 16, 16), L.check_sides("alex", 31, 31)
    for net, H, W in (("vgg", 15, 64), ("vgg", 64, 15), ("alex", 30, 64), ("alex", 64, 30)):
        with pytest.raises(ValueError, match="at least"):
            L.check_sides(net, H, W)
    assert L.MIN_SIDE == {"vgg": 16, "alex": 31}


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in NEW_SYMBOLS:
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.LpipsHeadDesc) == 40 and hip.LpipsHeadDesc.pairs.offset == 16
    assert ctypes.sizeof(hip.LpipsInputDesc) == 64 and hip.LpipsInputDesc.mul.offset == 36
    assert (hip.LPIPS_MAX_C, hip.LPIPS_TILE) == (512, O.TILE)
    assert lib.rcdm_version() == 0x000300


def test_argument_validation_without_gpu():
    """The entry points refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4

    def desc(lda=64, ldb=64, pairs=2, h=5, w=7, c=64, blocks=0):
        return hip.LpipsHeadDesc(lda, ldb, pairs, h, w, c, blocks, 0)
    wsb = lambda d: lib.rcdm_lpips_head_workspace_bytes(ctypes.byref(d))
    assert wsb(desc()) == 2 * 1 * 8 and wsb(desc(h=16, w=17)) == 2 * 5 * 8 and wsb(desc(c=512, lda=512, ldb=520)) == 16
    invalid = (desc(pairs=0), desc(h=0), desc(w=0), desc(c=0), desc(lda=56), desc(ldb=56), desc(blocks=-1))
    shape = (desc(c=60), desc(lda=68), desc(ldb=68), desc(c=520, lda=520, ldb=520), desc(pairs=65536), desc(h=8193))
    for bad in invalid + shape:
        assert wsb(bad) == 0
    assert lib.rcdm_lpips_head_workspace_bytes(None) == 0
    a, b, lin, out, ws, st = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0                    # never dereferenced
    head = lambda d, *args: lib.rcdm_lpips_head(ctypes.byref(d), *args)
    for bad in invalid:
        assert head(bad, a, b, lin, out, ws, 1 << 20, st) == EINVAL
    for bad in shape:
        assert head(bad, a, b, lin, out, ws, 1 << 20, st) == ESHAPE
    good = desc()
    assert lib.rcdm_lpips_head(None, a, b, lin, out, ws, 16, st) == EINVAL
    for args in ((0, b, lin, out, ws), (a, 0, lin, out, ws), (a, b, 0, out, ws), (a, b, lin, 0, ws), (a, b, lin, out, 0)):
        assert head(good, *args, 16, st) == EINVAL
    for args in ((a + 8, b, lin, out, ws), (a, b + 2, lin, out, ws), (a, b, lin + 4, out, ws), (a, b, lin, out + 4, ws),
                 (a, b, lin, out, ws + 8)):
        assert head(good, *args, 16, st) == EINVAL
    assert head(good, a, b, lin, out, ws, 8, st) == EWORKSPACE

    def idesc(pitch=30, stride=300, n=2, H=10, W=10, s2d=1, ld=8):
        return hip.LpipsInputDesc(pitch, stride, n, H, W, s2d, ld, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert hip.lpips_input_sides(idesc()) == (10, 10, 8) and hip.lpips_input_sides(idesc(s2d=4, ld=48)) == (3, 3, 48)
    assert hip.lpips_input_sides(idesc(pitch=3 * 67, H=67, W=67, s2d=4, ld=56)) == (18, 18, 48)
    rows = lambda d, *args: lib.rcdm_lpips_input_rows(ctypes.byref(d), *args)
    src, dst = 0x1000, 0x2000
    for bad in (idesc(n=0), idesc(H=0), idesc(pitch=29), idesc(stride=-1), idesc(ld=12), idesc(s2d=4, ld=40)):
        assert rows(bad, src, dst, st) == EINVAL
    for bad in (idesc(s2d=2), idesc(s2d=4, ld=48, H=6), idesc(H=8193)):
        assert rows(bad, src, dst, st) == ESHAPE
    assert rows(idesc(), 0, dst, st) == EINVAL and rows(idesc(), src, 0, st) == EINVAL and rows(idesc(), src, dst + 8, st) == EINVAL
    nan = idesc()
    nan.mul[1] = float("nan")
    assert rows(nan, src, dst, st) == EINVAL


# ------------------------------------------------------------------------------------------------ the package, where it imports
def test_oracle_against_the_lpips_package():
    """Only where the lpips package (and the torchvision it needs) is installed: its own forward on random-initialised towers
    against tests/lpips_oracle.py, and its state_dict() through check_state_dict.  Neither is a dependency of the project."""
    lpips = pytest.importorskip("lpips")
    pytest.importorskip("torchvision")
    rng = np.random.RandomState(0)
    for net, (H, W) in (("alex", (67, 95)), ("vgg", (32, 48))):
        model = lpips.LPIPS(net=net, pretrained=False, pnet_rand=True, verbose=False).eval()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k in sd:
            if k.endswith(".model.1.weight"):
                sd[k] = sd[k].abs()
        model.load_state_dict(sd)
        L.check_state_dict(sd, net)
        a, b = (rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8) for _ in range(2))
        to_t = lambda f: torch.from_numpy(f).to(torch.float32).permute(0, 3, 1, 2) / 255.0 * 2.0 - 1.0
        with torch.no_grad():
            total, layers = model(to_t(a), to_t(b), retPerLayer=True)
        want = np.stack([v.reshape(-1).numpy() for v in layers], axis=1).astype(np.float64)
        got = O.distance(sd, net, a, b)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-7), (got, want)
        assert np.allclose(got.sum(1), total.reshape(-1).numpy(), rtol=1e-4, atol=1e-7)
