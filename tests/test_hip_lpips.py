"""GPU: rcdms_amd.lpips and the kernels under it (csrc/lpips.hip), in guarded buffers (tests/guard.py).

  head, exact    identical inputs give exactly 0.0; one-hot pixels a = s e_i, b = t e_j give exactly lin_i + lin_j (i != j) and 0
                 (i == j); all-zero pixels on one or both sides are finite and equal the model.  No tolerance.
  head, oracle   within the a-priori bound of tests/lpips_oracle.py of the float64 head, and the numpy model's bits, at
                 C in {8, 64, 192, 512}, pixel counts {1, 63, 64, 65, 257}, P in {1, 3}, ld > C with poisoned pad columns, the two
                 sets in separate buffers and in one; features of magnitude 2^-14, where the oracle shows that the plausible
                 mistakes (epsilon inside the root, a norm over ld, a missing lin) lie at least ten bounds away; a rerun and
                 other grid sizes give the same bits.
  input rows     both layouts equal the oracle's rows bit for bit, from strips of a wider frame buffer with an odd pitch.
  towers         VGG-16 at 32 x 48 and AlexNet at 67 x 95, 2 pairs, synthetic full-width weights: every tapped feature map within
                 2 e_model of the fp32 oracle in relative RMS (e_model: the f16 model's own error, the rule of
                 tests/test_hip_inception.py); the distances equal rcdm_lpips_head on those taps bit for bit; chunked equals
                 unchunked; net(a, a) is exactly 0."""
import numpy as np
import pytest
import torch

from tests import guard as G
from tests import lpips_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GR = 8
SIDES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 257: (257, 1)}


@pytest.fixture(scope="module")
def hip(hiplib):
    from rcdms_amd import hip
    return hip


def run_head(hip, a, b, lin, lda=None, ldb=None, shared=False, blocks=0, sides=None):
    """rcdm_lpips_head on guarded buffers.  a, b: (P, hw, C) f16 numpy -> (P,) float64 numpy."""
    P, hw, c = a.shape
    h, w = sides or SIDES.get(hw, (1, hw))
    assert h * w == hw
    lda = lda or c + 8
    ldb = lda if shared else (ldb or c + 24)
    if shared:
        both = torch.from_numpy(np.concatenate([a, b]).reshape(2 * P * hw, c))
        av, ah = G.guarded_in(both, lda, device=DEV, guard_rows=GR)
        pa, pb, handles = av.data_ptr(), av.data_ptr() + 2 * P * hw * lda, [ah]
    else:
        av, ah = G.guarded_in(torch.from_numpy(a.reshape(P * hw, c)), lda, device=DEV, guard_rows=GR)
        bv, bh = G.guarded_in(torch.from_numpy(b.reshape(P * hw, c)), ldb, device=DEV, guard_rows=GR)
        pa, pb, handles = av.data_ptr(), bv.data_ptr(), [ah, bh]
    lv, lh = G.guarded_vec(torch.from_numpy(np.asarray(lin, np.float32)), device=DEV)
    d = hip.LpipsHeadDesc(lda, ldb, P, h, w, c, blocks, 0)
    need = hip.lpips_head_workspace_bytes(d)
    assert need == P * O.tiles(hw) * 8
    ov, oh = G.guarded_out(1, P, P + 3, torch.float64, device=DEV, guard_rows=GR)
    wv, wh = G.guarded_out(1, need // 8, need // 8 + 2, torch.float64, device=DEV, guard_rows=GR)
    hip.lpips_head(d, pa, pb, lv.data_ptr(), ov.data_ptr(), wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_written(oh)
    G.check_written(wh)
    G.check_all(*handles, lh, oh, wh)
    return oh.data.cpu().numpy().reshape(-1)


def head_case(P, hw, c, magnitude=1.0):
    seed = 1000 * P + 10 * hw + c
    return O.features(P, hw, c, seed, magnitude), O.features(P, hw, c, seed + 1, magnitude), O.lin_weights(c, seed + 2)


# ------------------------------------------------------------------------------------------------ head: exact answers
@pytest.mark.parametrize("c", [8, 64, 192, 512])
def test_head_exact_answers(hip, c):
    hw = 65
    lin = (np.arange(c) % 7 + 1).astype(np.float32) / 8.0                        # dyadic
    a = O.features(2, hw, c, 5)
    assert O.same_bits(run_head(hip, a, a.copy(), lin), np.zeros(2))             # identical inputs: exactly 0.0
    rng = np.random.RandomState(c)
    s = (2.0 ** -9 * (1 + rng.randint(0, 1 << 10, hw) / 1024.0) * 2.0 ** rng.randint(0, 20, hw)).astype(np.float16)
    t = (2.0 ** -9 * (1 + rng.randint(0, 1 << 10, hw) / 1024.0) * 2.0 ** rng.randint(0, 20, hw)).astype(np.float16)
    s[0], t[0], s[1], t[1] = 2.0 ** -9, 65504.0, 65504.0, 2.0 ** -9              # the ends of the range
    i, j = rng.randint(0, c, hw), rng.randint(0, c, hw)
    j = np.where(i == j, (j + 1) % c, j)
    a, b = np.zeros((1, hw, c), np.float16), np.zeros((1, hw, c), np.float16)
    a[0, np.arange(hw), i], b[0, np.arange(hw), j] = s, t
    want = (lin[i].astype(np.float64) + lin[j].astype(np.float64)).sum() / hw    # multiples of 1 / 8: every sum is exact
    assert O.same_bits(run_head(hip, a, b, lin), [want])
    b2 = np.zeros_like(b)
    b2[0, np.arange(hw), i] = t
    assert O.same_bits(run_head(hip, a, b2, lin), [0.0])                         # i == j: exactly 0
    z = np.zeros_like(a)
    both = run_head(hip, z, z.copy(), lin)
    assert O.same_bits(both, [0.0]) and O.same_bits(both, O.head_model(z, z, lin))
    for x, y in ((a, z), (z, b)):
        one = run_head(hip, x, y, lin)
        assert np.isfinite(one).all() and O.same_bits(one, O.head_model(x, y, lin))
    mixed_a, mixed_b = O.features(1, hw, c, 9), O.features(1, hw, c, 10)         # some pixels all zero on one side, some on both
    mixed_a[0, ::3], mixed_b[0, ::4] = 0, 0
    got = run_head(hip, mixed_a, mixed_b, lin)
    assert np.isfinite(got).all() and O.same_bits(got, O.head_model(mixed_a, mixed_b, lin))


# ------------------------------------------------------------------------------------------------ head: against the oracle
@pytest.mark.parametrize("c", [8, 64, 192, 512])
def test_head_within_the_bound_of_the_float64_oracle(hip, c):
    for hw in (1, 63, 64, 65, 257):
        for P in (1, 3):
            a, b, lin = head_case(P, hw, c)
            want, B, model = O.head_f64(a, b, lin), O.head_bound(a, b, lin), O.head_model(a, b, lin)
            for shared in (False, True):
                got = run_head(hip, a, b, lin, shared=shared)
                err = np.abs(got - want)
                print(f"C {c} hw {hw} P {P} shared {shared}: |kernel - f64| {err.max():.3e}, bound {B.min():.3e}, value {want[0]:.4f}")
                assert (err <= B).all(), (err, B)
                assert O.same_bits(got, model), (got, model)


def test_head_at_magnitude_2_to_minus_14_and_the_plausible_mistakes(hip):
    for c, hw, P in ((8, 257, 3), (64, 65, 3), (512, 63, 1)):
        a, b, lin = head_case(P, hw, c, 2.0 ** -14)
        want, B = O.head_f64(a, b, lin), O.head_bound(a, b, lin)
        got = run_head(hip, a, b, lin)
        assert (np.abs(got - want) <= B).all() and O.same_bits(got, O.head_model(a, b, lin))
        # on the oracle: each plausible mistake moves the result far beyond the bound on these inputs
        inside = O.head_f64(a, b, lin, eps_inside_root=True)
        print(f"C {c}: epsilon inside the root moves the result by {np.abs(inside / want - 1).max():.2e}, bound {(B / want).max():.2e}")
        assert (np.abs(inside - want) > 10 * B).all() and (np.abs(got - inside) > 9 * B).all()
        no_lin = O.head_f64(a, b, np.ones_like(lin))
        assert (np.abs(no_lin - want) > 100 * B).all()
        pad = np.full_like(a[..., :8], G.POISON)                                 # what the pad columns of run_head's buffers hold
        over_ld = O.head_f64(np.concatenate([a, pad], -1), np.concatenate([b, -pad], -1), np.concatenate([lin, np.zeros(8, np.float32)]))
        assert (np.abs(over_ld - want) > 100 * B).all()


def test_head_same_bits_on_a_rerun_and_for_every_grid(hip):
    a, b, lin = head_case(3, 257 * 5, 64)                                        # 21 tiles per pair, 63 jobs
    first = run_head(hip, a, b, lin)
    assert O.same_bits(first, O.head_model(a, b, lin))
    for blocks in (0, 1, 5, 63, 1000):
        assert O.same_bits(run_head(hip, a, b, lin, blocks=blocks), first), blocks


# ------------------------------------------------------------------------------------------------ input rows
@pytest.mark.parametrize("s2d,H,W", [(1, 16, 17), (1, 5, 3), (4, 31, 34), (4, 32, 33), (4, 33, 32), (4, 67, 95), (4, 7, 7)])
def test_input_rows_equal_the_oracle_bit_for_bit(hip, s2d, H, W):
    from rcdms_amd import lpips as L
    n = 3
    mul, add = L.input_constants()
    big = torch.from_numpy(np.random.RandomState(H * W + s2d).randint(0, 256, (n, H + 5, W + 8, 3)).astype(np.uint8)).to(DEV)
    big[0, 2, 5], big[1, 2 + H - 1, 5 + W - 1] = 0, 255                          # the corners hold both ends of the byte range
    frames = big[:, 2:2 + H, 5:5 + W]                                            # a strip: pitch 3 (W + 8) bytes, odd for these W
    assert frames.stride(1) == 3 * (W + 8) and not frames.is_contiguous()
    want = O.input_rows(frames.cpu().numpy(), s2d, mul, add)
    oh_, ow_, c_row = want.shape[1:]
    ld = c_row + 8
    d = hip.LpipsInputDesc(frames.stride(1), frames.stride(0), n, H, W, s2d, ld, mul, add)
    assert hip.lpips_input_sides(d) == (oh_, ow_, c_row)
    ov, oh = G.guarded_out(n * oh_ * ow_, c_row, ld, torch.float16, device=DEV, guard_rows=GR)
    hip.lpips_input_rows(d, frames.data_ptr(), ov.data_ptr())
    torch.cuda.synchronize()
    G.check_written(oh)
    G.check_out(oh)
    got = oh.data.cpu().numpy().reshape(want.shape)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    if s2d == 4:                                                                 # the border: two rows and columns of zeros
        q = got.reshape(n, oh_, ow_, 4, 4, 3)
        assert not q[:, 0, :, :2].any() and not q[:, :, 0, :, :2].any() and q[:, 1:-1, 1:-1].any()
    else:
        assert not got[..., 3:].any()


# ------------------------------------------------------------------------------------------------ towers
def rel_rms(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


@pytest.mark.parametrize("net_name,H,W", [("vgg", 32, 48), ("alex", 67, 95)])
def test_towers_and_distances(hip, net_name, H, W):
    from rcdms_amd import lpips as L
    sd = O.synthetic_state_dict(net_name, 1)
    net = L.LpipsNet(sd, net_name, device=DEV, batch=8)
    rng = np.random.RandomState(7)
    a, b = (rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8) for _ in range(2))
    b[1, : H // 2] = a[1, : H // 2]                                              # a pair that agrees on half the frame
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    taps, dist = net.taps(ta, tb)
    torch.cuda.synchronize()
    taps = [t.clone() for t in taps]
    frames = np.concatenate([a, b])
    ref = O.tower(sd, net_name, O.scaled_input(frames))
    x16 = torch.from_numpy(O.input_rows(frames, 1, *net.constants)[..., :3].astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    model = O.tower(sd, net_name, x16, f16=True)
    assert [t.shape[-1] for t in taps] == list(L.TAP_CHANNELS[net_name])
    for k, (got, r, m) in enumerate(zip(taps, ref, model)):
        r, m = r.permute(0, 2, 3, 1).numpy(), m.permute(0, 2, 3, 1).numpy()
        assert tuple(got.shape) == r.shape, (k, got.shape, r.shape)
        g = got.float().cpu().numpy()
        e_model, e_kernel = rel_rms(m, r), rel_rms(g, r)
        print(f"{net_name} tap {k} {r.shape[1]}x{r.shape[2]}x{r.shape[3]}: e_model {e_model:.3e}, kernels {e_kernel:.3e}, "
              f"mean activation {np.abs(r).mean():.3f}")
        assert np.isfinite(g).all() and (g >= 0).all() and e_kernel <= 2 * e_model, (k, e_kernel, e_model)
    # the distances are rcdm_lpips_head on those taps, bit for bit
    total, layers = net(ta, tb, return_layers=True)
    assert tuple(total.shape) == (2,) and tuple(layers.shape) == (2, 5) and total.dtype == torch.float64
    layers_np = layers.cpu().numpy()
    assert O.same_bits(layers_np, dist.cpu().numpy())
    lin = O.lins(sd)
    for k, t in enumerate(taps):
        rows = t.cpu().numpy().reshape(4, -1, t.shape[-1])
        assert O.same_bits(run_head(hip, rows[:2], rows[2:], lin[k], shared=True, sides=(t.shape[1], t.shape[2])), layers_np[:, k]), k
    want_total = layers_np[:, 0] + layers_np[:, 1]
    for k in (2, 3, 4):
        want_total = want_total + layers_np[:, k]
    assert O.same_bits(total.cpu().numpy(), want_total)
    oracle = O.distance(sd, net_name, a, b)
    print(f"{net_name}: distances {layers_np.sum(1)}, fp32 oracle {oracle.sum(1)}, largest relative difference of a tap "
          f"{np.abs(layers_np / oracle - 1).max():.2e}")
    assert (layers_np > 0).all() and layers_np[1].sum() < layers_np[0].sum()
    # chunks of one pair equal one chunk of two; strips are read by their pitch; identical frames give exactly 0
    one = L.LpipsNet(sd, net_name, device=DEV, batch=1)
    assert O.same_bits(one(ta, tb, return_layers=True)[1].cpu().numpy(), layers_np) and one.plans_built == 1
    wide = torch.zeros(2, 2, H, W + 3, 3, dtype=torch.uint8, device=DEV)
    wide[0, :, :, 3:], wide[1, :, :, :W] = ta, tb
    assert O.same_bits(net(wide[0, :, :, 3:], wide[1, :, :, :W], return_layers=True)[1].cpu().numpy(), layers_np)
    same, same_layers = net(ta, ta.clone(), return_layers=True)
    assert O.same_bits(same.cpu().numpy(), np.zeros(2)) and O.same_bits(same_layers.cpu().numpy(), np.zeros((2, 5)))
    lead = net(torch.stack([ta, tb]), torch.stack([tb, tb]))                     # leading shape (2, 2)
    assert tuple(lead.shape) == (2, 2) and O.same_bits(lead[0].cpu().numpy(), total.cpu().numpy()) and not lead[1].any()


def test_small_frames_and_host_tensors_are_refused(hip):
    from rcdms_amd import lpips as L
    net = L.LpipsNet(O.synthetic_state_dict("alex", 1), "alex", device=DEV)
    small = torch.zeros(1, 30, 64, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="at least"):
        net(small, small)
    ok = torch.zeros(1, 31, 31, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="differ"):
        net(ok, torch.zeros(1, 31, 32, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(hip.RcdmError):
        net(ok.cpu(), ok.cpu())
    assert net.plans_built == 0
    assert O.same_bits(net(ok, ok).cpu().numpy(), [0.0])                         # the smallest frame runs: one pixel at tap 5
