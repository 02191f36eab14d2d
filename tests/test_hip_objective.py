"""GPU: the two kernels of the denoising objective (csrc/objective.hip) in guarded buffers (tests/guard.py: poisoned pad columns
and guard bands around every input, NaN-filled outputs), against the numpy model of tests/objective_oracle.py bit for bit and
against its exact rationals within the a-priori bound derived there.  The operands of a geometry are built once
(objective_oracle.case) and shared by every test that uses it."""
import numpy as np
import pytest
import torch

from tests import guard as G
from tests import objective_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GR = 8                                          # guard rows around every two-dimensional operand


@pytest.fixture(scope="module")
def table(hiplib):
    from rcdms_amd.scheduler import DDPMScheduler
    return DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear").noise_table().numpy()


def vec(a):
    return G.guarded_vec(torch.tensor(np.asarray(a)), device=DEV)


def gpu_rows(g, t, table, offs, ld, c_pad, scale=O.OFFS_SCALE):
    """rcdm_diffuse_assemble on guarded buffers -> uint16 [(B f H W)][c_pad]."""
    from rcdms_amd import hip
    B, _, F, H, W = g["x0"].shape
    ins = [vec(g[k]) for k in ("x0", "noise", "mask", "masked")] + [vec(np.asarray(t, np.int64)), vec(table)]
    if offs is not None:
        ins.append(vec(offs))
    (x0, _), (noise, _), (mask, _), (masked, _), (tt, _), (tab, _) = ins[:6]
    ov, oh = G.guarded_out(B * F * H * W, c_pad, ld, torch.float16, device=DEV, guard_rows=GR)
    hip.diffuse_assemble(x0.data_ptr(), noise.data_ptr(), ins[6][0].data_ptr() if offs is not None else 0, scale, tt.data_ptr(),
                         tab.data_ptr(), table.shape[0], mask.data_ptr(), masked.data_ptr(), B, F, H, W, ov.data_ptr(), ld, c_pad)
    torch.cuda.synchronize()
    G.check_out(ov)
    for v, _ in ins:
        G.check_in(v)
    return oh.data.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def gpu_sqerr(eps, noise, offs, scale, ld, blocks=0):
    """rcdm_eps_sqerr on guarded buffers -> float64 [B][f].  eps: uint16 [(B f H W)][8]."""
    from rcdms_amd import hip
    B, _, F, H, W = noise.shape
    ev, eh = G.guarded_in(torch.tensor(np.ascontiguousarray(eps).view(np.int16)).view(torch.float16), ld, device=DEV, guard_rows=GR)
    ins = [vec(noise)] + ([vec(offs)] if offs is not None else [])
    need = hip.eps_sqerr_workspace_bytes(B, F, H, W)
    assert need == B * F * O.chunks_per_frame(H * W) * 8
    sv, sh = G.guarded_out(1, B * F, B * F + 3, torch.float64, device=DEV, guard_rows=GR)
    wv, wh = G.guarded_out(1, need // 8, need // 8 + 3, torch.float64, device=DEV, guard_rows=GR)
    hip.eps_sqerr(ev.data_ptr(), ld, ins[0][0].data_ptr(), ins[1][0].data_ptr() if offs is not None else 0, scale, B, F, H, W,
                  sv.data_ptr(), wv.data_ptr(), need, blocks=blocks)
    torch.cuda.synchronize()
    G.check_out(sv)
    G.check_out(wv)
    G.check_in(ev)
    for v, _ in ins:
        G.check_in(v)
    return sh.data.contiguous().cpu().numpy().reshape(B, F)


@pytest.mark.parametrize("ld,c_pad", O.ROW_SHAPES)
@pytest.mark.parametrize("B,F,H,W", O.GEOMETRIES)
def test_rows_equal_the_model_bit_for_bit(table, B, F, H, W, ld, c_pad):
    g = O.case(B, F, H, W, table)
    assert B == 1 or len(set(g["t"].tolist())) == B                     # mixed timesteps within the batch
    for offs in (None, g["offs"]):
        got = gpu_rows(g, g["t"], table, offs, ld, c_pad)
        want = O.rows(g["x0"], g["noise"], offs, O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], c_pad)
        assert np.array_equal(got, want), (offs is None, np.argwhere(got != want)[:4])
        assert np.all(got[:, 9:] == 0)
        # the contracted form gives other rows on these inputs: the kernel rounds every product and sum on its own
        fused = O.rows(g["x0"], g["noise"], offs, O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], c_pad, form="fma")
        assert not np.array_equal(got, fused)
    # and the rows are those of the torch route: ncfhw_to_rows(cat([add_noise(x0, n, t), mask, masked], 1))
    from rcdms_amd.scheduler import DDPMScheduler
    s = DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    x0, noise, offs = (torch.tensor(g[k]).to(DEV) for k in ("x0", "noise", "offs"))
    n = noise + O.OFFS_SCALE * offs[:, :, :, None, None]
    x = torch.cat([s.add_noise(x0, n, torch.tensor(g["t"]).to(DEV)), torch.tensor(g["mask"]).to(DEV), torch.tensor(g["masked"]).to(DEV)], 1)
    route = x.permute(0, 2, 3, 4, 1).reshape(-1, 9).half().cpu().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[:, :9], route)


def test_out_of_range_timesteps_give_nan_rows(table):
    B, F, H, W = 3, 5, 3, 5
    g = O.case(B, F, H, W, table)
    base = gpu_rows(g, g["t"], table, g["offs"], 24, 16)
    per = F * H * W
    for bad in (-1, table.shape[0]):
        t = g["t"].copy()
        t[1] = bad
        got = gpu_rows(g, t, table, g["offs"], 24, 16)
        assert np.all(got[per:2 * per, :4] == O.F16_NAN) and np.array_equal(got[per:2 * per, 4:], base[per:2 * per, 4:])
        assert np.array_equal(got[:per], base[:per]) and np.array_equal(got[2 * per:], base[2 * per:])


def test_sums_on_small_integers_are_exact(hiplib):
    B, F, H, W = 3, 5, 17, 16
    rng = np.random.default_rng(5)
    noise = rng.integers(-3, 4, (B, 4, F, H, W)).astype(np.float32)
    offs = rng.integers(-1, 2, (B, 4, F)).astype(np.float32)
    eps = O.eps_rows(B, F, H, W, 5, integers=True)
    e = eps.view(np.float16).astype(np.int64)[:, :4].reshape(B, F, H * W, 4)
    for o, k in ((None, 0), (offs, 2)):
        n = np.moveaxis(noise.astype(np.int64) + k * offs.astype(np.int64)[:, :, :, None, None], 1, -1).reshape(B, F, H * W, 4)
        want = ((e - n) ** 2).sum(axis=(2, 3)).astype(np.float64)
        assert O.same_bits(gpu_sqerr(eps, noise, o, 2.0, 24), want)


@pytest.mark.parametrize("ld", [8, 24, 72])
@pytest.mark.parametrize("B,F,H,W", O.GEOMETRIES)
def test_sums_equal_the_model_and_stay_within_the_bound(table, B, F, H, W, ld):
    g = O.case(B, F, H, W, table)
    for offs in (None, g["offs"]):
        got = gpu_sqerr(g["eps"], g["noise"], offs, O.OFFS_SCALE, ld)
        assert O.same_bits(got, O.sqerr(g["eps"], g["noise"], offs, O.OFFS_SCALE))
        if ld == 8:
            exact = O.sqerr_exact(g["eps"], g["noise"], offs, O.OFFS_SCALE)
            for b in range(B):
                for f in range(F):
                    err, bound = abs(O.Fraction(float(got[b, f])) - exact[b][f]), O.bound(exact[b][f], H * W)
                    print(f"B {B} f {F} {H}x{W} ({b},{f}): error {float(err):.3e}, bound {bound:.3e}")
                    assert err <= O.Fraction(bound)


def test_every_grid_gives_the_same_bits(table):
    g = O.case(3, 5, 17, 16, table)
    want = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE)
    for blocks in (1, 5, 1000, 0):
        for _ in range(2):
            assert O.same_bits(gpu_sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE, 8, blocks=blocks), want), blocks


def test_a_nan_prediction_makes_exactly_its_frame_nan(table):
    B, F, H, W = 3, 5, 17, 16
    g = O.case(B, F, H, W, table)
    eps = g["eps"].copy()
    eps[(1 * F + 3) * H * W + 260, 2] = O.F16_NAN                       # story 1, frame 3, the tail chunk
    got = gpu_sqerr(eps, g["noise"], g["offs"], O.OFFS_SCALE, 8)
    nan = np.isnan(got)
    assert nan[1, 3] and nan.sum() == 1
    clean = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE)
    assert np.array_equal(got.view(np.int64)[~nan], clean.view(np.int64)[~nan])


@pytest.mark.parametrize("B,F,H,W", [(3, 5, 3, 5), (3, 5, 17, 16), (1, 1, 1, 1)])
def test_plausible_mistakes_change_the_result(table, B, F, H, W):
    """The kernel's results equal the model's and differ from each of the model's wrong variants, on these very inputs."""
    g = O.case(B, F, H, W, table)
    args = (g["x0"], g["noise"], g["offs"], O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], 16)
    rows = gpu_rows(g, g["t"], table, g["offs"], 24, 16)
    fused = O.rows(*args, form="fma")
    assert np.array_equal(rows, O.rows(*args)) and np.all((rows != fused).reshape(B, -1).any(axis=1))
    got = gpu_sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE, 24)
    for variant in ("no_offs", "chan4") + (("neighbour",) if F > 1 else ()):
        wrong = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE, variant=variant)
        assert np.all(wrong.view(np.int64) != got.view(np.int64)), variant


def test_shape_errors_are_refused(hiplib):
    from rcdms_amd import hip
    x = torch.zeros(64, device=DEV)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.zeros(64, dtype=torch.float16, device=DEV)
    for ld, c_pad in ((16, 8), (24, 20), (20, 16), (16, 24)):
        with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
            hip.diffuse_assemble(x.data_ptr(), x.data_ptr(), 0, 0.0, t.data_ptr(), x.data_ptr(), 10, x.data_ptr(), x.data_ptr(), 1, 1,
                                 1, 1, out.data_ptr(), ld, c_pad)
    sq = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(hip.RcdmError, match="RCDM_ESHAPE"):
        hip.eps_sqerr(out.data_ptr(), 6, x.data_ptr(), 0, 0.0, 1, 1, 1, 1, sq.data_ptr(), sq.data_ptr(), 8)
    with pytest.raises(hip.RcdmError, match="RCDM_EWORKSPACE"):
        hip.eps_sqerr(out.data_ptr(), 8, x.data_ptr(), 0, 0.0, 1, 1, 1, 1, sq.data_ptr(), sq.data_ptr(), 0)
