"""GPU: rcdms_amd.kid and the kernels under it (csrc/kid.hip), in guarded buffers (tests/guard.py).

  gram         integer X != Y with nx != ny through scattered and reversed index lists: rcdm_poly_gram_f64 equals the integer
               reference element by element, bit for bit.  Sums are invariant under row permutations, so only this pins both
               operand maps and the C/D map of the float64 MFMA.
  sums         integer features: Sxx / Syy / Sxy equal the integer sums bit for bit and mmd^2 has the model's bits, at sizes
               around the tile (with c = 1 an unmasked padded row or column adds 1 per entry), with null lists and given ones,
               1 and 3 subsets, and a list with a repeated row (the mask goes by position).  Every shape runs at a pitch that
               takes the 16-byte loads and at one that takes single elements; the pad columns hold poison.
  independence subset s of a 3-subset call has the bits of the same subset run alone; two runs of one call have the same bits.
  goldens      every golden within the a-priori bound B of tests/kid_oracle.py of the 60-digit value.
  Python       FeatureBank (growth, widening, round trip), kernel_distance with the file's indices and with `seed`, `a is b`.
  StoryRunner  feature_banks=(generated, reference) at the tiny widths of tests/test_story_metrics_gpu.py."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import guard as G
from tests import kid_oracle as O
from tests.test_hip_frechet import _Recorder, call
from tests.test_kid_host import error_to_digits
from tests.test_story_gpu import DEV, S, chain  # noqa: F401  (chain: the module-scoped fixture)

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16}
GR = 8                                          # guard rows around every operand


def pitches(d):
    """One pitch that keeps rows 16-byte aligned (the vector loads) and one that does not; both > d."""
    return ((d + 3) // 4 * 4 + 4, (d + 3) // 4 * 4 + 3)


def device_list(idx):
    return None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(DEV)


def run_mmd(hip, x, y, ia, ib, gamma, coef0, degree, dtype, ldx, ldy, m=None):
    """rcdm_poly_mmd on guarded buffers -> (subsets, 4) numpy float64.  ia, ib: (subsets, m) arrays or None (then m rows 0 .. m - 1)."""
    xv, xh = G.guarded_in(torch.from_numpy(np.asarray(x, np.float32)).to(dtype), ldx, device=DEV, guard_rows=GR)
    yv, yh = G.guarded_in(torch.from_numpy(np.asarray(y, np.float32)).to(dtype), ldy, device=DEV, guard_rows=GR)
    subsets, m = (1, m) if ia is None else ia.shape
    desc = hip.MmdDesc(ldx, ldy, x.shape[0], y.shape[0], x.shape[1], subsets, m, degree,
                       hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32, gamma, coef0, 0)
    need = hip.poly_mmd_workspace_bytes(desc)
    assert need == subsets * 3 * O.tiles(m) ** 2 * 8
    ov, oh = G.guarded_out(subsets, 4, 4, torch.float64, device=DEV, guard_rows=GR)
    wv, wh = G.guarded_out(1, need // 8, need // 8 + 3, torch.float64, device=DEV, guard_rows=GR)
    la, lb = device_list(ia), device_list(ib)
    hip.poly_mmd(desc, xv.data_ptr(), yv.data_ptr(), hip.ptr(la), hip.ptr(lb), ov.data_ptr(), wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_written(oh)
    G.check_written(wh)
    return oh.data.cpu().numpy(), (xh, yh, oh, wh)


def run_gram(hip, x, y, ia, ib, gamma, coef0, degree, dtype, ldx, ldy):
    xv, xh = G.guarded_in(torch.from_numpy(np.asarray(x, np.float32)).to(dtype), ldx, device=DEV, guard_rows=GR)
    yv, yh = G.guarded_in(torch.from_numpy(np.asarray(y, np.float32)).to(dtype), ldy, device=DEV, guard_rows=GR)
    subsets, m = ia.shape
    desc = hip.MmdDesc(ldx, ldy, x.shape[0], y.shape[0], x.shape[1], subsets, m, degree,
                       hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32, gamma, coef0, 0)
    ov, oh = G.guarded_out(m, m, m + 5, torch.float64, device=DEV, guard_rows=GR)
    la, lb = device_list(ia), device_list(ib)
    hip.poly_gram_f64(desc, xv.data_ptr(), yv.data_ptr(), la.data_ptr(), lb.data_ptr(), ov.data_ptr(), m + 5)
    torch.cuda.synchronize()
    G.check_written(oh)
    return oh.data.cpu().numpy(), (xh, yh, oh)


def scattered_lists(m, nx, ny, subsets, seed):
    """ia: a reversed stretch of X's rows; ib: a random scatter of Y's."""
    rng = np.random.RandomState(seed)
    ia = np.stack([np.arange(nx - 1 - s, nx - 1 - s - m, -1) for s in range(subsets)])
    ib = np.stack([rng.permutation(ny)[:m] for _ in range(subsets)])
    return ia.astype(np.int32), ib.astype(np.int32)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("m", [2, 17, 64, 65])
def test_gram_exact(hiplib, m, dtype):
    from rcdms_amd import hip
    for d in (1, 3, 5, 16, 130):
        gamma, den = O.integer_gamma(d)
        nx, ny = m + 7, m + 3
        x, y = O.integer_features(nx, d, 100 * m + d), O.integer_features(ny, d, 200 * m + d)
        y[:, 0] += 2                                         # nothing about Y is shared with X; still exact in float16
        ia, ib = scattered_lists(m, nx, ny, 2, m + d)        # the entry uses the first subset only
        _, grams = O.integer_reference(x, y, ia[:1], ib[:1], den, 1, 3)
        for ld in pitches(d):
            got, handles = run_gram(hip, x, y, ia, ib, gamma, 1.0, 3, DTYPES[dtype], ld, ld + 4)
            assert O.same_bits(got, grams[0]), (d, ld, np.argwhere(got != grams[0])[:4])
            G.check_all(*handles)


@pytest.mark.parametrize("m", [2, 3, 17, 63, 64, 65, 97])
def test_sums_exact(hiplib, m):
    from rcdms_amd import hip
    for n, d in enumerate((1, 3, 5, 16, 48, 130)):
        dtype = (torch.float32, torch.float16)[(n + m) & 1]
        gamma, den = O.integer_gamma(d)
        nx, ny = m + 6, m + 1
        x, y = O.integer_features(nx, d, 300 * m + d), O.integer_features(ny, d, 400 * m + d)
        ia, ib = scattered_lists(m, nx, ny, 3, m + d)
        sums, _ = O.integer_reference(x, y, ia, ib, den, 1, 3)
        ident = np.arange(m, dtype=np.int32)[None, :]
        plain, _ = O.integer_reference(x, y, ident, ident, den, 1, 3)
        for ld in pitches(d):
            got, handles = run_mmd(hip, x, y, ia, ib, gamma, 1.0, 3, dtype, ld, ld + 4)
            assert O.same_bits(got[:, :3], sums), (d, ld, got[:, :3], sums)
            assert O.same_bits(got[:, 3], [O.mmd2(*row, m) for row in sums])
            G.check_all(*handles)
            got, handles = run_mmd(hip, x, y, None, None, gamma, 1.0, 3, dtype, ld + 4, ld, m=m)      # null lists, one subset
            assert O.same_bits(got[:, :3], plain) and O.same_bits(got[:, 3], [O.mmd2(*plain[0], m)])
            G.check_all(*handles)


def test_the_mask_goes_by_position(hiplib):
    from rcdms_amd import hip
    x, y = O.integer_features(12, 5, 1), O.integer_features(9, 5, 2)
    ia, ib = np.array([[4, 9, 4, 1, 4]], np.int32), np.array([[0, 1, 2, 3, 3]], np.int32)       # row 4 three times, row 3 twice
    sums, _ = O.integer_reference(x, y, ia, ib, 1, 1, 3)
    got, handles = run_mmd(hip, x, y, ia, ib, 1.0, 1.0, 3, torch.float32, 8, 7)
    assert O.same_bits(got[:, :3], sums)
    G.check_all(*handles)
    # a mask by row number would drop the six ordered pairs of positions that hold row 4, and the two that hold row 3 of Y
    k44, k33 = (int((x[4] * x[4]).sum()) + 1) ** 3, (int((y[3] * y[3]).sum()) + 1) ** 3
    assert k44 > 0 and k33 > 0 and got[0, 0] != sums[0, 0] - 6 * k44 and got[0, 1] != sums[0, 1] - 2 * k33


def test_subsets_are_independent_and_runs_repeat(hiplib):
    from rcdms_amd import hip
    g = O.load("subsets3")
    args = (float(g["gamma"]), float(g["coef0"]), int(g["degree"]), torch.float32, 12, 16)
    all3, handles = run_mmd(hip, g["x"], g["y"], g["ia"], g["ib"], *args)
    G.check_all(*handles)
    again, _ = run_mmd(hip, g["x"], g["y"], g["ia"], g["ib"], *args)
    assert O.same_bits(all3, again)
    for s in range(3):
        alone, _ = run_mmd(hip, g["x"], g["y"], g["ia"][s:s + 1], g["ib"][s:s + 1], *args)
        assert O.same_bits(alone[0], all3[s])
    big = O.load("m65_d130")                                     # four tiles, one of them doubled
    a1, _ = run_mmd(hip, big["x"], big["y"], big["ia"], big["ib"], float(big["gamma"]), 1.0, 3, torch.float32, 132, 133)
    a2, _ = run_mmd(hip, big["x"], big["y"], big["ia"], big["ib"], float(big["gamma"]), 1.0, 3, torch.float32, 132, 133)
    assert O.same_bits(a1, a2)


@pytest.mark.parametrize("name", list(O.CASES))
def test_against_the_goldens(hiplib, name):
    from rcdms_amd import hip
    g = O.load(name)
    d = g["x"].shape[1]
    B = g["bound"]
    for dtype in ([torch.float32, torch.float16] if name == "f16" else [torch.float32]):
        for ld in pitches(d):
            got, handles = run_mmd(hip, g["x"], g["y"], g["ia"], g["ib"], float(g["gamma"]), float(g["coef0"]), int(g["degree"]),
                                   dtype, ld, ld)
            for s in range(got.shape[0]):
                err = error_to_digits(got[s, 3], g["mp_digits"][s, 3])
                print(f"{name}[{s}] ld {ld}: kernel {got[s, 3]:.17g}, mpmath {g['mp_digits'][s, 3]}, |diff| {err:.3e} = {err / B[s]:.2e} B")
                assert err <= B[s]
            G.check_all(*handles)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_feature_bank(hiplib):
    from rcdms_amd.kid import FeatureBank
    g = O.load("f16")
    x = torch.from_numpy(np.concatenate([g["x"], g["y"]] * 5)).to(DEV)              # 200 rows of 24
    bank = FeatureBank(24, DEV)
    wide = torch.full((40, 30), G.POISON, device=DEV)
    wide[:, :24] = x[:40]
    bank.append(wide[:, :24])                                                       # rows of another pitch
    first = bank.rows().data_ptr()
    bank.append(x[40:60].to(torch.float16).reshape(4, 5, 24))                       # leading axes; float16 widened exactly
    bank.append(x[60:200])                                                          # past the first capacity: the buffer grows
    assert len(bank) == 200 and bank.rows().data_ptr() != first and bank.rows().dtype == torch.float32
    assert torch.equal(bank.rows(), x)
    with pytest.raises(ValueError):
        bank.append(torch.zeros(3, 23, device=DEV))
    with pytest.raises(ValueError):
        FeatureBank(24, DEV, dtype=torch.float16).append(x[:3])                     # float32 into a float16 bank
    half = FeatureBank(24, DEV, dtype=torch.float16).append(x[:7].to(torch.float16))
    assert half.rows().dtype == torch.float16 and torch.equal(half.rows().float(), x[:7])
    st = bank.stats()
    assert st.n == 200 and float((st.mean() - x.double().mean(dim=0)).abs().max()) <= 1e-12
    with tempfile.TemporaryDirectory() as tmp:
        bank.save(os.path.join(tmp, "bank.npz"))
        with np.load(os.path.join(tmp, "bank.npz")) as z:
            assert z.files == ["features"]
        back = FeatureBank.load(os.path.join(tmp, "bank.npz"), DEV)
    assert torch.equal(back.rows(), bank.rows())
    assert len(bank.clear()) == 0 and len(bank.append(x[:3])) == 3


def test_kernel_distance(hiplib):
    from rcdms_amd.kid import FeatureBank, draw_subsets, kernel_distance, polynomial_mmd
    g = O.load("subsets3")
    a = FeatureBank(12, DEV).append(torch.from_numpy(g["x"]).to(DEV))
    b = FeatureBank(12, DEV).append(torch.from_numpy(g["y"]).to(DEV))
    r = kernel_distance(a, b, indices=(g["ia"], g["ib"]))
    assert (r.subsets, r.subset_size) == (3, 19) and len(r.values) == 3
    for s in range(3):
        assert error_to_digits(r.values[s], g["mp_digits"][s, 3]) <= g["bound"][s]
    assert (r.mean, r.std) == O.kid(r.values)
    seeded = kernel_distance(a, b, subsets=3, subset_size=19, seed=7)                # the draws the file pins
    assert seeded.values == r.values and (seeded.mean, seeded.std) == (r.mean, r.std)
    dev = kernel_distance(a.rows(), b.rows(), indices=(torch.from_numpy(g["ia"]).to(DEV), torch.from_numpy(g["ib"]).to(DEV)))
    assert dev.values == r.values
    default = kernel_distance(a, b, subsets=4)                                      # subset_size None: min(1000, 31, 45)
    assert default.subset_size == 31 and default.subsets == 4 and np.isfinite(default.mean)
    out = polynomial_mmd(a.rows(), b.rows())
    assert tuple(out.shape) == (1, 4) and out.dtype == torch.float64 and out.is_cuda
    for bad in (np.array([[0, 31]]), np.array([[-1, 3]])):
        with pytest.raises(ValueError):
            kernel_distance(a, b, indices=(bad, np.array([[0, 1]])))
    with pytest.raises(ValueError):
        kernel_distance(a, b, indices=(torch.tensor([[0, 31]], device=DEV), torch.tensor([[0, 1]], device=DEV)))
    with pytest.raises(ValueError):
        kernel_distance(a, b, subset_size=32)
    # a is b: the same object on both sides
    same = kernel_distance(a, a, subsets=2, subset_size=10, seed=3)
    ia, ib = draw_subsets(31, 31, 2, 10, 3)
    want = O.evaluate(g["x"], g["x"], ia, ib, 1.0 / 12, 1.0, 3)
    bounds = O.bound(g["x"], g["x"], ia, ib, 1.0 / 12, 1.0, 3)
    for s in range(2):
        assert abs(same.values[s] - want[s, 3]) <= 2.0 * bounds[s]                  # two evaluations inside the rules


# ------------------------------------------------------------------------------------------------ StoryRunner
def test_story_runner_feature_banks(chain):
    from rcdms_amd.frechet import FeatureStats
    from rcdms_amd.kid import FeatureBank, kernel_distance
    b = chain
    gen, ref = FeatureBank(b.E, DEV), FeatureBank(b.E, DEV)
    sgen, sref = FeatureStats(b.E, DEV), FeatureStats(b.E, DEV)
    rec = _Recorder(b.runner.image_encoder)
    b.runner.image_encoder = rec
    try:
        res = call(b, metrics=("clip_i",), feature_stats=(sgen, sref), feature_banks=(gen, ref))
    finally:
        b.runner.image_encoder = rec.inner
    off = call(b, metrics=("clip_i",))
    assert len(gen) == 5 * S and len(ref) == 5 * S and sgen.n == 5 * S
    assert torch.equal(res.videos, off.videos) and torch.equal(res.clip_i, off.clip_i)
    assert sum(1 for e in rec.embeds if e.shape[0] == S * 5) == 2            # the targets and the generated frames, no third forward
    fed = rec.embeds[-1]
    assert torch.equal(gen.rows(), fed.reshape(S * 5, -1).float()) and torch.equal(ref.rows(), res.target_embeds.reshape(S * 5, -1).float())
    # the rows feature_stats saw in the same call: the same sums to the bit
    for bank, st in ((gen, sgen), (ref, sref)):
        again = FeatureStats(b.E, DEV, shift=st.shift).update(bank.rows())       # widening is exact: float32 rows, the same values
        assert torch.equal(again.sum, st.sum) and torch.equal(again.outer, st.outer)
    r = kernel_distance(gen, ref, subsets=5)
    print(f"story CLIP-KID over {len(gen)} frames at E = {b.E}: {r.mean:.6g} +- {r.std:.3g} (subsets of {r.subset_size})")
    assert r.subset_size == 5 * S and np.isfinite(r.mean) and r.std >= 0.0
    only = call(b, feature_banks=(gen, ref))
    assert only.clip_i is None and len(gen) == 10 * S
    with pytest.raises(ValueError, match="uint8"):
        call(b, feature_banks=(gen, ref), output_type="tensor")
    with pytest.raises(ValueError, match="stage 2"):
        call(b, feature_banks=(gen, ref), stage2=False)
