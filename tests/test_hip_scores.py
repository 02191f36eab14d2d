"""GPU: rcdms_amd.scores and the kernels under it (csrc/scores.hip), in guarded buffers (tests/guard.py; label bytes are guarded by
255s, which read as "present").

  label counts     the state equals Python-int arithmetic bit for bit at C in {1, 7, 9, 64} x N in {1, 63, 64, 65, 255, 256, 257,
                   1000} (one to four blocks of 256 rows), float32 and float16 logits at row strides above C, logits exactly at
                   the threshold, NaN logits, label bytes 0 / 1 / 255, per-class thresholds, all-negative rows and a
                   never-present class; the call ADDS into a non-zero state; each plausible mistake (">=", a NaN predicting 1, a
                   label read as == 1) would have changed a count on the same inputs.
  LabelCounts      leading axes, strided rows, bool labels; two updates equal one update of the concatenation; merge; save / load;
                   result() against the exact fractions of tests/scores_oracle.py for both zero_division values.
  Inception Score  every golden (C in {2, 7, 1000, 1008} x splits in {1, 3, 10} x N in {splits, 23, 257}, float16-representable
                   logits, logits across +-80, an order list, identical rows) within the a-priori bound B of the 60-digit value;
                   the same bits on a rerun, for every chunks_per_block, and for float16 against float32 storage of the same
                   values; order / shuffle_seed / a FeatureBank through the Python layer; refusals."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import guard as G
from tests import scores_oracle as O
from tests.test_scores_host import error_to_digits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16}
GR = 8                                          # guard rows around every operand
LABEL_N = (1, 63, 64, 65, 255, 256, 257, 1000)


def guarded_labels(y, ld):
    """uint8 labels in the middle of 255s (every guard byte says "present")."""
    n, C = y.shape
    buf = torch.full((n + 2 * GR, ld), 255, dtype=torch.uint8, device=DEV)
    buf[GR:GR + n, :C] = torch.from_numpy(y).to(DEV)
    return buf[GR:GR + n], buf, buf.clone()


def run_counts(hip, z, y, thr, dtype, ldz, ldl, start=None):
    """rcdm_label_counts on guarded buffers -> the int64 state as numpy.  start: the state before the call (default zeros)."""
    n, C = z.shape
    zv, zh = G.guarded_in(torch.from_numpy(z).to(dtype), ldz, device=DEV, guard_rows=GR)
    yv, ybuf, ysnap = guarded_labels(y, ldl)
    tv, th = (None, None) if thr is None else G.guarded_vec(torch.from_numpy(thr), device=DEV)
    L = hip.label_state_len(C)
    assert L == O.state_len(C)
    sv, sh = G.guarded_out(1, L, L + 3, torch.int64, device=DEV, guard_rows=GR)
    sh.data[0] = torch.zeros(L, dtype=torch.int64) if start is None else torch.from_numpy(start)
    desc = hip.LabelDesc(ldz, ldl, n, C, hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32, 0)
    need = hip.label_counts_workspace_bytes(desc)
    assert need == (-(-n // O.LABEL_ROWS) * L * 4 + 7) // 8 * 8
    wv, wh = G.guarded_out(1, need // 4, need // 4 + 5, torch.int32, device=DEV, guard_rows=GR)
    hip.label_counts(desc, zv.data_ptr(), yv.data_ptr(), hip.ptr(tv), sv.data_ptr(), wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_in(zh)
    G.check_out(sh)
    G.check_out(wh)
    if th is not None:
        G.check_in(th)
    assert torch.equal(ybuf, ysnap), "the labels changed"
    return sh.data[0].cpu().numpy()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("C", [1, 7, 9, 64])
def test_label_state_exact(hiplib, C, dtype):
    from rcdms_amd import hip
    seen = {"ge": 0, "nan1": 0, "label1": 0}
    for n in LABEL_N:
        for thresholds in (False, True):
            z, y, thr = O.label_inputs(C, n, 100 * C + n, thresholds=thresholds)
            want = O.label_state(z, y, thr)
            got = run_counts(hip, z, y, thr, DTYPES[dtype], C + 3, C + 5)
            assert got.dtype == np.int64 and np.array_equal(got, want), (n, thresholds, np.flatnonzero(got != want)[:8])
            for rule in seen:
                seen[rule] += not np.array_equal(O.label_state(z, y, thr, rule=rule), want)
    assert all(v > 0 for v in seen.values()), seen          # each mistake would have changed a count on these inputs


def test_label_goldens_blocks_and_accumulation(hiplib):
    from rcdms_amd import hip
    for name in O.LABEL_CASES:
        g = O.load_labels(name)
        C = g["logits"].shape[1]
        for dtype in (torch.float32, torch.float16):
            assert np.array_equal(run_counts(hip, g["logits"], g["labels"], g.get("thresholds"), dtype, C, C), g["state"])       # dense rows
    z, y, thr = O.label_inputs(9, 2500, 77, thresholds=True)              # ten blocks of 256 rows, the last ragged
    want = O.label_state(z, y, thr)
    assert np.array_equal(run_counts(hip, z, y, thr, torch.float32, 12, 16), want)
    start = np.arange(O.state_len(9), dtype=np.int64) * 1_000_000_007      # the call adds: nothing is zeroed, nothing is 32-bit
    assert np.array_equal(run_counts(hip, z, y, thr, torch.float16, 10, 9, start=start), want + start)


def test_label_counts_python_layer(hiplib):
    from rcdms_amd.scores import LabelCounts
    C = 9
    z, y, thr = O.label_inputs(C, 5 * 40, 5, thresholds=True)
    want = O.label_state(z, y, thr)
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    wide = torch.full((200, C + 4), G.POISON, device=DEV)
    wide[:, :C] = zt
    whole = LabelCounts(C, DEV, thr).update(wide[:, :C], yt)               # rows of another pitch
    assert whole.state().dtype == torch.int64 and np.array_equal(whole.state().cpu().numpy(), want)
    stories = LabelCounts(C, DEV, thr).update(zt.reshape(40, 5, C).half(), (yt != 0).reshape(40, 5, C))      # leading axes, f16, bool
    assert torch.equal(stories.state(), whole.state())
    two = LabelCounts(C, DEV, thr).update(zt[:77], yt[:77]).update(zt[77:], yt[77:])
    assert torch.equal(two.state(), whole.state())                          # two updates are one update of the concatenation
    a, b = LabelCounts(C, DEV, thr).update(zt[:120], yt[:120]), LabelCounts(C, DEV, thr).update(zt[120:], yt[120:])
    assert torch.equal(a.merge(b).state(), whole.state())
    frames = zt.reshape(40, 5, C)[:, 1:], yt.reshape(40, 5, C)[:, 1:]       # frames 1 .. 4 of every story: a strided view
    part = LabelCounts(C, DEV, thr).update(*frames)
    keep = np.arange(200).reshape(40, 5)[:, 1:].reshape(-1)
    assert np.array_equal(part.state().cpu().numpy(), O.label_state(z[keep], y[keep], thr))
    with tempfile.TemporaryDirectory() as tmp:
        whole.save(os.path.join(tmp, "counts.npz"))
        with np.load(os.path.join(tmp, "counts.npz")) as f:
            assert sorted(f.files) == ["label_state", "thresholds"] and np.array_equal(f["label_state"], want)
        back = LabelCounts.load(os.path.join(tmp, "counts.npz"), DEV)
    assert back.num_classes == C and torch.equal(back.state(), whole.state()) and np.array_equal(back.thresholds, thr)
    assert torch.equal(back.update(zt[:3], yt[:3]).state(), whole.update(zt[:3], yt[:3]).state())
    for zd in (0, 1):
        r, exact = two.result(zero_division=zd), O.figures(want, C, zd)
        for key in ("frame_accuracy", "f1_micro", "f1_macro", "f1_weighted", "f1_samples", "hamming"):
            assert abs(getattr(r, key) - exact[key]) <= 2 * O.U, key
        assert np.array_equal(r.f1, exact["f1"]) and np.array_equal(r.support, exact["support"]) and r.n == 200
        assert r.support[C - 1] == 0 and r.recall[C - 1] == float(zd)      # the never-present class: 0 / 0
    assert not two.clear().state().any() and np.array_equal(two.update(zt, yt).state().cpu().numpy(), want)
    for bad in ((zt[:, :8], yt[:, :8]), (zt, yt[:100]), (zt.double(), yt), (zt, yt.int()), (zt[:0], yt[:0])):
        with pytest.raises(ValueError):
            two.update(*bad)
    assert np.array_equal(two.state().cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ Inception Score
def run_isc(hip, z, splits, order, dtype, ld, cpb=0, row_h=True):
    """rcdm_inception_score on guarded buffers -> (kl (splits,), row_h (n,) or None) as numpy."""
    n, C = z.shape
    zv, zh = G.guarded_in(torch.from_numpy(z).to(dtype), ld, device=DEV, guard_rows=GR)
    ot = None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(DEV)
    desc = hip.IscDesc(ld, n, C, splits, hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32, cpb, 0)
    need = hip.inception_score_workspace_bytes(desc)
    assert need == (3 * n + splits * O.chunks(-(-n // splits)) * (C + 1)) * 8
    kv, kh = G.guarded_out(1, splits, splits + 3, torch.float64, device=DEV, guard_rows=GR)
    hv, hh = G.guarded_out(1, n, n + 1, torch.float64, device=DEV, guard_rows=GR)
    wv, wh = G.guarded_out(1, need // 8, need // 8 + 3, torch.float64, device=DEV, guard_rows=GR)
    hip.inception_score(desc, zv.data_ptr(), hip.ptr(ot), kv.data_ptr(), hv.data_ptr() if row_h else 0, wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_written(kh)
    G.check_all(zh, kh, hh, wh)
    if row_h:
        G.check_written(hh)
    return kh.data[0].cpu().numpy(), hh.data[0].cpu().numpy() if row_h else None


@pytest.mark.parametrize("C", sorted({v[0] for v in O.ISC_CASES.values()}))
def test_isc_against_the_goldens(hiplib, C):
    from rcdms_amd import hip
    worst = 0.0
    for name, (c, n, splits, variant) in O.ISC_CASES.items():
        if c != C:
            continue
        g = O.load_isc(name)
        B = g["bound"]
        for dtype in ([torch.float32, torch.float16] if variant == "f16" else [torch.float32]):
            for ld in (C, C + 3):
                got, row_h = run_isc(hip, g["logits"], splits, g["order"], dtype, ld)
                for k in range(splits):
                    err = error_to_digits(got[k], g["kl_digits"][k])
                    worst = max(worst, err / B[k])
                    print(f"{name}[{k}] ld {ld}: kernel {got[k]:.17g}, mpmath {g['kl_digits'][k]}, |diff| {err:.3e} = {err / B[k]:.2e} B")
                    assert err <= B[k]
                rows = np.arange(n) if g["order"] is None else g["order"]
                h = O.row_stats(g["logits"].astype(np.float64))[2][rows]
                assert np.all(np.abs(row_h - h) <= 2 * B.max())          # a_h, the rows' share of B, on either side
    print(f"C {C}: worst |kernel - mpmath| / B = {worst:.2e}")


def test_isc_same_bits_whatever_the_geometry(hiplib):
    from rcdms_amd import hip
    z = O.isc_logits(7, 1300)                                 # two splits of 650 positions: three chunks each, the last ragged
    base, base_h = run_isc(hip, z, 2, None, torch.float32, 8)
    assert np.all(np.abs(base - O.evaluate(z, 2)) <= 2 * O.bound(z, 2))
    for cpb in (0, 1, 2, 3, 64):
        got, row_h = run_isc(hip, z, 2, None, torch.float32, 8, cpb=cpb)
        assert O.same_bits(got, base) and O.same_bits(row_h, base_h), cpb
    other, _ = run_isc(hip, z, 2, None, torch.float32, 11, row_h=False)        # another pitch, no row_h
    assert O.same_bits(other, base)
    g = O.load_isc("c1008_n257_s1")                           # two chunks over four class blocks
    a = [run_isc(hip, g["logits"], 1, None, torch.float32, 1008, cpb=cpb)[0] for cpb in (0, 2, 0)]
    assert O.same_bits(a[0], a[1]) and O.same_bits(a[0], a[2])
    g = O.load_isc("f16_c100_n23_s3")                         # float16 storage widens exactly
    assert O.same_bits(run_isc(hip, g["logits"], 3, None, torch.float16, 104)[0], run_isc(hip, g["logits"], 3, None, torch.float32, 100)[0])
    # the splits are independent: split k of a three-split call over rows it alone sees
    g = O.load_isc("c7_n257_s3")
    all3, _ = run_isc(hip, g["logits"], 3, None, torch.float32, 7)
    for k, (b0, b1) in enumerate(O.split_bounds(257, 3)):
        assert O.same_bits(run_isc(hip, g["logits"][b0:b1], 1, None, torch.float32, 7)[0], all3[k:k + 1])


def test_inception_score_python_layer(hiplib):
    from rcdms_amd import hip
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.scores import inception_score
    g = O.load_isc("order_c7_n257_s10")
    z = torch.from_numpy(g["logits"]).to(DEV)
    low, _ = run_isc(hip, g["logits"], 10, g["order"], torch.float32, 7)
    r = inception_score(z, splits=10, shuffle_seed=O.ORDER_SEED)
    assert O.same_bits(np.array(r.kl), low) and len(r.scores) == 10
    assert (r.mean, r.std, r.scores) == O.isc(r.kl)
    for k in range(10):
        assert error_to_digits(r.kl[k], g["kl_digits"][k]) <= g["bound"][k]
    assert inception_score(z, splits=10, order=g["order"]).kl == r.kl
    assert inception_score(z, splits=10, order=torch.from_numpy(g["order"]).to(DEV)).kl == r.kl
    plain = inception_score(z, splits=10)
    assert plain.kl != r.kl and O.same_bits(np.array(plain.kl), run_isc(hip, g["logits"], 10, None, torch.float32, 7)[0])
    bank = FeatureBank(7, DEV).append(z[:100]).append(z[100:])
    assert inception_score(bank, splits=10).kl == plain.kl
    wide = torch.full((257, 12), G.POISON, device=DEV)
    wide[:, :7] = z
    assert inception_score(wide[:, :7], splits=10, chunks_per_block=4).kl == plain.kl          # strided rows
    assert inception_score(z.half(), splits=3).kl == inception_score(z.half().float(), splits=3).kl
    one = inception_score(z[:1], splits=1)                    # a single row is its own mean
    assert abs(one.kl[0]) <= O.bound(g["logits"][:1], 1)[0] and one.std == 0.0
    eq = O.load_isc("equal_c7_n23_s3")
    flat = inception_score(torch.from_numpy(eq["logits"]).to(DEV), splits=3)
    assert all(abs(v) <= b for v, b in zip(flat.kl, eq["bound"])) and abs(flat.mean - 1.0) <= 2 * eq["bound"].max()
    # refusals: the Python layer's and the entry point's own
    for bad, kw in ((z, {"splits": 258}), (z[:, :1], {}), (z.double(), {}), (z, {"order": np.arange(256)}),
                    (z, {"order": np.arange(257), "shuffle_seed": 0}), (z, {"chunks_per_block": -1})):
        with pytest.raises(ValueError):
            inception_score(bad, **kw)
    desc = hip.IscDesc(7, 257, 7, 10, hip.FSTATS_F32, 0, 0)
    need = hip.inception_score_workspace_bytes(desc)
    ws, out = torch.empty(need, dtype=torch.uint8, device=DEV), torch.full((10,), float("nan"), dtype=torch.float64, device=DEV)
    with pytest.raises(hip.RcdmError, match="EWORKSPACE"):
        hip.inception_score(desc, z.data_ptr(), 0, out.data_ptr(), 0, ws.data_ptr(), need - 8)
    with pytest.raises(hip.RcdmError, match="EINVAL"):
        hip.inception_score(hip.IscDesc(7, 257, 7, 258, hip.FSTATS_F32, 0, 0), z.data_ptr(), 0, out.data_ptr(), 0, ws.data_ptr(), need)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                             # refused before anything was launched
