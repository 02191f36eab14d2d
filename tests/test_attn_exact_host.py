"""CPU: the exact-answer assertions of tests/test_hip_attn_exact.py against a numpy model of the attention kernels' softmax
(tests/attn_exact.py), in the manner of tests/test_guard.py: the model that normalises by the sum of the ROUNDED
probabilities passes them on every shape the GPU test launches, the model that normalises by the unrounded sum (what
flash_attn_kernel and xattn_kernel did at d = 32 and d = 160) fails them, and stand-ins with a key-index slip, a column
permutation or a dropped mask fail the selection assertion.  Also the preconditions the GPU test's reasoning rests on: every
input is exactly representable in f16, every selection input has its score gap (float64)."""
import numpy as np
import pytest

from tests import attn_exact as X

ENTRIES = ("flash", "masked", "xattn", "wide", "temporal")


def _unity_case(entry, d, Lq, Lk, mode, gain):
    """q, k, v, valid, causal, batch of one unity launch, in the [batch][L][heads*d] layout (temporal: one problem per pixel)."""
    batch = X.BATCH * X.TEMPORAL_PIXELS if entry == "temporal" else X.BATCH
    q, k = X.unity_qk(entry, d, Lq, Lk, mode, gain, batch=batch)
    v = X.unity_v(batch * Lk, X.HEADS, d).reshape(batch, Lk, X.HEADS * d)
    valid, causal = X.unity_mask(d, Lk, mode) if mode else (None, False)
    return q, k, v, valid, causal


@pytest.mark.parametrize("entry", ENTRIES)
def test_unity_models(entry):
    """Consistent normalisation: zero mismatching elements on every shape, gain and mask.  Inconsistent normalisation: caught.
    What "caught" can mean follows from the defect: out = c_j (1 - delta), delta = sum(p - round(p)) / sum(p), and c_j is a power
    of two, under which f16 values lie c_j 2^-11 apart: the element leaves c_j when delta > 2^-12.  A row with a single visible key
    has p = 1, delta = 0: the two models are the same function there (Lk = 1, frames = 1, query 0 of a causal mask), and with a
    handful of keys delta stays below 2^-12 because the largest p is exactly 1; the mean loss of round-toward-zero is about
    2^-11.5 of the sum, so from a few dozen keys on most rows leave.  Asserted: identical output where every row sees one key; at
    least one element at every gain wherever >= 33 rows see >= 32 keys (the Lq = 1 launches have two rows here); more than half of the elements at gain 1 where every row sees
    >= 64 keys."""
    cases = [c for c in X.unity_cases() if c[0] == entry]
    assert cases
    n_sub = n_p = 0
    for _, d, Lq, Lk, mode in cases:
        for gain in X.GAINS:
            q, k, v, valid, causal = _unity_case(entry, d, Lq, Lk, mode, gain)
            for a in (q, k, v):
                assert X.is_f16_exact(a), (entry, d, Lq, Lk, mode, gain)
            if mode is None:                 # the model treats every (batch, head) alike: the first batch entry (temporal: the
                n = 1 if entry != "temporal" else 8          # first pixels) of the GPU test's inputs is enough
                q, k, v = q[:n], k[:n], v[:n]
            good, p_good = X.model_rows(q, k, v, X.HEADS, d, True, valid, causal)
            bad, _ = X.model_rows(q, k, v, X.HEADS, d, False, valid, causal)
            n_good, n_bad = X.unity_mismatches(good, X.HEADS, d), X.unity_mismatches(bad, X.HEADS, d)
            what = f"{entry} d={d} Lq={Lq} Lk={Lk} mask={mode} gain={gain}: {n_bad} / {bad.size} elements"
            assert n_good == 0, f"consistent model: {n_good} mismatches, {what}"
            if Lk == 1:
                assert n_bad == 0 and np.array_equal(good.view(np.uint16), bad.view(np.uint16)), what
            elif Lk >= 32 and good.shape[0] >= 33:
                assert n_bad >= 1, what
            if gain == 1 and Lk >= 64 and mode is None:
                assert 2 * n_bad > bad.size, what
            if gain == 3 and Lk >= 64 and mode is None:
                sub = (p_good > 0) & (p_good < np.float16(2.0 ** -14))
                assert sub.any(), f"{what}: no f16 subnormal among the rounded probabilities"
                n_sub, n_p = n_sub + int(sub.sum()), n_p + sub.size
    # the gain-3 inputs are there for the f16 subnormals among the rounded probabilities: a row sum that drops them (or a matrix
    # pipe that does) must show.  scores ~ 3 N(0, 1): p < 2^-14 = e^-9.7 for every score more than 9.7 below the row max, itself
    # ~ 3 * (2.3 .. 3.2) over 64 .. 1000 keys — z < -0.9 .. 0: between 18 % and half of the keys
    if n_p:
        print(f"{entry}: {n_sub / n_p:.3f} of the rounded probabilities at gain 3, Lk >= 64 are f16 subnormals")
        assert n_sub > 0.15 * n_p, f"{entry}: only {n_sub / n_p:.3f} of the gain-3 probabilities are f16 subnormals"


def test_unity_mask_leaves_every_query_a_key():
    for d in X.MASKED_D:
        for L in X.MASKED_L:
            for mode in X.MASKED_MODES:
                valid, causal = X.unity_mask(d, L, mode)
                for b in range(X.BATCH):
                    vis = X.visible(None if valid is None else valid[b], causal, L, L)
                    assert vis.any(axis=1).all(), (d, L, mode, b)
                if valid is not None and not causal:
                    assert not valid[:, 0].any() and not valid[1, :64].any()   # key 0 hidden; a whole first key tile hidden


def _selection_cases():
    """name, q, k, v, heads, d, pi, valid, causal, planted of every selection launch (temporal: in problem layout)."""
    out = []
    for entry, table in (("flash", X.SEL_FLASH), ("xattn", X.SEL_XATTN), ("wide", X.SEL_WIDE)):
        for d, Lq, Lk in table:
            q, k, v, pi = X.sel_case(entry, d, Lq, Lk)
            out.append((f"{entry} d={d} Lq={Lq} Lk={Lk}", q, k, v, d, pi, None, False, None))
    for d, frames in X.SEL_TEMPORAL:
        q, k, v, pi = X.sel_temporal_case(d, frames)
        out.append((f"temporal d={d} frames={frames}", q, k, v, d, pi, None, False, None))
    for d, L, pad, causal in X.SEL_MASKED:
        q, k, v, valid, pi, planted = X.sel_masked_case(d, L, pad, causal)
        out.append((f"masked d={d} L={L} pad={pad} causal={causal}", q, k, v, d, pi, valid, causal, planted))
    return out


@pytest.fixture(scope="module")
def selection_cases():
    return _selection_cases()


def test_selection_inputs_have_the_gap_and_are_f16_exact(selection_cases):
    for name, q, k, v, d, pi, valid, causal, planted in selection_cases:
        for a in (q, k, v):
            assert X.is_f16_exact(a), name
        gap = X.selection_gap(q, k, X.HEADS, d, pi, valid, causal)
        assert gap >= X.MIN_GAP, f"{name}: gap {gap}"
        assert np.abs(q).max() * d ** 0.5 * X.LOG2E < 2 ** 15, name        # the documented score range of rcdm.h
        assert (np.abs(v) >= 0.25).all() and (np.abs(v) <= 4).all(), name
        Lk = k.shape[1]
        for b in range(pi.shape[0]):
            for h in range(X.HEADS):
                kk = k[b][:, h * d:(h + 1) * d]
                if planted is None:
                    assert len(np.unique(kk, axis=0)) == Lk, f"{name}: K rows not pairwise distinct"
                    assert set(X.must_hit(Lk)) <= set(pi[b, h].tolist()), f"{name}: a boundary key is never selected"
        if planted is None and name.startswith("xattn"):
            assert all(len(set((pi[b, h] // 32).tolist())) == (Lk + 31) // 32 for b in range(pi.shape[0]) for h in range(X.HEADS)), name
        if planted is not None:
            L = Lk
            assert planted.mean() > 0.25, f"{name}: only {planted.mean():.2f} of the queries have a decoy"
            for b in range(pi.shape[0]):
                vis = X.visible(None if valid is None else valid[b], causal, L, L)
                for h in range(X.HEADS):
                    kk = k[b][:, h * d:(h + 1) * d]
                    for i in np.flatnonzero(planted[b, h]):
                        twins = [j for j in range(L) if j != pi[b, h, i] and np.array_equal(kk[j], kk[pi[b, h, i]])]
                        assert twins and not vis[i, twins].any(), f"{name}: query {i} sees its decoy"
                        assert all(not np.array_equal(v[b][j], v[b][pi[b, h, i]]) for j in twins), name
                    hit = set(pi[b, h].tolist())
                    assert 0 in hit, name


def test_selection_assertion_accepts_the_model_and_rejects_the_classic_slips(selection_cases):
    """out == V[pi] bit for bit: true of the consistent model on every selection input; false for a stand-in that reads key
    k + 1 for key k in the P V product, one that swaps two V columns, and (masked inputs) one that ignores the mask."""
    for name, q, k, v, d, pi, valid, causal, planted in selection_cases:
        if q.shape[0] > X.BATCH:            # temporal: a few pixels are enough for the model
            q, k, v, pi = q[:6], k[:6], v[:6], pi[:6]
            if planted is not None:
                planted = planted[:6]
        want = X.selection_expected(v, X.HEADS, d, pi)
        got, _ = X.model_rows(q, k, v, X.HEADS, d, True, valid, causal)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), name
        if k.shape[1] > 1:
            slip, _ = X.model_rows(q, k, np.roll(v, -1, axis=1), X.HEADS, d, True, valid, causal)
            assert not np.array_equal(slip.view(np.uint16), want.view(np.uint16)), f"{name}: key-index slip not caught"
        vp = v.copy()
        vp[..., [0, 1]] = vp[..., [1, 0]]
        perm, _ = X.model_rows(q, k, vp, X.HEADS, d, True, valid, causal)
        assert not np.array_equal(perm.view(np.uint16), want.view(np.uint16)), f"{name}: column swap not caught"
        if planted is not None:
            nomask, _ = X.model_rows(q, k, v, X.HEADS, d, True, None, False)
            L = q.shape[1]
            wrong = (nomask.view(np.uint16) != want.view(np.uint16)).reshape(-1, L, X.HEADS, d).any(axis=3)   # [batch][L][heads]
            assert wrong.transpose(0, 2, 1)[planted].all(), f"{name}: a query with a decoy does not notice the dropped mask"


def test_unity_assertion_rejects_a_column_mixup():
    d = 40
    v = X.unity_v(8, X.HEADS, d).astype(np.float16)
    assert X.unity_mismatches(v, X.HEADS, d) == 0
    rolled = np.roll(v, 5, axis=1)          # c_j has period 10 in j (sign x five exponents): any shift short of it shows
    assert X.unity_mismatches(rolled, X.HEADS, d) == rolled.size
    nan = v.copy()
    nan[3, 7] = np.nan
    assert X.unity_mismatches(nan, X.HEADS, d) == 1
    neg0 = np.zeros_like(v)
    assert X.unity_mismatches(neg0, X.HEADS, d) == neg0.size


def test_rtz_f16_rounds_toward_zero_and_keeps_subnormals():
    p = np.float32([1.0, 0.9999999, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -24, 2.0 ** -24 * 0.99, 3 * 2.0 ** -25, 0.0])
    r = X.rtz_f16(p).astype(np.float32)
    assert (r <= p).all()
    assert r.tolist() == [1.0, 1.0 - 2.0 ** -11, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24, 0.0, 2.0 ** -24, 0.0]


def test_model_gives_zero_rows_where_nothing_is_visible():
    g = np.random.default_rng(5)
    q = X.f16(g.standard_normal((1, 6, 16))).astype(np.float32)
    k = X.f16(g.standard_normal((1, 6, 16))).astype(np.float32)
    v = X.sel_values(g, (1, 6, 16))
    valid = np.ones((1, 6), dtype=np.uint8)
    valid[0, :3] = 0
    out, _ = X.model_rows(q, k, v, 2, 8, True, valid, True)
    assert (out[:3].view(np.uint16) == 0).all()
    assert np.array_equal(out[3].view(np.uint16), v[0, 3].astype(np.float16).view(np.uint16))
