"""CPU checks of tests/ln_cond.py: every case keeps its promise about the rounded values; a two-pass fp32 LayerNorm and the
library's tile rule (emulate_tiles, both producer tile widths) stay inside every budget on every case and shape — the budgets
are fair to the reference's operation —; the raw one-pass E[x^2] - mean^2 leaves the rstd budget on r64, r128, r256 and mixed
and the constant budget on at least one constant — the inputs discriminate —; and the accumulator of the deferred consumer's
x W'^T is exact in any order on the rows whose budget has no accumulation term."""
import numpy as np
import pytest

from tests import gn_cond as G
from tests import ln_cond as L

IDS = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(shape, case):
        if (shape, case) not in cache:
            cache[(shape, case)] = L.make_input(*shape, case)
        return cache[(shape, case)]
    return get


def test_cases_keep_their_promises(inputs):
    for shape in L.SHAPES:
        for case in L.CASES:
            inputs(shape, case)                     # make_input asserts the band, the signs and the constancy
    x = inputs((300, 64), "constant")
    assert (x == x[:, :1]).all() and (x[:len(G.CONSTANTS), 0] == G.f16(G.CONSTANTS)).all() and len(np.unique(x[:, 0])) > 100
    k = L.row_kinds(9, "mixed")
    assert list(k[:3]) == ["control", "r256", "constant"]
    xm = inputs((97, 200), "mixed")
    assert (xm[2] == G.f16(G.CONSTANTS[0])).all() and (xm[5] == G.f16(G.CONSTANTS[1])).all()
    xs = inputs((1000, 640), "spread").astype(np.float64).reshape(1000, 10, 64)
    bm = xs.mean(axis=2)
    assert (bm.std(axis=1) / xs.std(axis=2).mean(axis=1)).min() > 0.15       # the 64-wide blocks of a row do sit at different means


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_two_pass_and_tile_rule_are_inside_every_budget(inputs, shape, case):
    M, C = shape
    x = inputs(shape, case)
    kinds = L.row_kinds(M, case)
    mean, rstd = L.emulate_twopass(x)
    L.assert_stats(mean, rstd, x, kinds, f"two-pass fp32 {shape} {case}")
    gamma, beta = L.affine(C)
    L.assert_plain_output(L.twopass_output(x, gamma, beta), x, gamma, beta, kinds, f"two-pass fp32 {shape} {case}")
    w = L.consumer_weights(16, C)
    y64 = L.consumer64(x, w)
    tol = L.consumer_budget(y64, w, x, kinds)
    for bn in (64, 128):
        mean, rstd = L.emulate_tiles(x, bn)
        L.assert_stats(mean, rstd, x, kinds, f"tile rule, {bn}-wide tiles {shape} {case}")
        live = kinds != "control"
        fig = []
        for staged in (False, True):
            y = L.deferred_output(x, w, mean, rstd, staged)
            fig.append(float((np.abs(y - y64)[live] / tol[live]).max()) if live.any() else 0.0)
            fig.append(L.control_close(y[~live], y64[~live]))
        print(f"tile rule, {bn}-wide tiles {shape} {case}: deferred output {fig[0]:.3f} of its budget, control rows {fig[1]:.3f} of "
              f"theirs (with the f16 staging of the LDS-DMA tiles: {fig[2]:.3f}, {fig[3]:.3f})")
        assert fig[0] <= 1.0 and fig[1] <= 1.0      # the statistics' share; the staging order is the GPU test's business


@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_raw_one_pass_leaves_the_budgets(inputs, shape):
    M, C = shape
    for bn in (64, 128):
        for case, breaks in (("control", False), ("r64", True), ("r128", True), ("r256", True), ("mixed", True)):
            x = inputs(shape, case)
            mean, rstd = L.emulate_onepass(x, bn)
            e = L.stat_figures(mean, rstd, x, L.row_kinds(M, case))
            print(f"one-pass fp32, {bn}-wide tiles {shape} {case}: rstd at {e['rstd']:.2f} of its budget")
            assert (e["rstd"] > 1.0) == breaks, (case, bn, e)
        x = inputs(shape, "constant")
        mean, rstd = L.emulate_onepass(x, bn)
        e = L.stat_figures(mean, rstd, x, L.row_kinds(M, "constant"))
        print(f"one-pass fp32, {bn}-wide tiles {shape} constant: rstd at {e['const_rstd']:.2f} of its budget")
        assert e["const_rstd"] > 1.0, (bn, e)


@pytest.mark.parametrize("case", ["r64", "r128", "r256", "spread", "constant"])
def test_accumulator_is_exact_in_any_order(inputs, case):
    """x W'^T summed in fp32 forwards, backwards and in interleaved blocks of 16 (an MFMA k-slice) gives the same bits, and
    they are the float64 sum: the deferred consumer's budget needs no accumulation term on these rows."""
    shape = (640, 1280)
    x = inputs(shape, case)[:64]
    w = L.consumer_weights(16, shape[1])
    Wp = w["Wp"].astype(np.float32)
    prod = x[:, None, :] * Wp[None, :, :]                       # exact: 11-bit x 2-bit significands
    assert (prod.astype(np.float64) == x.astype(np.float64)[:, None, :] * w["Wp"][None, :, :]).all()
    C = shape[1]
    orders = [np.arange(C), np.arange(C)[::-1], np.arange(C).reshape(-1, 16).T.reshape(-1)]
    sums = []
    for o in orders:
        acc = np.zeros(prod.shape[:2], dtype=np.float32)
        for c in o:
            acc = acc + prod[:, :, c]
        sums.append(acc)
    exact = x.astype(np.float64) @ w["Wp"].T
    for s in sums:
        assert (s.view(np.int32) == sums[0].view(np.int32)).all() and (s.astype(np.float64) == exact).all()
