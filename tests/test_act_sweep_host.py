"""CPU: the references and budgets of tests/act_sweep.py hold up on their own, before any kernel is asked.

1. The fp32 models of the four forms (numpy float32, step by step in the order of the source) are inside their budgets on
   the WHOLE grid, before and after one rounding to f16 — no value is skipped or masked in any comparison.
2. Every mutant of MUTATIONS exceeds its budget somewhere; for each, the share of a close()-style test on random normal
   operands it would pass is printed (the argument tests/test_rowchain_exact_host.py makes with close_accepts).
3. The facts the comment above gelu2 (csrc/common.h) and DESIGN.md state: how far the three-term form is from the true GELU
   in f16 ulps and where, against the five-term form of the fused feed-forward.
4. The conditions of the fused feed-forward's operands (ff_case) hold on every launch of GRID_FF."""
import numpy as np
import pytest

from tests import act_sweep as A

X16 = A.GRID16
X32 = X16.astype(np.float32)
X64 = X16.astype(np.float64)


def _ratios(name, kind, got32, ref, x64):
    got = got32.astype(np.float64)
    raw = A.worst(np.abs(got - ref), A.budget(kind, x64, ref), x64)
    rnd = A.worst(np.abs(A.f16r(got) - ref), A.budget(kind, x64, ref, 1), x64)
    print(f"{name}: unrounded {raw[0]:.4f} of the budget at x = {raw[1]:.6g}; after one f16 rounding {rnd[0]:.4f} at x = {rnd[1]:.6g}")
    return raw[0], rnd[0]


def test_grids():
    assert X16.size == 61442 and np.unique(X16.view(np.uint16)).size == 61442
    assert (np.abs(X64[X64 != 0]) >= 2.0 ** -14).all() and np.abs(X64).max() == 65504.0
    assert (X16.view(np.uint16) == 0x8000).sum() == 1 and (X16.view(np.uint16) == 0).sum() == 1
    ff = A.GRID_FF.astype(np.float64)
    dense = X64[(X64 < 0) & (np.abs(X64) >= 0.5) & (np.abs(X64) < 6.5)]
    assert dense.size == 3 * 1024 + 640 and np.isin(dense, ff).all()
    assert np.isin(X64[::16][np.abs(X64[::16]) <= 16], ff).all() and np.abs(ff).max() <= 16
    assert np.unique(A.GRID_FF.view(np.uint16)).size == A.GRID_FF.size
    print(f"GRID16 {X16.size} values, GRID_FF {ff.size} values = {-(-ff.size // A.FF_C)} launches of {A.FF_C}")


def test_references_against_each_other():
    """The float64 references agree with their textbook forms where those are well conditioned, and the stable forms take
    over where they are not."""
    import math
    mid = X64[np.abs(X64) <= 4]          # 2^-50: two float64 ulps of the largest value
    plain = np.array([0.5 * t * (1.0 + math.erf(t / math.sqrt(2.0))) for t in mid])
    assert np.abs(A.gelu64(mid) - plain).max() <= 2 ** -50
    assert A.gelu64(np.array([-10.0]))[0] == pytest.approx(-10.0 * 7.619853024160527e-24, rel=1e-12)     # Phi(-10)
    with np.errstate(over="ignore"):
        assert np.abs(A.silu64(mid) - mid / (1.0 + np.exp(-mid))).max() <= 2 ** -50
        assert np.abs(A.quick64(mid) - mid / (1.0 + np.exp(-1.702 * mid))).max() <= 2 ** -50
        assert np.abs(A.mish64(mid) - mid * np.tanh(np.log1p(np.exp(mid)))).max() <= 2 ** -50
    for f in (A.gelu64, A.quick64, A.silu64, A.mish64):
        y = f(X64)
        assert np.isfinite(y).all() and (y[X64 > 40] == X64[X64 > 40]).all() and (np.abs(y[X64 < -40]) < 1e-15).all()
    e = A.temb64(np.array([0.0, 2.0]), 6)
    assert (e[0] == [1, 1, 1, 0, 0, 0]).all() and e[1, 0] == math.cos(2.0) and e[1, 3] == math.sin(2.0)
    assert e[1, 1] == math.cos(2.0 * math.exp(-A.LN1E4 / 3))


def test_models_inside_their_budgets():
    g3 = _ratios("three-term GELU (gelu2)", "gelu3", A.gelu_f32(X32, A.GELU3), A.gelu64(X64), X64)
    g5 = _ratios("five-term GELU (geglu_slice)", "gelu5", A.gelu_f32(X32, A.GELU5), A.gelu64(X64), X64)
    qk = _ratios("quick-GELU (quick_gelu2)", "quick", A.quick_f32(X32), A.quick64(X64), X64)
    si = _ratios("SiLU (silu_f), f16 arguments", "silu", A.silu_f32(X32), A.silu64(X64), X64)
    assert 0.80 <= g3[0] <= 0.88 and g3[1] < 1.0          # measured 0.8400 at x = -2.293 / 0.9934
    assert g5[0] <= 0.40 and g5[1] < 1.0                  # 0.3049 / 0.9974
    # quick-GELU has no fp32-output site: its evaluation term is only ever used next to a rounding term.  Unrounded the
    # model measures 1.07 at x = -26.4, where the value is 1e-18 (the exponent constant's own rounding, which the term
    # counts with the product's as one u); with the rounding term 0.9997.
    assert qk[1] < 1.0 and qk[0] < 1.1
    assert si[0] < 1.0 and si[1] < 1.0
    xs = A.off_grid(X16)
    xs64 = xs.astype(np.float64)
    got, ref = A.silu_f32(xs).astype(np.float64), A.silu64(xs64)
    full = A.worst(np.abs(got - ref), A.budget("silu", xs64, ref), xs64)
    tight = A.worst(np.abs(got - ref), (4.0 + 2.0 * np.abs(xs64)) * A.U * np.abs(ref) + 1e-30, xs64)
    print(f"SiLU on the {xs.size} fp32 arguments: {full[0]:.4f} of the budget at x = {full[1]:.6g}; {tight[0]:.4f} of a (4 + 2 |x|) u |y| bound")
    assert full[0] < 1.0 and 0.6 <= tight[0] < 1.0        # 0.5550 / 0.6966
    assert xs64.min() < -87.3 and xs64.max() > 88 and (A.f16r(xs64[xs.size // 2:]) != xs64[xs.size // 2:])[X64 != 0].all()


def _randn_share(name, hidden):
    """The mutant on what the tolerance suites feed the function: f16-rounded normal operands (gates N(0, 1), the GEGLU's
    hidden value N(0, 1) too), 64 tests of 4096 values; the share of tests close() passes as a whole, and of elements."""
    g = np.random.default_rng(5)
    tests = elems = 0
    for _ in range(64):
        x = A.f16r(g.standard_normal(4096)).astype(np.float32)
        if name == "geglu_swap":
            h = A.f16r(g.standard_normal(4096))
            got = x.astype(np.float64) * A.gelu_f32(h.astype(np.float32)).astype(np.float64)
            ref = h * A.gelu64(x.astype(np.float64))
        else:
            got, ref, _ = A.mutant(name, x, hidden)
        ok = A.close_accepts(A.f16r(got), ref)
        tests += bool(ok.all())
        elems += ok.mean()
    return tests / 64, elems / 64


@pytest.mark.parametrize("name", [m for m in A.MUTATIONS if not m.startswith("temb")])
def test_mutant_is_rejected(name):
    hidden = -1.5       # the GPU test's second GEGLU pass
    got, ref, bud = A.mutant(name, X32, hidden)
    r, at = A.worst(np.abs(got - ref), bud, X64)
    rr, at_r = A.worst(np.abs(A.f16r(got) - ref), bud + A.rounding(ref, 1), X64)
    tests, elems = _randn_share(name, hidden)
    print(f"{name} ({A.MUTATIONS[name]}): {r:.4g} of the budget at x = {at:.6g} unrounded, {rr:.4g} at x = {at_r:.6g} after one f16 "
          f"rounding; close() on N(0, 1) operands passes {100 * tests:.0f} % of the tests, {100 * elems:.2f} % of the elements")
    if name == "gelu5_under_gelu3_budget":
        # the five-term mutant the five-term budget rejects (gelu5_coef) is invisible to the three-term budget
        assert r < 1.0 and rr < 1.0
        own = A.mutant("gelu5_coef", X32)
        assert A.worst(np.abs(own[0] - own[1]), own[2], X64)[0] > 1.0
        return
    assert r > 1.0 and rr > 1.0, f"{name} stays inside the budget"
    if name == "gelu3_coef":
        # at x -> 0 the polynomial has to sum to 1/2: 1e-4 more is 1e-4 |x| = 8 times the documented 1.25e-5 |x|
        contract = A.worst(np.abs(got - ref), A.FORM["gelu3"] * np.abs(X64) + A.FTZ, X64)
        print(f"  against the documented contract 1.25e-5 |x| alone: {contract[0]:.3f} at x = {contract[1]:.6g}")
        assert contract[0] > 7.5


@pytest.mark.parametrize("name", ["temb_swap", "temb_half_minus_one"])
@pytest.mark.parametrize("dim", [d for d in A.TEMB_DIMS if d > 2])
def test_embedding_mutant_is_rejected(name, dim):
    """(dim 2 has a single frequency, w = 1: i / (half - 1) has nothing to act on, and the swap is tested from dim 6 up too.)"""
    t = A.temb_rows(7)
    ref, bud = A.temb64(t, dim), A.budget_temb(t, dim)
    got = A.temb64(t, dim, swap=name == "temb_swap", half_minus_one=name == "temb_half_minus_one")
    r, _ = A.worst(np.abs(got - ref), bud, 0.0)
    ok = A.close_accepts(got, ref)
    print(f"{name} at dim {dim}: {r:.4g} of the budget; close() accepts {100 * ok.mean():.1f} % of the elements")
    assert r > 1.0
    fp32 = A.temb64(t, dim).astype(np.float32).astype(np.float64)         # the reference rounded to fp32 is inside
    assert A.worst(np.abs(fp32 - ref), bud, 0.0)[0] < 1.0


def test_three_term_form_against_the_true_gelu():
    """What csrc/common.h and DESIGN.md say with numbers.  The three-term form's error is bounded relative to |x|, not to the
    value: on gates in [-6, -2] it is up to 20.8 f16 ulps of the true GELU away (x = -4.012: true -1.209e-4, the form
    -1.222e-4; 21 ulps once both are rounded to f16), inside 1.25e-5 |x| everywhere (0.84 at x = -2.293).  The five-term
    form of the fused feed-forward stays within 0.97 ulp."""
    ref = A.gelu64(X64)
    g3 = A.gelu_f32(X32, A.GELU3).astype(np.float64)
    g5 = A.gelu_f32(X32, A.GELU5).astype(np.float64)
    d3, d5 = np.abs(g3 - ref) / A.ulp16(ref), np.abs(g5 - ref) / A.ulp16(ref)
    i = int(np.argmax(d3))
    print(f"three-term: {d3[i]:.2f} f16 ulps at x = {X64[i]:.6g} (true {ref[i]:.4e}, form {g3[i]:.4e}); five-term: {d5.max():.3f} at x = {X64[np.argmax(d5)]:.6g}")
    assert 20.5 <= d3[i] <= 21.1 and X64[i] == pytest.approx(-4.012, abs=2e-3)
    assert ref[i] == pytest.approx(-1.209e-4, rel=1e-3) and g3[i] == pytest.approx(-1.222e-4, rel=1e-3)
    assert d5.max() <= 0.97
    assert (d3[(X64 > -2) | (X64 < -6)] < 8).all() and d3[(X64 <= -2) & (X64 >= -6)].max() == d3[i]
    stored = np.abs(A.f16r(g3) - A.f16r(ref)) / A.ulp16(ref)
    assert stored.max() == 21.0
    ratio = A.worst(np.abs(g3 - ref), A.budget("gelu3", X64, ref), X64)
    alone = A.worst(np.abs(g3 - ref), A.FORM["gelu3"] * np.abs(X64) + A.FTZ, X64)
    print(f"of form + evaluation: {ratio[0]:.4f} at x = {ratio[1]:.6g}; of 1.25e-5 |x| alone: {alone[0]:.4f} at x = {alone[1]:.6g}")
    assert 0.80 <= ratio[0] <= 0.88 and ratio[1] == pytest.approx(-2.293, abs=2e-3) and alone[0] < 0.9
    # the two feed-forwards of one layer: the difference of the forms in ulps of the value, and in units of |h| = 1
    both = np.abs(A.f16r(g3) - A.f16r(g5)) / A.ulp16(ref)
    j = int(np.argmax(both))
    print(f"fused against unfused: up to {both[j]:.0f} f16 ulps at gate {X64[j]:.6g}; |gelu3 - gelu5| <= {np.abs(g3 - g5).max():.3g}")
    assert 20 <= both[j] <= 22 and -6 <= X64[j] <= -2 and np.abs(g3 - g5).max() < 2.7e-5


def test_ff_cases_hold_on_every_launch():
    """ff_case asserts its own conditions (y = +-1, gate = the swept value, |h| in [1, 2), 2^13 h in [8192, 16384) where the
    residual is rounded away); every value of GRID_FF is in exactly one launch."""
    seen, w5, w3 = [], 0.0, 0.0
    for i in range(0, A.GRID_FF.size, A.FF_C):
        c = A.ff_case(A.GRID_FF[i:i + A.FF_C])
        seen.append(c["vals"][:c["n"]])
        assert (c["p"] == 2.0 ** np.round(np.log2(c["p"]))).all()
        # the five-term model passes the launch's five-term budget; the three-term form in its place would not
        bud = A.budget("gelu5", c["vals"], c["h_ref"], n_round=1, scale=c["p"])
        for form in (A.GELU5, A.GELU3):
            h = A.f16r((c["p"].astype(np.float32) * A.gelu_f32(c["vals"].astype(np.float32), form)).astype(np.float32))
            r = A.worst(np.abs(h - c["h_ref"]), bud, c["vals"])[0]
            w5, w3 = (max(w5, r), w3) if form is A.GELU5 else (w5, max(w3, r))
    print(f"fused feed-forward operands: the five-term model uses {w5:.4f} of the five-term budget, the three-term form {w3:.2f}")
    assert w5 < 1.0 and w3 > 5.0                               # 0.9946 / 6.26
    seen = np.concatenate(seen)
    assert seen.size == A.GRID_FF.size and (seen == A.GRID_FF.astype(np.float64)).all()
