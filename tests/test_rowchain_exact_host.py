"""CPU: the exact-answer cases of tests/rowchain_exact.py without a GPU.

1. Every case tests/test_hip_rowchain_exact.py launches: the conditions that make its answer exact hold on the reference
   (check_case), the hidden-dense phases switch every hidden unit on in exactly one launch, and an fp32 two-pass LayerNorm
   (1.0f / 320 multiplied as the kernel does, eps 0 / 1e-6 / 1e-5, rstd off by +-2^-16) rounds to the integer rows.
2. The model is mutated in one place at a time — the defects a row chain can have that move one term — and every mutation
   breaks exact equality.  Next to each, the same mutation is applied to the chain on the tolerance suites' usual operands
   (randn rows, randn * K^-0.5 weights, C = 320) and the share of the touched elements that close() of
   tests/test_hip_kernels.py still accepts is printed: what the tolerance lets through.
   One mutation the exact cases CANNOT see, and the test says so instead of pretending: the LayerNorm variance as
   E[x^2] - mean^2 in fp32.  On a two-valued f16 row E[x^2] = m^2 + v^2 and mean^2 = m^2 need at most 2 * 11 + 1 bits, so
   both are exact in fp32 and the form gives the two-pass result bit for bit at any mean / spread f16 can hold.  It differs
   only on rows that are not two-valued: that stays with the tolerance tests (rows with |mean| = 4 sigma there)."""
import numpy as np
import pytest

from tests import rowchain_exact as R


# ---- 1. every GPU case's conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s["name"] for s in R.ALL_CASES])
def test_case_conditions(name):
    c = R.case(name)
    info = R.check_case(c)
    print(name, {k: round(v, 3) for k, v in info.items()})
    assert c["M"] in (16, 160, 176, 333, 480) or (c["tail"] == 4 and (c["b"], c["hw"]) in ((1, 32), (1, 48), (2, 48)))
    if c["tail"] == 4:
        assert c["pe"] is None


def test_determinism_cases_have_three_blocks():
    assert all(R.BY_NAME[n]["M"] == 480 for n in R.CASES_F)


@pytest.mark.parametrize("P,names", [(4, [f"D-ff-hid4-{p}" for p in range(4)]), (16, [f"D-t0-hid16-{p}" for p in range(16)]),
                                     (4, [f"D-t2-hid4-{p}" for p in range(4)])])
def test_every_hidden_unit_is_on_in_exactly_one_phase(P, names):
    on = np.stack([R.case(n)["b1"][4 * R.C:] == 16 for n in names])
    assert (on.sum(axis=0) == 1).all()
    # within every 32-unit group the on position moves across both 16-column halves (the A and the B chunk of the group)
    pos = np.stack([np.flatnonzero(o.reshape(-1, 32)[g]) for o in on for g in (0, 7)])
    assert (pos < 16).any() and (pos >= 16).any()
    for n in names:
        c = R.case(n)
        assert R.BY_NAME[n]["ff"][1] == P and (c["w1"][4 * R.C:] == 0).all() and (np.abs(c["w1"][:4 * R.C]) == 1).all()


@pytest.mark.parametrize("name", ["C-t3-f8-r20", "A-t3-res", "D-ff-hid4-0", "E-select-2-48"])
def test_fp32_layernorm_rounds_to_the_integer(name):
    """What an fp32 kernel computes — the sum times 1.0f / 320, two passes, rsqrt off by a relative 2^-16 either way — rounds
    to the integer at mean / spread 0, 16 and 64, for eps 0, 1e-6 and the production 1e-5.  (rsqrtf(1) == 1 is not used: the
    rows have v = 1, 2 and 4, and eps moves every rstd off a power of two.)"""
    c = R.case(name)
    rows = np.arange(c["M"])
    bpe = np.broadcast_to(c["ln_b"], (c["M"], R.C)) + (c["pe"][(rows // c["rpf"]) % c["frames"]] if c["pe"] is not None else 0.0)
    for eps in (0.0, 1e-6, 1e-5):
        for factor in (1.0, 1.0 + 2.0 ** -16, 1.0 - 2.0 ** -16):
            y = R._ln_fp32(c["T"], c["ln_g"], bpe, eps, False, factor)
            assert (R.f16r(y) == c["y_int"]).all(), (eps, factor)


# ---- 2. mutations ---------------------------------------------------------------------------------------------------------
def _share(name, c, key="out"):
    """The mutation on the tolerance suites' operands: print the share of the touched elements close() accepts."""
    got, ref = R.model(c, name)[key], R.model(c)[key]
    touched = got != ref
    assert touched.any(), f"{name} touches nothing on the random operands"
    ok = R.close_accepts(got, ref) & touched
    share = ok.sum() / touched.sum()
    print(f"{name} ({R.MUTATIONS[name]}): touches {int(touched.sum())} of {touched.size} elements of {key} on the randn chain; "
          f"close() accepts {100 * share:.1f} % of them")
    return share


def _rejected(mutation, case_name, key="out"):
    c = R.case(case_name)
    got = R.model(c, mutation)[key]
    n = int((got != c["ref"][key]).sum())
    assert n > 0, f"{mutation} leaves {key} of {case_name} unchanged"
    print(f"{mutation} on {case_name}: {n} of {got.size} elements of {key} differ")
    return n


def test_mutation_stage_a_zero_kstep():
    for name in ("A-t3-res", "A-t3-perm", "B-176-t3-dense", "E-unity-2-48"):
        _rejected("stage_a_zero_kstep", name, "tok")
    _rejected("stage_a_zero_kstep", "A-t3-res")
    c = R.randn_case(3)
    _share("stage_a_zero_kstep", c, "tok")
    _share("stage_a_zero_kstep", c)


def test_mutation_tail_stale_fragment():
    for name in ("C-t3-f5-r64", "A-t1-res", "B-160-t1"):
        assert _rejected("tail_stale_fragment", name) >= R.case(name)["M"]       # every row, somewhere in the fragment
    _share("tail_stale_fragment", R.randn_case(3, pe_frames=5))


def test_mutation_b1p_swap_pair():
    for name in ("D-ff-hid4-0", "D-t0-hid16-7", "D-t2-hid4-3", "D-ff-gate-M480", "D-t2-gate"):
        _rejected("b1p_swap_pair", name)
    _share("b1p_swap_pair", R.randn_case(0))


def test_mutation_ff_b_next_group():
    hit = 0
    for ph in range(4):      # units 176..191: on in some phases only — every phase is run, and one of them must see it
        c = R.case(f"D-ff-hid4-{ph}")
        hit += int((R.model(c, "ff_b_next_group")["out"] != c["ref"]["out"]).any())
    assert hit >= 1
    for name in ("D-ff-gate-M480", "D-t0-gate", "D-t2-gate"):
        _rejected("ff_b_next_group", name)
    _share("ff_b_next_group", R.randn_case(0))


def test_mutation_pe_row_off_by_one():
    for name in ("C-t3-f5-r64", "C-t3-f8-r20", "C-t1-f8-r64", "C-t1-f5-r20", "B-176-t3-pe"):
        c = R.case(name)
        last = (np.arange(c["M"]) + 1) % c["rpf"] == 0
        bad = (R.model(c, "pe_row_off_by_one")["out"] != c["ref"]["out"]).any(axis=1)
        assert (bad == last).all(), f"{name}: exactly the last row of every frame has to change"
    _share("pe_row_off_by_one", R.randn_case(3, pe_frames=5))


def test_mutation_gn_sample_plus_one():
    for name in ("B-176-t3", "B-176-t0", "B-176-t3-pe", "B-176-t3-dense"):
        _rejected("gn_sample_plus_one", name, "tok")
    _rejected("gn_sample_plus_one", "B-176-t3")
    c = R.randn_case(3, M=528, res=False, gn_rows=176)
    _share("gn_sample_plus_one", c, "tok")
    _share("gn_sample_plus_one", c)


def test_mutation_proj_skip_residual():
    for name in ("A-t2-res", "D-t2-hid4-0", "D-t2-hid16", "D-t2-gate"):
        assert _rejected("proj_skip_residual", name) == 16 * R.case(name)["M"]   # tok is never 0: every row, all 16 channels
    _share("proj_skip_residual", R.randn_case(2))


def test_mutation_att_v_next_frame():
    for name in ("E-select-1-32", "E-select-1-48", "E-select-2-48"):
        _rejected("att_v_next_frame", name)
    c = R.case("E-unity-2-48")
    assert (R.model(c, "att_v_next_frame")["out"] == c["ref"]["out"]).all()      # unity cannot see it (v is the same in every frame)
    _share("att_v_next_frame", R.randn_case(4, M=5 * 32, res=True, b=1, hw=32))


def test_variance_as_e2_minus_mean2_is_invisible_on_two_valued_rows():
    """See the module docstring: on these rows the fp32 E[x^2] - mean^2 form is exact, so no exact case rejects it — asserted,
    so that nobody reads the suite as covering it.  On rows that are not two-valued it does move the output: the share close()
    accepts on random rows at mean / spread 64 is printed."""
    for name in ("C-t3-f8-r20", "A-t3-res", "D-t0-hid16-4", "E-select-2-48"):
        c = R.case(name)
        m = R.model(c, "ln_var_e2")
        assert (m["y"] == c["ref"]["y"]).all() and (m["out"] == c["ref"]["out"]).all()
        t = c["T"].astype(np.float32)
        assert ((t * t).sum(axis=1, dtype=np.float32) == (c["T"] ** 2).sum(axis=1)).all()      # the fp32 sum of squares is exact
    c = R.randn_case(3, res=False)
    c["ba"] = c["ba"] + 64.0 * 0.7       # rows at mean / spread ~ 64 (stage A's output has a spread of ~ 1)
    got, ref = R.model(c, "ln_var_e2"), R.model(c)
    touched = got["out"] != ref["out"]
    assert touched.any()
    ok = R.close_accepts(got["out"], ref["out"]) & touched
    print(f"ln_var_e2 on randn rows at mean / spread 64: touches {int(touched.sum())} of {touched.size} outputs, max |y - y_ref| "
          f"{np.abs(got['y'] - ref['y']).max():.3g}; close() accepts {100 * ok.sum() / touched.sum():.1f} % of them")
