"""CPU checks of tests/gn_cond.py: on every case and every shape the GPU test uses, the reference's operation (torch's fp32
F.group_norm / var_mean on the CPU) stays inside all three budgets — the inputs are fair — and a raw one-pass
sum / sum-of-squares in fp32 leaves the rstd budget on r128, r256 and constant while it meets it on control — the inputs
discriminate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gn_cond as G


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(shape, case):
        if (shape, case) not in cache:
            cache[(shape, case)] = G.make_input(*shape, G.GROUPS, case)
        return cache[(shape, case)]
    return get


def test_cases_cover_both_signs_and_the_band():
    x = G.make_input(2, 64, 320, 32, "r256")
    m, v, _ = G.reference(x, 2, 64, 320, 32, 1e-5)
    assert (m > 0).any() and (m < 0).any()
    assert np.abs(m).min() >= 3.9 and np.abs(m).max() <= 1010
    assert (G.group_kinds(2, 32, "mixed")[0, :3] == np.array(["control", "r256", "constant"], dtype=object)).all()
    xc = G.make_input(1, 16, 64, 32, "constant").reshape(16, 32, 2)
    assert (xc == xc[:1]).all() and len(np.unique(xc[0])) > 3


@pytest.mark.parametrize("case", G.CASES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_operation_is_inside_every_budget(inputs, shape, case):
    samples, rows, C = shape
    x = inputs(shape, case)
    kinds = G.group_kinds(samples, G.GROUPS, case)
    xt = torch.from_numpy(x).reshape(samples, rows, G.GROUPS, C // G.GROUPS)
    gamma, beta = G.affine(C)
    x4 = torch.from_numpy(x).reshape(samples, rows, C).permute(0, 2, 1)[..., None].contiguous()     # (N, C, rows, 1)
    for eps in G.EPS:
        var, mean = torch.var_mean(xt, dim=(1, 3), unbiased=False)
        rstd = (var + eps).rsqrt()
        G.assert_stats(mean.numpy(), rstd.numpy(), x, samples, rows, C, G.GROUPS, eps, kinds, f"torch fp32 {shape} {case} eps {eps}")
        for silu in (False, True):
            y = F.group_norm(x4, G.GROUPS, torch.from_numpy(gamma), torch.from_numpy(beta), eps)
            if silu:
                y = F.silu(y)
            y = y[..., 0].permute(0, 2, 1).reshape(samples * rows, C).half().float().numpy()
            y64 = G.reference(x, samples, rows, C, G.GROUPS, eps, gamma, beta, silu)[3]
            G.assert_output(y, y64, gamma, C, G.GROUPS, kinds, samples, rows, silu, f"torch fp32 {shape} {case} eps {eps} silu {silu}")


@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_one_pass_sums_leave_the_rstd_budget(inputs, shape):
    samples, rows, C = shape
    for case, breaks in (("control", False), ("r128", True), ("r256", True), ("constant", True)):
        x = inputs(shape, case)
        kinds = G.group_kinds(samples, G.GROUPS, case)
        for eps in G.EPS:
            mean, rstd = G.emulate_onepass(x, samples, rows, C, G.GROUPS, eps)
            e = G.stat_errors(mean, rstd, x, samples, rows, C, G.GROUPS, eps, kinds)
            print(f"one-pass fp32 {shape} {case} eps {eps}: rstd rel err {e['rstd']:.3e}, mean err / std {e['mean']:.3e}")
            assert (e["rstd"] > G.RSTD_REL) == breaks, (case, eps, e)
