"""CPU: the exact-answer cases of tests/gemm_exact.py without a GPU.

1. The numpy model runs end to end at every shape tests/test_hip_gemm_exact.py launches, with the split count the library's
   own planner answers (the plan queries need no device): every condition holds, and rounding the slabs to f16 leaves the
   answer exact.
2. The model is mutated in one place at a time — the defects an implicit GEMM can have that move one term — and every
   mutation breaks exact equality.  Next to each, the same mutation is applied to the 2880-term convolution (320 channels,
   3x3) on the kernel suites' usual operands (randn activations, randn * K^-0.5 weights) and the share of the touched
   elements that close() of tests/test_hip_kernels.py still accepts is printed: what the tolerance lets through."""
import numpy as np
import pytest

from tests import gemm_exact as X


@pytest.fixture(scope="module")
def hip():
    from rcdms_amd import hip
    hip.load()
    yield hip
    hip.set_igemm_variant(-1)


# ---- 1. every GPU case's shape ------------------------------------------------------------------------------------------
def _exact_through_slabs(problem, splits, acc):
    parts = problem.partials(splits)
    biggest = X.check_partials(parts)
    for slab in (None, np.float16):
        assert (X.reduce_slabs(parts, slab) == acc).all()
    return biggest


@pytest.mark.parametrize("M,N,K,epi,split,scale", X.GEMM_CASES)
def test_gemm_cases(hip, M, N, K, epi, split, scale):
    c = X.gemm_case(M, N, K, epi, scale)
    acc = c["problem"].acc()
    assert (acc == c["A"] @ c["W"].T).all()
    d = hip.GemmDesc(M, N, K, K + 8, N + 16, N + 8, epi, c["rps"], N + 8, scale, split)
    seen = set()
    try:
        for variant in range(1, 11):
            hip.set_igemm_variant(variant)
            splits = hip.gemm_plan_query(d)["splits"]
            assert split in (0, 1) or splits > 1
            if splits > 1 and splits not in seen:
                seen.add(splits)
                _exact_through_slabs(c["problem"], splits, acc)
    finally:
        hip.set_igemm_variant(-1)


@pytest.mark.parametrize("n_img,H,W,cin,cout,stride,up,pao,split,cin2", X.CONV_CASES + X.ADD1X1_CASES)
def test_conv_cases(hip, n_img, H, W, cin, cout, stride, up, pao, split, cin2):
    c = X.conv_case(n_img, H, W, cin, cout, stride, up, pao, cin2, 7, 0.5 if cin2 else 1.0)
    p = c["problem"]
    acc = p.acc()
    d = hip.ConvDesc(n_img, H, W, cin, cout, stride, up, cin + 8, cout, cout, 7, c["rps"], cout, 1.0, split, pao, 0, cin2, cin2 + 16 if cin2 else 0)
    seen = set()
    try:
        for variant in range(1, 11):
            hip.set_igemm_variant(variant)
            plan = hip.conv3x3_plan_query(d)
            assert plan["k_steps"] == p.nk
            assert split == 1 or plan["splits"] > 1
            if plan["splits"] > 1 and plan["splits"] not in seen:
                seen.add(plan["splits"])
                _exact_through_slabs(p, plan["splits"], acc)
    finally:
        hip.set_igemm_variant(-1)


def test_dup_rows_gnstat_and_tap_plane_shapes(hip):
    """The remaining launches of the GPU file: dup_rows (300 x 320 x 256), the *_gnstat pair, the nine tap planes."""
    for (M, N, K, epi, split) in ((300, 320, 256, 1, 2), (320, 320, 320, 7, 2)):
        c = X.gemm_case(M, N, K, epi, 1.0)
        _exact_through_slabs(c["problem"], split, c["problem"].acc())
    c = X.conv_case(2, 8, 8, 128, 320, 1, 0, 0, 0, 7, 1.0)
    _exact_through_slabs(c["problem"], 3, c["problem"].acc())
    gnd = hip.GroupNormDesc(2, 64, 320, 32, 328, 320, 1e-5, 0)
    assert hip.conv3x3_gnstat_ok(hip.ConvDesc(2, 8, 8, 128, 320, 1, 0, 136, 328, 320, 7, 64, 320, 1.0, 3, 0, 0, 0, 0), gnd)
    for up in (0, 1):
        c = X.conv_case(3, 4, 6, 64, 64, 1, up, 0, 0, 1, 1.0)
        planes = c["x"].reshape(-1, 64) @ c["w"].transpose(2, 3, 0, 1).reshape(9 * 64, 64).T      # [pixel][tap * c_out + c]
        X.check_output(planes)
        # the gather: output pixel (Y, X) sums the planes' values of the source pixels its taps land on
        n, H, W = 3, 4, 6
        H2, W2 = H << up, W << up
        out = np.zeros((n, H2, W2, 64))
        for ky in range(3):
            for kx in range(3):
                for Y in range(H2):
                    for Xc in range(W2):
                        yy, xx = Y + ky - 1, Xc + kx - 1
                        if 0 <= yy < H2 and 0 <= xx < W2:
                            rows = np.arange(n) * H * W + (yy >> up) * W + (xx >> up)
                            out[:, Y, Xc] += planes[rows, (ky * 3 + kx) * 64:(ky * 3 + kx + 1) * 64]
        assert (out.reshape(-1, 64) + c["bias"] == c["ref"]).all()


@pytest.mark.parametrize("n_img,H,W,cin,cout", sorted({c[:5] for c in X.UP2_CASES}))
def test_up2_cases(hip, n_img, H, W, cin, cout):
    c = X.up2_case(n_img, H, W, cin, cout)       # (asserts that the four phases are the upsampled convolution)
    for p in c["problems"]:
        acc = p.acc()
        for splits in (2, 3):
            if p.nk >= splits and -(-p.nk // -(-p.nk // splits)) == splits:
                _exact_through_slabs(p, splits, acc)
    assert np.abs(X.up2_pack(c["w"])).max() <= 4


@pytest.mark.parametrize("n_img,H,W,cin,cin2,cout,epi,split,scale,gn", X.WINO_CASES)
def test_wino_cases(hip, n_img, H, W, cin, cin2, cout, epi, split, scale, gn):
    c = X.wino_case(n_img, H, W, cin, cin2, cout, epi, scale, gn)
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 0, cin + 8, cout, cout if epi & 4 else 0, epi, H * W, cout, scale, split, 0, 0, cin2,
                     cin2 + 16 if cin2 else 0)
    assert hip.conv3x3_wino_supported(d)
    splits = hip.conv3x3_wino_plan_query(d)[5]
    assert split <= 1 or splits > 1
    biggest = X.wino_check(c, splits)
    print(f"largest transform-domain partial {biggest}")


def test_slab_range_cases():
    """The cancellation and out-of-range operands of the GPU file: what the model says about them."""
    for P in (2048, 40000, 81920):
        c = X.cancel_gemm_case(P)
        parts = c["problem"].partials(2)
        assert (parts[0] == P).all() and (parts.sum(axis=0) == c["r"]).all()
        assert (X.reduce_slabs(parts, None) == c["r"]).all()                  # fp32 slabs: exact
        got = X.reduce_slabs(parts, np.float16)
        if P > 65504:
            assert not np.isfinite(got).any()                                 # f16 slabs out of range: +-inf, their sum NaN
        else:
            err = np.abs(got.astype(np.float16).astype(np.float64) - c["r"])
            bound = X.slab_error_bound(parts, c["r"])
            assert (err <= bound).all()
            print(f"P = {P}: largest error of f16 slabs {err.max()}, bound {bound.max()}")
    for A in X.WINO_CANCEL_LEVELS:
        c = X.cancel_wino_case(A)
        exact, slabs, V, U = X.wino_model(c["x"], c["w"], 2, None, None, np.float16, None)
        assert (exact == c["acc"]).all()                                      # f16 operands and fp32 slabs: exact
        got, _, _, _ = X.wino_model(c["x"], c["w"], 2, None, None, np.float16, np.float16)
        bound = X.wino_slab_error_bound(slabs, c["acc"])
        err = np.abs(got.astype(np.float16).astype(np.float64) - c["acc"])
        assert np.isfinite(got).all() and (err <= bound).all()
        print(f"Winograd, pixel level {A}: largest slab value {np.abs(slabs).max()}, largest error of f16 slabs {err.max()}, bound {bound.max()}")
    c = X.overflow_wino_case()
    got, slabs, V, U = X.wino_model(c["x"], c["w"], 1, None, None, np.float16, None)
    assert np.isinf(V).any(), "B^T d B of the checkerboard stays inside f16"
    big = c["big_rows"]
    assert not np.isfinite(got[big]).any() and (got[~big] == c["acc"][~big]).all()
    assert np.abs(c["acc"]).max() == 0                                        # the nine-tap sums cancel exactly


# ---- 2. mutations -------------------------------------------------------------------------------------------------------
def _randn_conv(cin=320, cout=64, n_img=2, H=8, W=8, cin2=0):
    """The kernel suites' usual operands at the 2880-term convolution (f16-rounded randn, weights * K^-0.5)."""
    g = np.random.default_rng(99)
    h16 = lambda a: a.astype(np.float16).astype(np.float64)
    x = h16(g.standard_normal((n_img, H, W, cin)))
    w = h16(g.standard_normal((cout, cin, 3, 3)) * (9 * cin) ** -0.5)
    x2 = h16(g.standard_normal((n_img, H, W, cin2))) if cin2 else None
    w2 = h16(g.standard_normal((cout, cin2)) * cin2 ** -0.5) if cin2 else None
    return x, w, x2, w2


def _share(name, got, ref):
    """Print the share of the elements the mutation touched that close() accepts; return it."""
    touched = got != ref
    assert touched.any()
    ok = X.close_accepts(got, ref) & touched
    share = ok.sum() / touched.sum()
    print(f"{name}: touches {int(touched.sum())} of {touched.size} elements of the randn convolution; close() accepts {100 * share:.1f} % of them")
    return share


def test_mutation_dropped_k_step():
    """The last k-step of a middle split-K slice is dropped."""
    c = X.conv_case(2, 8, 8, 320, 320, 1, 0, 0, 0, 7, 1.0)
    p = c["problem"]
    assert not (p.partials(4, "drop_last_step_of_middle_split").sum(axis=0) == p.acc()).all()
    c = X.gemm_case(161, 168, 704, 1, 1.0)
    assert not (c["problem"].partials(3, "drop_last_step_of_middle_split").sum(axis=0) == c["problem"].acc()).all()
    x, w, _, _ = _randn_conv()
    q = X.conv_problem(x, w)
    _share("dropped k-step", q.partials(4, "drop_last_step_of_middle_split").sum(axis=0), q.acc())


def test_mutation_dropped_k_tail():
    """The 8-channel K tail is dropped (GEMM: K = 200; conv: c_in = 72)."""
    c = X.gemm_case(130, 72, 200, 1 | 4, 1.0)
    assert not (X.gemm_problem(c["A"], c["W"], "drop_k_tail").acc() == c["problem"].acc()).all()
    c = X.conv_case(6, 10, 6, 72, 72, 1, 0, 0, 0, 7, 1.0)
    assert not (X.conv_problem(c["x"], c["w"], mutate="drop_c_tail").acc() == c["problem"].acc()).all()
    x, w, _, _ = _randn_conv(cin=328)      # 2880 terms + a tail of 8 channels (72 terms)
    _share("dropped 8-channel tail", X.conv_problem(x, w, mutate="drop_c_tail").acc(), X.conv_problem(x, w).acc())


def test_mutation_doubled_border_tap():
    c = X.conv_case(6, 10, 6, 72, 72, 1, 0, 0, 0, 7, 1.0)
    assert not (X.conv_problem(c["x"], c["w"], mutate="double_border_tap").acc() == c["problem"].acc()).all()
    x, w, _, _ = _randn_conv()
    _share("doubled border tap", X.conv_problem(x, w, mutate="double_border_tap").acc(), X.conv_problem(x, w).acc())


def test_mutation_swapped_wino_positions():
    c = X.wino_case(2, 8, 8, 128, 0, 192, 1 | 4, 1.0, False)
    got = X.wino_model(c["x"], c["w"], 2, mutate="swap_positions")[0]
    assert not (got == c["acc"]).all()
    x, w, _, _ = _randn_conv()
    ref = X.wino_model(x, w, 1, operand_dtype=None)[0]
    assert np.abs(ref - X.conv_problem(x, w).acc()).max() < 1e-5      # (the model's slabs are fp32)
    _share("swapped Winograd positions", X.wino_model(x, w, 1, operand_dtype=None, mutate="swap_positions")[0], ref)


def test_mutation_wrong_parity_pixel():
    c = X.wino_case(2, 8, 8, 128, 64, 320, 0, 1.0, False)
    got = X.wino_model(c["x"], c["w"], 2, c["x2"], c["w2"], mutate="wrong_parity_pixel")[0]
    assert not (got == c["acc"]).all()
    x, w, x2, w2 = _randn_conv(cin2=320)
    ref = X.wino_model(x, w, 1, x2, w2, operand_dtype=None)[0]
    _share("second input's parity entry from the wrong pixel", X.wino_model(x, w, 1, x2, w2, operand_dtype=None, mutate="wrong_parity_pixel")[0], ref)


def test_mutation_second_input_order():
    c = X.conv_case(2, 8, 8, 320, 320, 1, 0, 0, 640, 7, 0.5)
    got = X.conv_problem(c["x"], c["w"], x2=c["x2"], w2=c["w2"], mutate="swap_second_input_with_last_tap").acc()
    assert not (got == c["problem"].acc()).all()
    x, w, x2, w2 = _randn_conv(cin2=320)
    _share("second input's k-step swapped with the last tap", X.conv_problem(x, w, x2=x2, w2=w2, mutate="swap_second_input_with_last_tap").acc(),
           X.conv_problem(x, w, x2=x2, w2=w2).acc())
