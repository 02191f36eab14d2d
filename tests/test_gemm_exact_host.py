"""CPU: the exact-answer cases of tests/gemm_exact.py without a GPU.

1. The numpy model runs end to end at every shape tests/test_hip_gemm_exact.py launches, with the split count the library's
   own planner answers (the plan queries need no device): every condition holds, and rounding the slabs to f16 leaves the
   answer exact.
2. The model is mutated in one place at a time — the defects an implicit GEMM can have that move one term — and every
   mutation breaks exact equality.  Next to each, the same mutation is applied to the 2880-term convolution (320 channels,
   3x3) on the kernel suites' usual operands (randn activations, randn * K^-0.5 weights) and the share of the touched
   elements that close() of tests/test_hip_kernels.py still accepts is printed: what the tolerance lets through.
3. The operand addressing the three tile kernels share (rcdms_amd/csrc/igemm_loader.h) runs on the CPU
   (tools/igemm_loader_host.cpp): the operands gathered through its offsets are the model's A and W, the tile order is a
   bijection, and one moved border tap breaks the comparison.
4. The same for the batched GEMM of the Winograd conv (rcdms_amd/csrc/wino_loader.h, the tool's `wino` mode): every
   (entry, split, tile) is dealt to exactly one block on both paths of the dealing, and the gathered operands are the
   model's V / U panels and the second input's parity pixels."""
import os
import subprocess

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


# ---- 3. the kernels' operand addressing (csrc/igemm_loader.h), run on the CPU by tools/igemm_loader_host.cpp -----------------
# For every case the GPU file launches, at every tile shape the planner gives it: gathering the raw input and the packed
# weight through the offsets the kernels would hand to the DMA (out of bounds read as 0) gives the A and W matrices of the
# case's Problem, columns in k order per k-step of 64.  Integer arrays, compared with ==.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SEG2 = 0x7fffffff
POISON = 777.0           # the padding behind a row's channels (lda > c_in): no operand has this value
LOADER_FIELDS = ("M", "N", "Cin", "Ktot", "Hi", "Wi", "Ho", "Wo", "stride", "up", "pad", "lda", "nk", "nk1", "Cin2", "lda2", "ph_rows",
                 "tilesM", "tilesN")


@pytest.fixture(scope="module")
def loader_tool(tmp_path_factory):
    """tools/igemm_loader_host.cpp built with the project's compiler (host side only), no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("igemm_loader") / "igemm_loader_host")
    cmd = [build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-I", build.CSRC,
           os.path.join(ROOT, "tools", "igemm_loader_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def loader_args(taps, bm, bn, geom):
    f = dict(Hi=1, Wi=1, Ho=1, Wo=1, stride=1, up=0, pad=1, nk1=NO_SEG2, Cin2=0, lda2=0, ph_rows=0)
    f.update(geom)
    return [str(v) for v in [taps, bm, bn] + [f[k] for k in LOADER_FIELDS]]


def run_loader(tool, taps, bm, bn, geom):
    """The tool's records [n][7]: (kind, tile, k-step, tile row, lane chunk, first channel within the k-step, byte offset | -1)."""
    r = subprocess.run([tool] + loader_args(taps, bm, bn, geom), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.fromstring(r.stdout.decode(), dtype=np.int64, sep=" ").reshape(-1, 7)


def padded_rows(a, ld):
    """[rows][c] -> the flat buffer of rows of stride ld, POISON behind the channels."""
    out = np.full((a.shape[0], ld), POISON)
    out[:, :a.shape[1]] = a
    return out.reshape(-1)


def in_k_steps(mat, steps, rows):
    """A Problem's matrix as the kernels see it: [rows][nk * 64], k-step ks at columns ks * 64, zeros where a row, or a
    channel of a short k-step, does not exist."""
    out = np.zeros((rows, len(steps) * X.BK))
    for ks, (lo, hi) in enumerate(steps):
        out[:mat.shape[0], ks * X.BK:ks * X.BK + hi - lo] = mat[:, lo:hi]
    return out


def _gather(rec, raws, want, rows_of, tile_rows, nk):
    """rec: the records of one operand.  True if the values behind the offsets equal want[row][k-step columns]."""
    kind, lin, ks, row, lch, c, off = rec.T
    assert ((c % 8 == 0) & (c >= 0) & (c < X.BK) & (lch >= 0) & (lch < 8) & (row >= 0) & (row < tile_rows)).all()
    n_tiles = int(lin.max()) + 1
    assert len(rec) == n_tiles * nk * tile_rows * 8, "a piece is missing or printed twice"
    for chunk in (c // 8, lch):        # every (tile, k-step, row) has each source chunk and each LDS slot once: the swizzle is a bijection
        assert np.unique(((lin * nk + ks) * tile_rows + row) * 8 + chunk).size == len(rec)
    vals = np.zeros((len(rec), 8))
    for k, raw in raws.items():
        sel = (kind == k) & (off >= 0)
        assert (off[sel] % 16 == 0).all(), "a DMA piece that is not 16-byte aligned"
        first = off[sel] // 2
        assert (first + 8 <= raw.size).all(), "an offset past the end of the operand"
        vals[sel] = raw[first[:, None] + np.arange(8)]
    assert np.isin(kind[off >= 0], list(raws)).all()
    return bool((vals == want[rows_of(lin, row)[:, None], (ks * X.BK + c)[:, None] + np.arange(8)]).all())


def gathered_equals_model(rec, bm, bn, plan, raw_a, raw_w, A_want, W_want, nk1=NO_SEG2, raw_a2=None, ph_rows=0):
    """rec: the tool's output for one (case, tile shape).  A_want [tilesM * bm][nk * 64], W_want [phase][tilesN * bn][nk * 64]."""
    tm, tn, nk = plan["tiles_m"], plan["tiles_n"], plan["k_steps"]
    tiles = rec[rec[:, 0] == 3]
    assert (tiles[:, 1] == np.arange(tm * tn)).all()
    assert sorted(zip(tiles[:, 2].tolist(), tiles[:, 3].tolist())) == [(i * bm, j * bn) for i in range(tm) for j in range(tn)]
    m0, n0 = tiles[:, 2], tiles[:, 3]
    act, wgt = rec[rec[:, 0] <= 1], rec[rec[:, 0] == 2]
    assert ((act[:, 0] == 1) == (act[:, 2] >= nk1)).all(), "the second input is read at the k-steps from nk1 on, and only there"
    raws = {0: raw_a} if raw_a2 is None else {0: raw_a, 1: raw_a2}
    ok_a = _gather(act, raws, A_want, lambda lin, row: m0[lin] + row, bm, nk)
    phase_rows = W_want.shape[1]
    ok_w = _gather(wgt, {2: raw_w}, W_want.reshape(-1, W_want.shape[2]),
                   lambda lin, row: (m0[lin] // ph_rows if ph_rows else 0) * phase_rows + n0[lin] + row, bn, nk)
    return ok_a and ok_w


def tile_plans(hip, query, desc, variants=range(1, 11), usable=lambda: True):
    """The distinct tile shapes the planner gives the case over the forced variants: {(bm, bn): plan}."""
    out = {}
    try:
        for v in variants:
            hip.set_igemm_variant(v)
            if usable():
                p = query(desc)
                out.setdefault((p["bm"], p["bn"]), p)
    finally:
        hip.set_igemm_variant(-1)
    return out


def conv_operands(hip, case):
    """One conv case -> (geometry without the tiles, raw buffers, Problem, descriptor)."""
    n_img, H, W, cin, cout, stride, up, pao, split, cin2 = case
    c = X.conv_case(n_img, H, W, cin, cout, stride, up, pao, cin2, 7, 0.5 if cin2 else 1.0)
    p = c["problem"]
    lda, lda2 = cin + 8, (cin2 + 16 if cin2 else 0)
    geom = dict(M=n_img * p.Ho * p.Wo, N=cout, Cin=cin, Ktot=9 * cin + cin2, Hi=H, Wi=W, Ho=p.Ho, Wo=p.Wo, stride=stride, up=up,
                pad=0 if pao else 1, lda=lda, nk1=p.nk1 if cin2 else NO_SEG2, Cin2=cin2, lda2=lda2)
    w = c["w"].reshape(cout, cin, 9).transpose(0, 2, 1).reshape(cout, 9 * cin)          # rcdm_pack_conv3x3: [c_out][tap][c_in]
    raw = dict(raw_a=padded_rows(c["x"].reshape(-1, cin), lda), raw_w=(np.concatenate([w, c["w2"]], axis=1) if cin2 else w).reshape(-1),
               raw_a2=padded_rows(c["x2"].reshape(-1, cin2), lda2) if cin2 else None)
    d = hip.ConvDesc(n_img, H, W, cin, cout, stride, up, lda, cout, cout, 7, c["rps"], cout, 1.0, split, pao, 0, cin2, lda2)
    return geom, raw, p, d


def check_tiles(tool, taps, plans, geom, raw, A_of, W_of, nk1=NO_SEG2, ph_rows=0):
    assert plans
    for (bm, bn), plan in sorted(plans.items()):
        g = dict(geom, nk=plan["k_steps"], tilesM=plan["tiles_m"], tilesN=plan["tiles_n"])
        rec = run_loader(tool, taps, bm, bn, g)
        assert gathered_equals_model(rec, bm, bn, plan, raw["raw_a"], raw["raw_w"], A_of(plan["tiles_m"] * bm), W_of(plan["tiles_n"] * bn),
                                     nk1, raw.get("raw_a2"), ph_rows), f"{bm}x{bn} tile: the gathered operands are not the model's"
    return sorted(plans)


@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in X.GEMM_CASES}))
def test_loader_gemm_operands(hip, loader_tool, M, N, K):
    c = X.gemm_case(M, N, K, 1, 1.0)
    p = c["problem"]
    d = hip.GemmDesc(M, N, K, K + 8, N + 16, N + 8, 1, c["rps"], N + 8, 1.0, 1)
    geom = dict(M=M, N=N, Cin=K, Ktot=K, lda=K + 8)
    raw = dict(raw_a=padded_rows(c["A"], K + 8), raw_w=c["W"].reshape(-1))
    shapes = check_tiles(loader_tool, 1, tile_plans(hip, hip.gemm_plan_query, d), geom, raw,
                         lambda rows: in_k_steps(p.A, p.steps, rows), lambda rows: in_k_steps(p.W, p.steps, rows)[None])
    assert len(shapes) == 7, shapes       # 64x64, 128x64, 128x128, 160x160, 160x256, 160x320, 256x256


@pytest.mark.parametrize("case", sorted({c[:8] + (1,) + c[9:] for c in X.CONV_CASES + X.ADD1X1_CASES}), ids=lambda c: "-".join(map(str, c)))
def test_loader_conv_operands(hip, loader_tool, case):
    geom, raw, p, d = conv_operands(hip, case)
    shapes = check_tiles(loader_tool, 9, tile_plans(hip, hip.conv3x3_plan_query, d), geom, raw,
                         lambda rows: in_k_steps(p.A, p.steps, rows), lambda rows: in_k_steps(p.W, p.steps, rows)[None], geom["nk1"])
    assert len(shapes) == 7, shapes


@pytest.mark.parametrize("n_img,H,W,cin,cout", sorted({c[:5] for c in X.UP2_CASES}))
def test_loader_up2_operands(hip, loader_tool, n_img, H, W, cin, cout):
    """The phase form (TAPS = 4) on the ping-pong tiles whose rows divide a phase."""
    c = X.up2_case(n_img, H, W, cin, cout)
    probs = c["problems"]
    lda, src = cin + 8, n_img * H * W
    d = hip.ConvDesc(n_img, H, W, cin, cout, 1, 2, lda, cout, 0, X.EPI_BIAS, 1, 0, 1.0, 1)
    geom = dict(M=4 * src, N=cout, Cin=cin, Ktot=4 * cin, Hi=H, Wi=W, Ho=H, Wo=W, lda=lda, ph_rows=src)
    raw = dict(raw_a=padded_rows(c["x"].reshape(-1, cin), lda), raw_w=X.up2_pack(c["w"]).reshape(-1))
    plans = tile_plans(hip, hip.conv3x3_plan_query, d, (6, 7, 8), lambda: hip.conv3x3_up2_supported(d))
    A = np.concatenate([q.A for q in probs])                      # virtual row = phase * ph_rows + source pixel
    shapes = check_tiles(loader_tool, 4, plans, geom, raw, lambda rows: in_k_steps(A, probs[0].steps, rows),
                         lambda rows: np.stack([in_k_steps(q.W, q.steps, rows) for q in probs]), ph_rows=src)
    assert all(src % bm == 0 for bm, _ in shapes) and (160, 320) in shapes


@pytest.mark.parametrize("tiles_m,tiles_n", [(1, 1), (3, 5), (9, 2), (17, 7), (8, 8), (1, 40)])
def test_loader_tile_order_is_a_bijection(loader_tool, tiles_m, tiles_n):
    for bm, bn in ((64, 64), (160, 320)):
        rec = run_loader(loader_tool, 1, bm, bn, dict(M=tiles_m * bm, N=tiles_n * bn, Cin=64, Ktot=64, lda=64, nk=0, tilesM=tiles_m, tilesN=tiles_n))
        assert (rec[:, 0] == 3).all() and (rec[:, 1] == np.arange(tiles_m * tiles_n)).all()
        hit = sorted(zip(rec[:, 2].tolist(), rec[:, 3].tolist()))
        assert hit == [(i * bm, j * bn) for i in range(tiles_m) for j in range(tiles_n)]        # every tile once


def test_mutation_moved_border_tap(hip, loader_tool):
    """One border tap moved: the tap above an image's first pixel, outside the image, reads the pixel itself instead."""
    case = (6, 10, 6, 72, 72, 1, 0, 0, 1, 0)
    geom, raw, p, d = conv_operands(hip, case)
    plan = tile_plans(hip, hip.conv3x3_plan_query, d, (3,))[(64, 64)]
    g = dict(geom, nk=plan["k_steps"], tilesM=plan["tiles_m"], tilesN=plan["tiles_n"])
    rec = run_loader(loader_tool, 9, 64, 64, g)
    check = lambda r: gathered_equals_model(r, 64, 64, plan, raw["raw_a"], raw["raw_w"], in_k_steps(p.A, p.steps, plan["tiles_m"] * 64),
                                            in_k_steps(p.W, p.steps, plan["tiles_n"] * 64)[None])
    assert check(rec)
    piece = lambda ks: np.flatnonzero((rec[:, 0] == 0) & (rec[:, 1] == 0) & (rec[:, 2] == ks) & (rec[:, 3] == 0) & (rec[:, 5] == 0))[0]
    border, below = piece(1), piece(4)        # k-steps 1 and 4: taps (0, 1) and (1, 1) of the first 64 channels
    assert rec[border, 6] == -1 and rec[below, 6] >= 0
    moved = rec.copy()
    moved[border, 6] = rec[below, 6]
    assert not check(moved)


# ---- 4. the Winograd GEMM's work dealing and operand addressing (csrc/wino_loader.h), through the same tool ---------------
def run_wino_loader(tool, n_img, H, W, K, K2, N, lda2, splits, tiles_m, tiles_n, nk):
    args = ["wino"] + [str(v) for v in (n_img, H, W, K, K2, N, lda2, splits, tiles_m, tiles_n, nk)]
    r = subprocess.run([tool] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.fromstring(r.stdout.decode(), dtype=np.int64, sep=" ").reshape(-1, 7)


# (K2, splits, tiles_m, tiles_n, the dealing's path).  WX = (E - 16) * splits * tiles items of the second input, WM = 16 *
# splits * tiles of the positions: both multiples of 8 -> every XCD takes its share of each ("shares"), else one contiguous
# run per XCD over all items ("runs").  E = 16 has WX = 0 and WM a multiple of 16: always "shares"; the last case is the
# same 1 x 3 tiling with a second input, where WX = 12.
@pytest.mark.parametrize("K2,splits,tiles_m,tiles_n,path", [(128, 2, 2, 2, "shares"), (0, 1, 1, 3, "shares"), (128, 3, 1, 1, "runs"),
                                                           (128, 1, 1, 3, "runs")])
def test_wino_items_are_a_bijection(loader_tool, K2, splits, tiles_m, tiles_n, path):
    E, tiles = (20 if K2 else 16), tiles_m * tiles_n
    WX, WM = (E - 16) * splits * tiles, 16 * splits * tiles
    assert ("shares" if (WX | WM) % 8 == 0 else "runs") == path
    rec = run_wino_loader(loader_tool, 2, 4, 4, 64, K2, 16, K2 + 16 if K2 else 0, splits, tiles_m, tiles_n, 0)
    assert (rec[:, 0] == 3).all() and (rec[:, 1] == np.arange(E * splits * tiles)).all() and (rec[:, 6] == 0).all()
    hit = sorted(zip(rec[:, 4].tolist(), rec[:, 5].tolist(), rec[:, 2].tolist(), rec[:, 3].tolist()))
    assert hit == [(e, s, i * 160, j * 160) for e in range(E) for s in range(splits) for i in range(tiles_m) for j in range(tiles_n)]
    if path == "runs" and (WX + WM) % 8:                     # a short last run: the XCDs' run lengths differ by one, longer first
        order = {(e, s, m0, n0): k for k, (e, s, m0, n0) in enumerate(
            ((16 + e if e < E - 16 else e - (E - 16)), s, i * 160, j * 160)
            for e in range(E) for s in range(splits) for j in range(tiles_n) for i in range(tiles_m))}
        item = np.array([order[(e, s, m0, n0)] for e, s, m0, n0 in zip(rec[:, 4].tolist(), rec[:, 5].tolist(), rec[:, 2].tolist(), rec[:, 3].tolist())])
        runs = [item[x::8] for x in range(8)]
        assert all((np.diff(r) == 1).all() for r in runs)                      # each XCD: consecutive items
        assert [len(r) for r in runs] == sorted((len(r) for r in runs), reverse=True) and len(runs[0]) - len(runs[7]) == 1
        assert all(runs[x + 1][0] == runs[x][-1] + 1 for x in range(7))


def test_wino_loader_operands(loader_tool):
    """n_img = 2, H = W = 4 (T = 8 tiles), K = 64, K2 = 128, N = 16, two k-steps walked for every entry: gathering through the
    printed offsets gives the model's V / U panels and, for entries 16 + 2a + b, the (2ty + a, 2tx + b) pixels of the second
    input against W2; tile rows past T, weight rows past N and (positions, second k-step) channels past K are out of bounds."""
    n_img, H, W, K, K2, N, nk = 2, 4, 4, 64, 128, 16, 2
    lda2, T = K2 + 16, n_img * (H // 2) * (W // 2)
    c = X.wino_case(n_img, H, W, K, K2, N, 0, 1.0, False)
    _, _, V, U = X.wino_model(c["x_eff"], c["w"], 1, c["x2"], c["w2"])
    rec = run_wino_loader(loader_tool, n_img, H, W, K, K2, N, lda2, 1, 1, 1, nk)
    items = rec[rec[:, 0] == 3]
    assert sorted(items[:, 4].tolist()) == list(range(20)) and (items[:, 2] == 0).all() and (items[:, 3] == 0).all()
    raw_x2 = padded_rows(c["x2"].reshape(-1, K2), lda2)

    def panel(mat):              # [rows][Kd] -> what the tile sees: [160][nk * 64], zeros past the rows and past Kd
        out = np.zeros((160, nk * X.BK))
        out[:mat.shape[0], :mat.shape[1]] = mat
        return out

    seen_oob = set()
    for lin, entry in zip(items[:, 1].tolist(), items[:, 4].tolist()):
        mine = rec[(rec[:, 0] != 3) & (rec[:, 1] == lin)].copy()
        mine[:, 1] = 0
        act, wgt = mine[mine[:, 0] <= 1], mine[mine[:, 0] == 2]
        if entry < 16:
            a_kind, raw_a, want_a = 0, V[entry // 4, entry % 4].reshape(-1), panel(V[entry // 4, entry % 4])
            raw_w, want_w, Kd = U[entry // 4, entry % 4].reshape(-1), panel(U[entry // 4, entry % 4]), K
        else:
            a, b = (entry - 16) >> 1, (entry - 16) & 1
            a_kind, raw_a, want_a = 1, raw_x2, panel(c["x2"][:, a::2, b::2].reshape(T, K2))
            raw_w, want_w, Kd = c["w2"].reshape(-1), panel(c["w2"]), K2
        assert (act[:, 0] == a_kind).all()
        rows_of = lambda lin_, row: row
        assert _gather(act, {a_kind: raw_a}, want_a, rows_of, 160, nk), f"entry {entry}: the gathered A operand is not the model's"
        assert _gather(wgt, {2: raw_w}, want_w, rows_of, 160, nk), f"entry {entry}: the gathered weight operand is not the model's"
        for r, rows, what in ((act, T, "tile row past T"), (wgt, N, "weight row past N")):
            inside = (r[:, 3] < rows) & (r[:, 2] * X.BK + r[:, 5] < Kd)
            assert (r[inside, 6] >= 0).all() and (r[~inside, 6] == -1).all()
            if (r[:, 3] >= rows).any():
                seen_oob.add(what)
            if (r[:, 2] * X.BK + r[:, 5] >= Kd).any():
                seen_oob.add("channel chunk past Kd")
    assert seen_oob == {"tile row past T", "weight row past N", "channel chunk past Kd"}
