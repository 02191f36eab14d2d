"""CPU: the scores from logits before a GPU runs them.  The label figures (rcdms_amd.scores.label_scores and the exact-fraction
model of tests/scores_oracle.py) against scikit-learn on random cases; the Inception-Score model against the 60-digit goldens
(tools/mint_scores_golden.py) within the a-priori bound B, against closed forms and against the two-pass definition; the shared
core csrc/scores_core.h compiled into tools/scores_host.cpp — the label state exactly, KL to the model's bits where libm's exp
and log agree with numpy's and within B otherwise; the split boundaries; and the argument checks of the new entry points and of
the Python layer, which need no device."""
import ctypes
import math
import os
import subprocess
from decimal import Decimal, localcontext

import numpy as np
import pytest

from tests import scores_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_label_state_len", "rcdm_label_counts_workspace_bytes", "rcdm_label_counts",
               "rcdm_inception_score_workspace_bytes", "rcdm_inception_score")
SKLEARN_SHAPES = [(1, 5), (7, 257), (9, 1000), (64, 300)]           # (C, N)


def error_to_digits(value, digits):
    """|value - the 50-digit decimal| without rounding the reference to float64 first."""
    with localcontext() as ctx:
        ctx.prec = 80
        return float(abs(Decimal(float(value)) - Decimal(str(digits))))


# ------------------------------------------------------------------------------------------------ label figures
@pytest.mark.parametrize("C,N", SKLEARN_SHAPES)
@pytest.mark.parametrize("zero_division", [0, 1])
def test_figures_against_sklearn(C, N, zero_division):
    metrics = pytest.importorskip("sklearn.metrics")
    from rcdms_amd.scores import label_scores
    z, y, thr = O.label_inputs(C, N, 31 * C + N, thresholds=C == 9)
    state = O.label_state(z, y, thr)
    true, pred = (y != 0).astype(np.int64), O.predictions(z, thr)
    assert C == 1 or true[:, C - 1].sum() == 0                     # a never-present class
    assert N < 5 or ((true.sum(axis=1) == 0) & (pred.sum(axis=1) == 0)).any()      # empty rows predicted empty
    exact, got = O.figures(state, C, zero_division), label_scores(state, C, zero_division)
    kw = dict(zero_division=zero_division)
    scale = 1
    if C == 1:          # scikit-learn reads a dense (N, 1) array as a binary column: give it a second, empty class and keep it out
        true, pred = (np.concatenate([a, np.zeros_like(a)], axis=1) for a in (true, pred))      # of the averages by labels=[0]
        kw["labels"] = [0]
        scale = 2       # hamming_loss takes no labels: the empty class doubles its denominator, exactly
    want = {
        "frame_accuracy": metrics.accuracy_score(true, pred),
        "hamming": scale * metrics.hamming_loss(true, pred),
        "f1_micro": metrics.f1_score(true, pred, average="micro", **kw),
        "f1_macro": metrics.f1_score(true, pred, average="macro", **kw),
        "f1_weighted": metrics.f1_score(true, pred, average="weighted", **kw),
        "f1_samples": metrics.f1_score(true, pred, average="samples", **kw),
    }
    # three evaluations of one rational number: the exact one rounded once, ours (fsum: within two roundings), scikit-learn's
    # (a float64 mean of k values in [0, 1] in its own order: within k 2^-53)
    terms = {"frame_accuracy": N, "hamming": N * C, "f1_micro": 2, "f1_macro": C + 2, "f1_weighted": C + 2, "f1_samples": N}
    for key, w in want.items():
        print(f"C {C} N {N} zd {zero_division} {key}: exact {exact[key]:.17g}, ours {getattr(got, key):.17g}, sklearn {w:.17g}")
        assert abs(getattr(got, key) - exact[key]) <= 2 * O.U
        assert abs(w - exact[key]) <= O.mean_tolerance(terms[key])
    p, r, f, s = metrics.precision_recall_fscore_support(true, pred, average=None, **kw)
    assert np.array_equal(got.support, s) and np.array_equal(exact["support"], s)
    for ours, ex, sk in ((got.precision, exact["precision"], p), (got.recall, exact["recall"], r), (got.f1, exact["f1"], f)):
        assert np.array_equal(ours, ex) and np.abs(sk - ex).max() <= 2 * O.U
    assert got.n == N and got.hist.shape == (C + 1, C + 1) and int(got.hist.sum()) == N
    assert np.array_equal(got.tp + got.fn, got.support)


def test_label_goldens_and_mistakes():
    changed = {"ge": 0, "nan1": 0, "label1": 0}
    for name in O.LABEL_CASES:
        g = O.load_labels(name)
        thr = g.get("thresholds")
        assert np.array_equal(O.label_state(g["logits"], g["labels"], thr), g["state"])
        assert g["state"].dtype == np.int64 and g["state"].shape == (O.state_len(g["logits"].shape[1]),)
        for rule in changed:
            assert np.array_equal(O.label_state(g["logits"], g["labels"], thr, rule=rule), g[f"state_{rule}"])
            changed[rule] += not np.array_equal(g[f"state_{rule}"], g["state"])
    assert all(v >= 3 for v in changed.values()), changed           # each mistake shows on the three larger cases
    g = O.load_labels("c7_n257")
    assert np.isnan(g["logits"]).any() and (g["logits"] == 0.0).any() and set(np.unique(g["labels"]).tolist()) == {0, 1, 255}
    assert "thresholds" in O.load_labels("c9_n1000")


def test_state_merges_by_addition_and_zero_division():
    from rcdms_amd.scores import label_scores, label_state_len
    z, y, _ = O.label_inputs(7, 100, 3)
    whole = O.label_state(z, y)
    assert np.array_equal(O.label_state(z[:37], y[:37]) + O.label_state(z[37:], y[37:]), whole)
    assert label_state_len(7) == O.state_len(7) == 1 + 21 + 64
    # all-negative rows with no labels: every quotient is 0 / 0
    empty = O.label_state(np.full((4, 3), -1.0, np.float32), np.zeros((4, 3), np.uint8))
    for zd in (0, 1):
        r = label_scores(empty, 3, zd)
        assert r.frame_accuracy == 1.0 and r.hamming == 0.0
        assert (r.f1_micro, r.f1_macro, r.f1_weighted, r.f1_samples) == (float(zd),) * 4
        assert np.array_equal(r.precision, np.full(3, float(zd))) and np.array_equal(r.support, np.zeros(3, np.int64))
    # the documented deviation: round(sigmoid(x)) in float32 is 0 for 0 < x <~ 6e-8, the rule here says 1
    import torch
    x = torch.tensor([1e-8, 6e-8, 1.2e-7])
    assert torch.round(torch.sigmoid(x)).tolist() == [0.0, 0.0, 1.0] and O.predictions(x.numpy()[None, :])[0].tolist() == [1, 1, 1]
    for bad in (np.zeros(5, np.int64), np.zeros(O.state_len(3), np.int32)):
        with pytest.raises(ValueError):
            label_scores(bad, 3)
    with pytest.raises(ValueError, match="no rows"):
        label_scores(np.zeros(O.state_len(3), np.int64), 3)
    with pytest.raises(ValueError):
        label_scores(empty, 3, zero_division=0.5)


# ------------------------------------------------------------------------------------------------ Inception Score: the model
def test_cases_cover_the_grid():
    for c in (2, 7, 1000, 1008):
        for s in (1, 3, 10):
            for n in (s, 23, 257):
                assert O.ISC_CASES[f"c{c}_n{n}_s{s}"] == (c, n, s, None)
    z = O.isc_logits(64, 23, "span80")
    assert z.min() < -70 and z.max() > 70
    z = O.isc_logits(100, 23, "f16")
    assert np.array_equal(z.astype(np.float16).astype(np.float32), z)
    o = O.isc_order("order_c7_n257_s10")
    assert sorted(o.tolist()) == list(range(257)) and not np.array_equal(o, np.arange(257))
    for name in os.listdir(O.GOLDEN):
        if name.startswith(("isc_", "scores_")):
            assert os.path.getsize(os.path.join(O.GOLDEN, name)) < 200_000, name


@pytest.mark.parametrize("name", list(O.ISC_CASES))
def test_model_against_the_60_digit_value(name):
    g = O.load_isc(name)
    B = O.bound(g["logits"], g["splits"])
    assert np.array_equal(B, g["bound"])                     # a-priori: a function of the inputs alone
    model = O.evaluate(g["logits"], g["splits"], g["order"])
    for k in range(g["splits"]):
        err = error_to_digits(model[k], g["kl_digits"][k])
        print(f"{name}[{k}]: model {model[k]:.17g}, mpmath {g['kl_digits'][k]}, |diff| {err:.3e} = {err / B[k]:.2e} B")
        assert err <= B[k]
    # against the file's model figures: the same bits unless the numpy at hand rounds an exp or a log the other way
    assert O.same_bits(model, g["model"]) or np.all(np.abs(model - g["model"]) <= 2 * B)
    assert np.all(np.abs(O.two_pass(g["logits"], g["splits"], g["order"]) - model) <= 2 * B)      # the one-pass form is the definition


def test_closed_forms():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    # identical rows: every row is the mean, KL is 0
    g = O.load_isc("equal_c7_n23_s3")
    assert all(abs(float(v)) < 1e-55 for v in g["kl_digits"])               # 0 to the 60 digits of the minting
    assert np.all(np.abs(O.evaluate(g["logits"], 3)) <= g["bound"])
    # one-hot by a margin, cycling through the classes: the mean is uniform
    for C, reps, margin, splits in ((7, 3, 3.0, 1), (7, 2, 3.0, 4), (2, 5, 0.5, 1), (1000, 1, 12.0, 1), (9, 29, 40.0, 3)):
        z = O.one_hot_rows(C, C * reps * splits, margin)
        want, B = O.one_hot_kl(C, margin, mp), O.bound(z, splits)
        got = O.evaluate(z, splits)
        for k in range(splits):
            err = float(abs(mp.mpf(float(got[k])) - want))
            print(f"one-hot C {C} margin {margin}: KL {got[k]:.17g}, |diff| {err:.3e} = {err / B[k]:.2e} B")
            assert err <= B[k]
    assert float(O.one_hot_kl(7, 40.0, mp)) == pytest.approx(math.log(7), rel=1e-12)          # confident and diverse: IS -> C


def test_split_boundaries():
    assert O.split_bounds(23, 10) == [(0, 2), (2, 4), (4, 6), (6, 9), (9, 11), (11, 13), (13, 16), (16, 18), (18, 20), (20, 23)]
    sizes = [b - a for a, b in O.split_bounds(23, 10)]
    assert sorted(set(sizes)) == [2, 3] and sum(sizes) == 23
    assert O.split_bounds(10, 10) == [(k, k + 1) for k in range(10)] and O.split_bounds(257, 1) == [(0, 257)]
    # a row moved across a boundary changes both neighbours: split k really is positions [k N // splits, (k + 1) N // splits)
    z = O.isc_logits(7, 23)
    base = O.evaluate(z, 10)
    swapped = np.arange(23)
    swapped[[5, 6]] = [6, 5]                                     # position 5 ends split 2, position 6 starts split 3
    moved = O.evaluate(z, 10, swapped)
    assert moved[2] != base[2] and moved[3] != base[3] and O.same_bits(np.delete(moved, [2, 3]), np.delete(base, [2, 3]))
    inside = np.arange(23)
    inside[[6, 7]] = [7, 6]                                      # both inside split 3: the set is the same, the order is not
    assert np.all(np.abs(O.evaluate(z, 10, inside) - base) <= O.bound(z, 10))


def test_shuffle_rule():
    from rcdms_amd.scores import shuffled_order
    o = shuffled_order(257, O.ORDER_SEED)
    assert o.dtype == np.int32 and np.array_equal(o, O.isc_order("order_c7_n257_s10"))
    assert np.array_equal(o, np.random.RandomState(O.ORDER_SEED).permutation(257))


# ------------------------------------------------------------------------------------------------ the classifier input
def test_every_byte_normalises_as_torchvision_does():
    """The kernel's (u8 (1 / 255) - mean) (1 / std) and torchvision's (u8 / 255 - mean) / std in float32 round to the same f16 for
    all 256 bytes under both sets of constants: the bit-for-bit claim does not hang on the frames of this file."""
    from rcdms_amd import inception as I
    u, f = np.arange(256, dtype=np.float32), np.float32
    for mean, std in ((I.IMAGENET_MEAN, I.IMAGENET_STD), (I.TRANSFORM_INPUT_MEAN, I.TRANSFORM_INPUT_STD)):
        for m, s in zip(mean, std):
            kernel = ((u * (f(1) / f(255)) - f(m)) * (f(1) / f(s))).astype(np.float16)
            assert np.array_equal(kernel.view(np.int16), ((u / f(255) - f(m)) / f(s)).astype(np.float16).view(np.int16))
    # transform_input folds: ((v - m) / s) (s / 0.5) + (m - 0.5) / 0.5 = (v - 0.5) / 0.5
    v = np.linspace(0.0, 1.0, 256)
    for m, s in zip(I.IMAGENET_MEAN, I.IMAGENET_STD):
        assert np.abs(((v - m) / s) * (s / 0.5) + (m - 0.5) / 0.5 - (v - 0.5) / 0.5).max() < 1e-14


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/scores_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("scores") / "scores_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "scores_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def run_labels(host_tool, tmp_path, z, y, thr):
    paths = [str(tmp_path / "z.raw"), str(tmp_path / "y.raw")]
    np.ascontiguousarray(z, np.float32).tofile(paths[0])
    np.ascontiguousarray(y, np.uint8).tofile(paths[1])
    if thr is not None:
        paths.append(str(tmp_path / "t.raw"))
        np.ascontiguousarray(thr, np.float32).tofile(paths[2])
    r = subprocess.run([host_tool, "labels", str(z.shape[0]), str(z.shape[1]), *paths], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([int(v) for v in r.stdout.split()], np.int64)


def run_isc(host_tool, tmp_path, z, splits, order):
    paths = [str(tmp_path / "z.raw")]
    np.ascontiguousarray(z, np.float64).tofile(paths[0])
    if order is not None:
        paths.append(str(tmp_path / "o.raw"))
        np.ascontiguousarray(order, np.int32).tofile(paths[1])
    r = subprocess.run([host_tool, "isc", str(z.shape[0]), str(z.shape[1]), str(splits), *paths], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([float(v) for v in r.stdout.split()])


@pytest.mark.parametrize("name", list(O.LABEL_CASES))
def test_host_tool_label_state_is_exact(host_tool, tmp_path, name):
    g = O.load_labels(name)
    assert np.array_equal(run_labels(host_tool, tmp_path, g["logits"], g["labels"], g.get("thresholds")), g["state"])


def test_host_tool_label_state_across_blocks(host_tool, tmp_path):
    z, y, thr = O.label_inputs(9, 2500, 77, thresholds=True)                # ten blocks of 256 rows, the last ragged
    assert np.array_equal(run_labels(host_tool, tmp_path, z, y, thr), O.label_state(z, y, thr))


@pytest.mark.parametrize("name", [n for n, v in O.ISC_CASES.items() if v[1] <= 23 or v[0] <= 7])
def test_host_tool_inception_score(host_tool, tmp_path, name):
    g = O.load_isc(name)
    got = run_isc(host_tool, tmp_path, g["logits"], g["splits"], g["order"])
    model = O.evaluate(g["logits"], g["splits"], g["order"])
    same = O.same_bits(got, model)
    print(f"{name}: host tool {'has the model bits' if same else 'differs from the model (libm against numpy)'}")
    for k in range(g["splits"]):
        assert error_to_digits(got[k], g["kl_digits"][k]) <= g["bound"][k]
    assert same or np.all(np.abs(got - model) <= 2 * g["bound"])


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(6).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run("isc", "3", "2", "1", p)
    assert r.returncode == 0 and len(r.stdout.split()) == 1
    assert run("isc", "3", "2", "4", p).returncode == 2                  # more splits than rows
    assert run("isc", "6", "1", "1", p).returncode == 2                  # one class
    r = run("isc", "3", "3", "1", p)
    assert r.returncode == 2 and b"exactly" in r.stderr
    q = str(tmp_path / "o.raw")
    np.array([0, 1, 3], np.int32).tofile(q)
    r = run("isc", "3", "2", "1", p, q)
    assert r.returncode == 2 and b"outside" in r.stderr
    assert run("labels", "3", "65", p, p).returncode == 2
    assert run("labels", "3", "2", p, p).returncode == 2                 # 48 bytes are neither 6 float32 nor 6 labels
    r = run("nothing")
    assert r.returncode == 2 and b"usage" in r.stderr


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in NEW_SYMBOLS:
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.LabelDesc) == 32 and hip.LabelDesc.n.offset == 16 and hip.LabelDesc.flags.offset == 28
    assert ctypes.sizeof(hip.IscDesc) == 32 and hip.IscDesc.n.offset == 8 and hip.IscDesc.flags.offset == 28
    assert lib.rcdm_version() == 0x000300
    for c in (1, 7, 9, 64):
        assert lib.rcdm_label_state_len(c) == O.state_len(c)
    assert lib.rcdm_label_state_len(0) == 0 and lib.rcdm_label_state_len(65) == 0


def test_argument_validation_without_gpu():
    """The entry points refuse bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    F32, F16 = hip.FSTATS_F32, hip.FSTATS_F16

    def ldesc(ldz=12, ldl=9, n=100, classes=9, dtype=F32, flags=0):
        return hip.LabelDesc(ldz, ldl, n, classes, dtype, flags)

    lws = lambda d: lib.rcdm_label_counts_workspace_bytes(ctypes.byref(d))
    assert lws(ldesc()) == 1 * O.state_len(9) * 4 and lws(ldesc(n=1025)) == 5 * O.state_len(9) * 4
    assert lws(ldesc(classes=1, ldz=1, ldl=1)) == 32                         # 8 int32
    assert lws(ldesc(classes=2, ldz=2, ldl=2)) == 64                         # 16 int32
    assert lws(ldesc(classes=4, ldz=4, ldl=4)) == 152                        # 37 int32 = 148 bytes, rounded up to 8
    invalid = (ldesc(n=0), ldesc(classes=0), ldesc(ldz=8), ldesc(ldl=8), ldesc(dtype=7), ldesc(flags=1))
    shape = (ldesc(classes=65, ldz=65, ldl=65), ldesc(n=(1 << 30) + 1))
    for bad in invalid + shape:
        assert lws(bad) == 0
    assert lib.rcdm_label_counts_workspace_bytes(None) == 0
    z, y, t, s, ws, st = 0x1000, 0x2001, 0x3000, 0x4000, 0x5000, 0                # never dereferenced; labels need no alignment
    count = lambda d, *a: lib.rcdm_label_counts(ctypes.byref(d), *a)
    good, nb = ldesc(), lws(ldesc())
    for bad in invalid:
        assert count(bad, z, y, t, s, ws, 1 << 20, st) == EINVAL
    for bad in shape:
        assert count(bad, z, y, t, s, ws, 1 << 40, st) == ESHAPE
    assert lib.rcdm_label_counts(None, z, y, t, s, ws, nb, st) == EINVAL
    for a in ((0, y, t, s), (z, 0, t, s), (z, y, t, 0)):                          # null pointers (thresholds may be null)
        assert count(good, *a, ws, nb, st) == EINVAL
    assert count(good, z + 2, y, t, s, ws, nb, st) == EINVAL and count(ldesc(dtype=F16), z + 1, y, t, s, ws, nb, st) == EINVAL
    assert count(good, z, y, t + 2, s, ws, nb, st) == EINVAL and count(good, z, y, t, s + 4, ws, nb, st) == EINVAL
    assert count(good, z, y, t, s, ws + 4, nb, st) == EINVAL
    assert count(good, z, y, t, s, 0, nb, st) == EWORKSPACE and count(good, z, y, 0, s, ws, nb - 8, st) == EWORKSPACE

    def idesc(ld=1008, n=257, classes=1008, splits=10, dtype=F32, cpb=0, flags=0):
        return hip.IscDesc(ld, n, classes, splits, dtype, cpb, flags)

    iws = lambda d: lib.rcdm_inception_score_workspace_bytes(ctypes.byref(d))
    assert iws(idesc()) == (3 * 257 + 10 * 1 * 1009) * 8
    assert iws(idesc(n=11040)) == (3 * 11040 + 10 * 5 * 1009) * 8 and iws(idesc(n=10)) == (30 + 10 * 1009) * 8
    invalid = (idesc(n=0), idesc(classes=0), idesc(splits=0), idesc(splits=258), idesc(ld=1007), idesc(dtype=7), idesc(cpb=-1),
               idesc(cpb=65), idesc(flags=1))
    shape = (idesc(classes=1, ld=1), idesc(classes=4097, ld=4097), idesc(n=(1 << 30) + 1), idesc(n=70000, splits=65536))
    for bad in invalid + shape:
        assert iws(bad) == 0
    assert lib.rcdm_inception_score_workspace_bytes(None) == 0
    o, out, rh = 0x3000, 0x4000, 0x6000
    isc = lambda d, *a: lib.rcdm_inception_score(ctypes.byref(d), *a)
    good, nb = idesc(), iws(idesc())
    for bad in invalid:
        assert isc(bad, z, o, out, rh, ws, 1 << 30, st) == EINVAL
    for bad in shape:
        assert isc(bad, z, o, out, rh, ws, 1 << 40, st) == ESHAPE
    assert lib.rcdm_inception_score(None, z, o, out, rh, ws, nb, st) == EINVAL
    assert isc(good, 0, o, out, rh, ws, nb, st) == EINVAL and isc(good, z, o, 0, rh, ws, nb, st) == EINVAL
    assert isc(good, z + 2, o, out, rh, ws, nb, st) == EINVAL and isc(idesc(dtype=F16), z + 1, o, out, rh, ws, nb, st) == EINVAL
    assert isc(good, z, o + 2, out, rh, ws, nb, st) == EINVAL and isc(good, z, o, out + 4, rh, ws, nb, st) == EINVAL
    assert isc(good, z, o, out, rh + 4, ws, nb, st) == EINVAL and isc(good, z, o, out, rh, ws + 4, nb, st) == EINVAL
    assert isc(good, z, 0, out, 0, 0, nb, st) == EWORKSPACE and isc(good, z, 0, out, 0, ws, nb - 8, st) == EWORKSPACE


def test_python_layer_refuses_before_any_device_access(tmp_path):
    import torch
    from rcdms_amd import hip
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.scores import LabelCounts, inception_score
    with pytest.raises(hip.RcdmError):
        LabelCounts(9, "cpu")
    for bad in (0, 65):
        with pytest.raises(ValueError):
            LabelCounts(bad, "cuda")
    with pytest.raises(ValueError):
        LabelCounts(9, "cuda", thresholds=[0.0] * 8)
    with pytest.raises(ValueError):
        LabelCounts(2, "cuda", thresholds=[0.0, float("nan")])
    lc = LabelCounts(9, "cuda", thresholds=[0.5] * 9)
    assert lc.state() is None
    with pytest.raises(ValueError, match="no rows"):
        lc.result()
    with pytest.raises(ValueError):
        lc.result(zero_division=2)
    z, y = torch.zeros(4, 9), torch.zeros(4, 9, dtype=torch.uint8)
    with pytest.raises(hip.RcdmError):
        lc.update(z, y)
    with pytest.raises(TypeError):
        lc.update(np.zeros((4, 9), np.float32), y)
    with pytest.raises(ValueError):
        lc.merge(LabelCounts(7, "cuda"))
    with pytest.raises(ValueError, match="thresholds"):
        lc.merge(LabelCounts(9, "cuda"))
    np.savez(tmp_path / "bad.npz", label_state=np.zeros(11, np.int64))
    with pytest.raises(ValueError):
        LabelCounts.load(tmp_path / "bad.npz", "cuda")
    np.savez(tmp_path / "bad2.npz", label_state=np.zeros(O.state_len(9), np.float64))
    with pytest.raises(ValueError):
        LabelCounts.load(tmp_path / "bad2.npz", "cuda")
    lc.save(tmp_path / "empty.npz")
    with np.load(tmp_path / "empty.npz") as f:
        assert sorted(f.files) == ["label_state", "thresholds"] and not f["label_state"].any()

    host = torch.zeros(30, 7)
    with pytest.raises(hip.RcdmError):
        inception_score(host)
    with pytest.raises(TypeError):
        inception_score(np.zeros((30, 7), np.float32))
    for bad, kw in ((torch.zeros(30, 1), {}), (torch.zeros(30, 4097), {}), (torch.zeros(5, 7), {}), (host, {"splits": 0}),
                    (host.double(), {}), (torch.zeros(30), {}), (host, {"chunks_per_block": 65}), (host, {"order": list(range(29))}),
                    (host, {"order": [0] * 29 + [30]}), (host, {"order": np.zeros(30)}), (host, {"order": list(range(30)), "shuffle_seed": 1})):
        with pytest.raises(ValueError):
            inception_score(bad, **kw)
    with pytest.raises(ValueError, match="no rows"):
        inception_score(FeatureBank(7, "cuda"))
