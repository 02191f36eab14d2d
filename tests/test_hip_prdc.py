"""GPU: rcdms_amd.prdc and the kernels under it (csrc/prdc.hip), in guarded buffers (tests/guard.py).

  exact        integer features in -3 .. 3, centred (an unmasked padded row — the zero vector — is then a near neighbour), at sizes
               around the tile, both dtypes, a pitch that takes the 16-byte loads and one that does not, col_chunks 1, 2 and 3
               (more chunks than tile columns included): r2, fake_count, real_hit, real_min2 and the four numerators equal the
               Python-int reference ELEMENT BY ELEMENT, bit for bit.  Totals are invariant under row permutations; only the
               per-sample vectors pin the lane maps.  tests/test_prdc_host.py shows that the strict rule, one extra zero row and
               `<` on coverage each change a count on every one of these shapes.
  edges        n = k + 1; nx < 64 < ny and the reverse; real is fake (one buffer); three identical rows with k = 2.
  independence two runs of one call have the same bits; results do not depend on col_chunks (non-integer features).
  goldens      counts and per-sample integers equal, radii and minima within the a-priori bound of the exact values.
  Python       manifold_metrics on banks and tensors, the cached FeatureBank.radii2, knn_radii2 alone, a story-sized case."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import guard as G
from tests import prdc_oracle as O
from tests.test_hip_frechet import _Recorder
from tests.test_kid_host import error_to_digits
from tests.test_story_gpu import DEV

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16}
GR = 8                                          # guard rows around every operand
CHUNKS = (1, 2, 3)


def pitches(d):
    """One pitch that keeps rows 16-byte aligned (the vector loads) and one that does not; both > d."""
    return ((d + 3) // 4 * 4 + 4, (d + 3) // 4 * 4 + 3)


@functools.lru_cache(maxsize=None)
def integer_case(nx, ny, d, k):
    """(x, y, the Python-int reference), computed once per shape and left unchanged."""
    x, y = O.integer_pair(nx, ny, d)
    return x, y, O.integer_reference(x, y, k)


def rows_in(a, dtype, ld):
    return G.guarded_in(torch.from_numpy(np.asarray(a, np.float32)).to(dtype), ld, device=DEV, guard_rows=GR)


def code(hip, dtype):
    return hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32


def vec_out(n, dtype):
    return G.guarded_out(1, n, n + 3, dtype, device=DEV, guard_rows=GR)


def run_radii(hip, xv, n, d, ld, k, dtype, chunks):
    """rcdm_knn_radii2 on a guarded operand -> (the guarded r2 view, handles)."""
    desc = hip.KnnDesc(ld, n, d, k, code(hip, dtype), chunks, 0)
    need = hip.knn_radii2_workspace_bytes(desc)
    assert need == (n + chunks * n * k) * 8 if chunks else need >= (n + n * k) * 8          # 0: the library's choice
    rv, rh = vec_out(n, torch.float64)
    wv, wh = vec_out(need // 8, torch.float64)                # NaN-filled: nothing relies on a cleared workspace
    hip.knn_radii2(desc, xv.data_ptr(), rv.data_ptr(), wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_written(rh)
    return rv, (rh, wh)


def run_all(hip, x, y, k, dtype, ldx, ldy, chunks, same=False):
    """Both radius sweeps and the count sweep on guarded buffers -> (result dict of numpy arrays, handles)."""
    nx, ny, d = x.shape[0], y.shape[0], x.shape[1]
    xv, xh = rows_in(x, dtype, ldx)
    yv, yh = (xv, xh) if same else rows_in(y, dtype, ldy)
    rxv, hx = run_radii(hip, xv, nx, d, ldx, k, dtype, chunks)
    ryv, hy = (rxv, ()) if same else run_radii(hip, yv, ny, d, ldy, k, dtype, chunks)
    desc = hip.PrdcDesc(ldx, ldy, nx, ny, d, code(hip, dtype), chunks, 0)
    need = hip.prdc_counts_workspace_bytes(desc)
    assert need > 0 and need % 8 == 0
    ov, oh = vec_out(4, torch.int64)
    fv, fh = vec_out(ny, torch.int32)
    hv, hh = vec_out(nx, torch.int32)
    mv, mh = vec_out(nx, torch.float64)
    wv, wh = vec_out(need // 8, torch.float64)
    hip.prdc_counts(desc, xv.data_ptr(), yv.data_ptr(), rxv.data_ptr(), ryv.data_ptr(), ov.data_ptr(), fv.data_ptr(), hv.data_ptr(),
                    mv.data_ptr(), wv.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_written(mh)
    got = {"radii2_real": hx[0].data[0].cpu().numpy(), "radii2_fake": (hx if same else hy)[0].data[0].cpu().numpy(),
           "fake_count": fh.data[0].cpu().numpy(), "real_hit": hh.data[0].cpu().numpy(), "real_min2": mh.data[0].cpu().numpy(),
           "counts": oh.data[0].cpu().numpy()}
    return got, (xh, yh, *hx, *hy, oh, fh, hh, mh, wh)


def assert_same(got, want, what):
    for key in ("radii2_real", "radii2_fake", "real_min2"):
        assert O.same_bits(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].ravel(), got[key][:8], want[key][:8])
    for key in ("fake_count", "real_hit", "counts"):
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].ravel(), got[key][:8], want[key][:8])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("shape", O.INTEGER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_cases_are_exact(hiplib, shape, dtype):
    from rcdms_amd import hip
    nx, ny, d, k = shape
    x, y, want = integer_case(*shape)
    for ld in pitches(d):
        for chunks in CHUNKS:
            got, handles = run_all(hip, x, y, k, DTYPES[dtype], ld, ld + 4, chunks)
            assert_same(got, want, (ld, chunks))
            G.check_all(*handles)


@pytest.mark.parametrize("shape", [(4, 4, 2, 3), (17, 18, 5, 16), (40, 100, 7, 5), (100, 40, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_edges(hiplib, shape):
    """n = k + 1: every other row is a neighbour; one set inside a tile and the other beyond it."""
    from rcdms_amd import hip
    nx, ny, d, k = shape
    x, y = O.integer_features(nx, d, 31 * nx + d), O.integer_features(ny, d, 37 * ny + d)
    want = O.integer_reference(x, y, k)
    for ld, chunks in zip(pitches(d), (1, 2)):
        got, handles = run_all(hip, x, y, k, torch.float32, ld, ld, chunks)
        assert_same(got, want, (ld, chunks))
        G.check_all(*handles)


def test_real_is_fake(hiplib):
    from rcdms_amd import hip
    x = O.integer_features(70, 6, 5)
    want = O.integer_reference(x, x, 5)
    assert tuple(want["counts"][[0, 1, 3]]) == (70, 70, 70)                      # a set covers itself
    got, handles = run_all(hip, x, x, 5, torch.float16, 8, 8, 2, same=True)
    assert_same(got, want, "one buffer")
    G.check_all(*handles)


def test_identical_rows_have_radius_zero(hiplib):
    """Three identical rows and k = 2: the twins are each other's neighbours at distance 0 (exclusion by position, not by value),
    and the closed ball of radius 0 still holds them."""
    from rcdms_amd import hip
    x, y = O.integer_features(9, 4, 1), O.integer_features(8, 4, 2)
    x[[1, 4, 7]] = x[1]
    y[2] = x[1]
    want = O.integer_reference(x, y, 2)
    assert (want["radii2_real"][[1, 4, 7]] == 0).all() and want["fake_count"][2] >= 3 and (want["real_min2"][[1, 4, 7]] == 0).all()
    got, handles = run_all(hip, x, y, 2, torch.float32, 4, 7, 1)
    assert_same(got, want, "twins")
    G.check_all(*handles)


def test_runs_repeat_and_chunks_do_not_matter(hiplib):
    from rcdms_amd import hip
    g = O.load("n65_70_d130_k5")                                               # non-integer features: the dots are rounded
    args = (g["x"], g["y"], int(g["k"]), torch.float32, 132, 133)
    first, handles = run_all(hip, *args, 1)
    G.check_all(*handles)
    again, _ = run_all(hip, *args, 1)
    assert_same(again, first, "second run")
    for chunks in (0, 2, 3, 7):
        other, handles = run_all(hip, *args, chunks)             # 0: the library's choice
        assert_same(other, first, f"col_chunks {chunks}")
        G.check_all(*handles)


@pytest.mark.parametrize("name", list(O.CASES))
def test_against_the_goldens(hiplib, name):
    from rcdms_amd import hip
    g = O.load(name)
    d, k = g["x"].shape[1], int(g["k"])
    same = name == "self"
    for dtype in ([torch.float32, torch.float16] if name == "f16" else [torch.float32]):
        for ld, chunks in zip(pitches(d), (2, 1)):
            got, handles = run_all(hip, g["x"], g["y"], k, dtype, ld, ld, chunks, same=same)
            for key in ("counts", "fake_count", "real_hit"):
                assert np.array_equal(got[key], g[key]), (key, got[key], g[key])
            for key, digits, B in (("radii2_real", g["radii2_real_digits"], g["bound_real"]),
                                   ("radii2_fake", g["radii2_fake_digits"], g["bound_fake"])):
                err = np.array([error_to_digits(v, s) for v, s in zip(got[key], digits)])
                print(f"{name} ld {ld} {key}: largest |diff| {err.max():.3e}, largest share of its bound {(err / B).max():.2e}")
                assert (err <= B).all()
            assert (np.abs(got["real_min2"] - g["real_min2"]) <= g["bound_min2"]).all()
            G.check_all(*handles)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_manifold_metrics_on_banks_and_tensors(hiplib):
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.prdc import knn_radii2, manifold_metrics
    g = O.load("n33_40_d48_k5")
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    r = manifold_metrics(x, y)                                                   # nearest_k = 5 by default
    assert (r.n_real, r.n_fake, r.nearest_k) == (33, 40, 5) and r.counts == tuple(int(v) for v in g["counts"])
    assert (r.precision, r.recall, r.density, r.coverage) == O.ratios(g["counts"], 33, 40, 5)
    assert r.fake_count.dtype == torch.int32 and r.real_min2.dtype == torch.float64 and r.radii2_real.is_cuda
    assert np.array_equal(r.fake_count.cpu().numpy(), g["fake_count"]) and np.array_equal(r.real_hit.cpu().numpy(), g["real_hit"])
    assert (np.abs(r.radii2_real.cpu().numpy() - g["radii2_real"]) <= g["bound_real"]).all()
    a, b = FeatureBank(48, DEV).append(x), FeatureBank(48, DEV).append(y)
    rb = manifold_metrics(a, b, nearest_k=5)
    assert rb.counts == r.counts and torch.equal(rb.radii2_fake, r.radii2_fake) and torch.equal(rb.real_min2, r.real_min2)
    wide = torch.full((33, 60), G.POISON, device=DEV)
    wide[:, :48] = x
    rs = manifold_metrics(wide[:, :48], b)                                       # strided rows, a tensor against a bank
    assert rs.counts == r.counts and torch.equal(rs.radii2_real, r.radii2_real)
    alone = knn_radii2(y, 5)
    assert alone.dtype == torch.float64 and tuple(alone.shape) == (40,) and torch.equal(alone, r.radii2_fake)
    assert torch.equal(knn_radii2(y, 5, col_chunks=3), alone)
    k3 = manifold_metrics(a, b, nearest_k=3)                                     # the precision / recall paper's k
    want = O.evaluate(g["x"], g["y"], 3)
    assert k3.counts == tuple(int(v) for v in want["counts"]) and k3.nearest_k == 3
    me = manifold_metrics(a, a)                                                  # real is fake
    assert me.precision == 1.0 and me.recall == 1.0 and me.coverage == 1.0 and me.density == 6.0 / 5.0
    with pytest.raises(ValueError):
        manifold_metrics(x, y[:, :47])
    with pytest.raises(ValueError):
        manifold_metrics(x, y.half())
    with pytest.raises(ValueError):
        manifold_metrics(x[:5], y)                                               # 5 rows at k = 5


def test_bank_radii_are_cached(hiplib, monkeypatch):
    """A second call launches no radius kernel for a bank that has not changed; append invalidates."""
    from rcdms_amd import prdc
    from rcdms_amd.kid import FeatureBank
    g = O.load("n17_23_d5_k3")
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    inner = prdc._radii2
    rec = _Recorder(lambda *a, **kw: types.SimpleNamespace(image_embeds=inner(*a, **kw)))     # keeps every radius vector computed
    monkeypatch.setattr(prdc, "_radii2", lambda *a, **kw: rec(*a, **kw).image_embeds)
    ref, gen = FeatureBank(5, DEV).append(x), FeatureBank(5, DEV).append(y)
    first = prdc.manifold_metrics(ref, gen, nearest_k=3)
    assert len(rec.embeds) == 2 and first.counts == tuple(int(v) for v in g["counts"])
    second = prdc.manifold_metrics(ref, gen, nearest_k=3)
    assert len(rec.embeds) == 2 and second.counts == first.counts                # no radius sweep at all
    assert ref.radii2(3) is first.radii2_real and len(rec.embeds) == 2
    ref.radii2(2)
    assert len(rec.embeds) == 3                                                  # kept per k
    gen.append(y[:4])
    third = prdc.manifold_metrics(ref, gen, nearest_k=3)
    assert len(rec.embeds) == 4 and third.n_fake == 27                           # only the changed bank is swept again
    want = O.evaluate(g["x"], np.concatenate([g["y"], g["y"][:4]]), 3)
    assert np.array_equal(third.fake_count.cpu().numpy(), want["fake_count"])
    gen.clear().append(y)
    assert prdc.manifold_metrics(ref, gen, nearest_k=3).counts == first.counts and len(rec.embeds) == 5
    prdc.manifold_metrics(ref, y, nearest_k=3)                                   # a tensor has no cache
    assert len(rec.embeds) == 6


def test_story_sized_case(hiplib):
    """300 rows of d = 1280 in float32 against the numpy model: the counts equal where every comparison has a margin above twice
    the a-priori bound (checked here, on the model's distances), the radii within the bound."""
    from rcdms_amd.prdc import manifold_metrics
    rng = np.random.RandomState(5)                      # an 8-dimensional latent cloud in 1280 features plus a little noise
    W = rng.standard_normal((8, 1280)) / np.sqrt(8.0)
    x = (rng.standard_normal((300, 8)) @ W + 0.05 * rng.standard_normal((300, 1280))).astype(np.float32)
    y = ((0.8 * rng.standard_normal((300, 8)) + 0.3) @ W + 0.05 * rng.standard_normal((300, 1280))).astype(np.float32)
    want = O.evaluate(x, y, 5)
    Bx, By, Bxy = O.radius_bound(x), O.radius_bound(y), O.bound(x, y)
    D = O.dist2(O.norms2(x), O.norms2(y), O.dots(x, y))
    safe = (np.abs(D - want["radii2_real"][:, None]) > 2 * np.maximum(Bxy, Bx[:, None])).all() and \
        (np.abs(D - want["radii2_fake"][None, :]) > 2 * np.maximum(Bxy, By[None, :])).all()
    assert safe, "the generator no longer gives a margin-safe case"
    r = manifold_metrics(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    assert r.counts == tuple(int(v) for v in want["counts"]) and 0 < r.counts[1] < 300 and 0 < r.counts[3] < 300
    assert np.array_equal(r.fake_count.cpu().numpy(), want["fake_count"]) and np.array_equal(r.real_hit.cpu().numpy(), want["real_hit"])
    assert (np.abs(r.radii2_real.cpu().numpy() - want["radii2_real"]) <= 2 * Bx).all()      # two evaluations inside the rules
    assert (np.abs(r.radii2_fake.cpu().numpy() - want["radii2_fake"]) <= 2 * By).all()
    assert (np.abs(r.real_min2.cpu().numpy() - want["real_min2"]) <= 2 * Bxy.max(axis=1)).all()
