"""GPU: rcdms_amd.frechet and the kernels under it (csrc/frechet.hip), in guarded buffers (tests/guard.py).

  statistics   integer-valued features and an integer shift: `sum` and `outer` equal the int64 sums bit for bit, in one update
               and split into updates of 1, 4 and the rest; the pad columns d..ld hold poison.  The TN product on doubles with
               A != B pins the lane maps of the float64 MFMA (a swapped row / column map passes a symmetric product).
  finalize     mean and covariance against the same operations in numpy float64; the covariance is symmetric bit for bit.
  distance     exact on diagonal covariances of perfect squares; within the budget of tests/frechet_oracle.py of the 60-digit
               goldens (tests/golden/frechet_*.npz) on d = 1 .. 48, rank-deficient sets, a set against itself, a mean offset,
               and merged halves.  The budget comes from the model's error against mpmath, never from the kernel.
  cache        a reference set is factored once; an update invalidates its factor.
  StoryRunner  feature_stats=(generated, reference) at the tiny widths of tests/test_story_metrics_gpu.py."""
import numpy as np
import pytest
import torch

from tests import frechet_oracle as O
from tests import guard as G
from tests.test_story_gpu import CAPS, DEV, S, chain, cuda_gen  # noqa: F401  (chain: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8), (3, 17, 24), (5, 16, 16), (37, 40, 48), (64, 96, 96)]     # (n, d, ld)
DTYPES = {"f32": torch.float32, "f16": torch.float16}


def integer_features(n, d, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(-8, 9, size=(n, d)), rng.randint(-3, 4, size=d)


def run_update(hip, x, k, ld, dtype, splits):
    """The entry point on guarded buffers.  -> (sum (d,), outer (d, d)) as numpy float64."""
    n, d = x.shape
    xv, xh = G.guarded_in(torch.from_numpy(x).to(dtype), ld, device=DEV)
    kv, kh = G.guarded_vec(torch.from_numpy(k).to(torch.float32), device=DEV)
    sv, sh = G.guarded_out(1, d, d + 3, torch.float64, device=DEV, guard_rows=4)
    ov, oh = G.guarded_out(d, d, d, torch.float64, device=DEV)
    sh.data.zero_()
    oh.data.zero_()
    code = hip.FSTATS_F16 if dtype == torch.float16 else hip.FSTATS_F32
    r = 0
    for m in splits:
        m = min(m, n - r)
        if m <= 0:
            break
        hip.feature_stats_update(hip.FStatsDesc(ld, m, d, code, 0), xv[r:].data_ptr(), kv.data_ptr(), sv.data_ptr(), ov.data_ptr())
        r += m
    assert r == n
    torch.cuda.synchronize()
    G.check_all(xh, kh, sh, oh)
    return sh.data[0].cpu().numpy(), oh.data.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("n,d,ld", SHAPES)
def test_statistics_exact(hiplib, n, d, ld, dtype):
    from rcdms_amd import hip
    x, k = integer_features(n, d, 100 * n + d)
    xc = x.astype(np.int64) - k
    want_sum, want_outer = xc.sum(axis=0).astype(np.float64), (xc.T @ xc).astype(np.float64)
    s1, o1 = run_update(hip, x, k, ld, DTYPES[dtype], [n])
    assert same_bits(s1, want_sum), (s1, want_sum)
    assert same_bits(o1, want_outer), np.argwhere(o1 != want_outer)[:4]
    s2, o2 = run_update(hip, x, k, ld, DTYPES[dtype], [1, 4, n])
    assert same_bits(s2, want_sum) and same_bits(o2, want_outer)


@pytest.mark.parametrize("k,m,n", [(1, 1, 1), (5, 17, 33), (37, 70, 40)])
def test_gemm_tn_f64_exact_with_asymmetric_operands(hiplib, k, m, n):
    from rcdms_amd import hip
    rng = np.random.RandomState(k + m)
    a, b = rng.randint(-9, 10, size=(k, m)).astype(np.float64), rng.randint(-9, 10, size=(k, n)).astype(np.float64)
    b[:, 0] += 100.0                                   # nothing about B is symmetric or shared with A
    av, ah = G.guarded_in(torch.from_numpy(a), m + 3, device=DEV, guard_rows=8)
    bv, bh = G.guarded_in(torch.from_numpy(b), n + 1, device=DEV, guard_rows=8)
    cv, ch = G.guarded_out(m, n, n + 5, torch.float64, device=DEV, guard_rows=64)
    hip.gemm_tn_f64(m, n, k, av.data_ptr(), m + 3, bv.data_ptr(), n + 1, cv.data_ptr(), n + 5)
    torch.cuda.synchronize()
    G.check_all(ah, bh, ch)
    G.check_written(ch)
    assert same_bits(ch.data.cpu().numpy(), a.T @ b)


@pytest.mark.parametrize("n,d,ld", SHAPES)
def test_finalize_against_numpy(hiplib, n, d, ld):
    from rcdms_amd.frechet import FeatureStats
    x, k = integer_features(n, d, 100 * n + d)
    buf = torch.full((n, ld), G.POISON, dtype=torch.float32, device=DEV)
    buf[:, :d] = torch.from_numpy(x).to(torch.float32)
    st = FeatureStats(d, DEV, shift=k.astype(np.float32)).update(buf[:, :d])          # strided rows, read where they lie
    xc = x.astype(np.int64) - k
    s, outer = xc.sum(axis=0).astype(np.float64), (xc.T @ xc).astype(np.float64)
    want_mean = k.astype(np.float64) + s / n
    mean = st.mean().cpu().numpy()
    assert st.n == n and (np.abs(mean - want_mean) <= 4.0 * O.EPS * np.abs(want_mean)).all()
    if n < 2:
        with pytest.raises(ValueError):
            st.cov()
        return
    want_cov = (outer - np.outer(s, s) / n) / (n - 1)
    cov = st.cov()
    assert torch.equal(cov.view(torch.int64), cov.T.contiguous().view(torch.int64)), "the covariance is not symmetric bit for bit"
    cov = cov.cpu().numpy()
    err = np.abs(cov - want_cov)
    print(f"finalize ({n}, {d}): worst relative error {np.max(err / np.maximum(np.abs(want_cov), 1e-300)):.2e}")
    assert (err <= 4.0 * O.EPS * np.abs(want_cov)).all()
    assert abs(float(st.trace().item()) - np.trace(want_cov)) <= 4.0 * O.EPS * d * np.abs(np.diag(want_cov)).sum()


@pytest.mark.parametrize("d", [8, 17])
def test_distance_exact_on_diagonal_perfect_squares(hiplib, d):
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    rng = np.random.RandomState(d)
    ra, rb = rng.randint(0, 9, size=d), rng.randint(0, 9, size=d)       # the roots; zeros included
    ra[1], rb[2], rb[d - 1] = 0, 0, 0
    ra[0], rb[0] = 8, 5
    mu_a, mu_b = rng.randint(-5, 6, size=d).astype(np.float64), rng.randint(-5, 6, size=d).astype(np.float64)
    a = FeatureStats.from_moments(mu_a, np.diag((ra * ra).astype(np.float64)), device=DEV)
    b = FeatureStats.from_moments(mu_b, np.diag((rb * rb).astype(np.float64)), device=DEV)
    r = frechet_distance(a, b)
    assert r.sweeps == (1, 1, 1)                                        # no pair rotates: one sweep finds that out
    assert (r.rank_a, r.rank_b) == (int((ra != 0).sum()), int((rb != 0).sum()))
    assert r.mean_term == float(((mu_a - mu_b) ** 2).sum()) and r.trace_a == float((ra * ra).sum()) and r.trace_b == float((rb * rb).sum())
    assert r.sqrt_trace == float((ra * rb).sum())
    assert r.distance == float(((mu_a - mu_b) ** 2).sum() + ((ra - rb) ** 2).sum())


def stats_of(x, dtype=torch.float32):
    from rcdms_amd.frechet import FeatureStats
    return FeatureStats(x.shape[1], DEV).update(torch.from_numpy(x).to(DEV, dtype))


@pytest.mark.parametrize("name", O.CASES)
def test_distance_against_the_goldens(hiplib, name):
    from rcdms_amd.frechet import frechet_distance
    g = O.load(name)
    d, s, want = g["xa"].shape[1], float(g["scale"]), float(g["mp_distance"])
    bound = O.budget(d, s, O.MODEL_ERROR[name])
    a, b = stats_of(g["xa"]), stats_of(g["xb"])
    r = frechet_distance(a, b)
    err = abs(r.distance - want)
    print(f"{name}: kernel {r.distance:.17g}, mpmath {want:.17g}, |diff| {err:.3e} = {err / (d * O.EPS * s):.2f} d eps s "
          f"(budget {bound / (d * O.EPS * s):.2f}), sweeps {r.sweeps}, ranks {r.rank_a}/{r.rank_b}")
    assert err <= bound
    assert [r.rank_a, r.rank_b] == g["model_ranks"].tolist()
    assert max(r.sweeps) <= O.MAX_SWEEPS
    if name == "self":
        # the same set twice, as two objects and as one: within the budget of 0, a tiny negative allowed and not clamped
        rs = frechet_distance(a, a)
        print(f"  one object against itself: {rs.distance:.3e}")
        assert abs(rs.distance) <= bound and rs.mean_term == 0.0
    if name == "merge":
        from rcdms_amd.frechet import FeatureStats
        xa = g["xa"]
        h = xa.shape[0] // 2
        first, second = stats_of(xa[:h]), stats_of(xa[h:])
        assert not torch.equal(first.shift, second.shift)              # the halves are centred differently: merge re-centres
        merged = first.merge(second)
        assert merged.n == a.n
        rm = frechet_distance(merged, b)
        print(f"  merged halves: {rm.distance:.17g}, |diff| {abs(rm.distance - want):.3e}")
        assert abs(rm.distance - want) <= bound
        scale = float(a.cov().abs().max())
        assert float((merged.cov() - a.cov()).abs().max()) <= 16.0 * O.EPS * scale * xa.shape[0]
        # the statistics survive the .npz round trip (pytorch-fid's keys)
        import os
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            a.save(os.path.join(tmp, "a.npz"))
            with np.load(os.path.join(tmp, "a.npz")) as z:
                assert sorted(z.files) == ["mu", "n", "sigma"]
            back = FeatureStats.load(os.path.join(tmp, "a.npz"), DEV)
        assert back.n == a.n and torch.equal(back.cov(), a.cov()) and torch.equal(back.mean(), a.mean())
        assert frechet_distance(back, b).distance == r.distance


def test_half_precision_features_and_leading_axes(hiplib):
    from rcdms_amd.frechet import FeatureStats
    g = O.load("d31_odd")
    x16 = torch.from_numpy(g["xa"]).to(DEV, torch.float16)
    a = FeatureStats(31, DEV).update(x16.reshape(4, 10, 31))
    mean, cov, _ = O.moments(x16.cpu().numpy(), a.shift.cpu().numpy())
    assert a.n == 40
    assert float((a.mean().cpu() - torch.from_numpy(mean)).abs().max()) <= 4.0 * O.EPS * np.abs(mean).max()
    assert float((a.cov().cpu() - torch.from_numpy(cov)).abs().max()) <= 40 * O.EPS * np.abs(cov).max()
    with pytest.raises(ValueError):
        a.update(torch.zeros(3, 30, device=DEV))
    with pytest.raises(ValueError):
        a.update(torch.zeros(3, 31, device=DEV, dtype=torch.float64))


def test_factor_cache(hiplib):
    from rcdms_amd.frechet import frechet_distance
    g = O.load("n_lt_d_one")
    a, ref = stats_of(g["xa"]), stats_of(g["xb"])
    first = frechet_distance(a, ref)
    assert min(first.sweeps) >= 1
    a2 = stats_of(g["xa"][:8])
    second = frechet_distance(a2, ref)
    assert second.sweeps[1] == 0 and second.sweeps[0] >= 1 and second.rank_b == first.rank_b      # the reference was factored once
    again = frechet_distance(a, ref)
    assert again.sweeps[:2] == (0, 0) and again.distance == first.distance
    ref.update(torch.from_numpy(g["xa"][:3]).to(DEV))
    third = frechet_distance(a, ref)
    assert third.sweeps[1] >= 1 and third.sweeps[0] == 0 and third.distance != first.distance   # the update dropped the factor


# ------------------------------------------------------------------------------------------------ StoryRunner
def call(b, **kw):
    args = dict(num_inference_steps=3, prior_steps=3, guidance_scale=2.0, prior_guidance_scale=4.0, output_type="uint8",
                generator=[cuda_gen(s) for s in (51, 52, 53)], prior_generator=[cuda_gen(s) for s in (41, 42, 43)])
    args.update(kw)
    return b.runner(b.frames, CAPS, **args)


class _Recorder:
    """Stands in for the runner's vision tower and keeps the `image_embeds` of every forward it is asked for."""

    def __init__(self, inner):
        self.inner, self.embeds = inner, []

    def __call__(self, *args, **kw):
        out = self.inner(*args, **kw)
        self.embeds.append(out.image_embeds)
        return out

    def __getattr__(self, name):
        return getattr(self.inner, name)


def test_story_runner_feature_stats(chain):
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    b = chain
    gen, ref = FeatureStats(b.E, DEV), FeatureStats(b.E, DEV)
    rec = _Recorder(b.runner.image_encoder)
    b.runner.image_encoder = rec
    try:
        res = call(b, metrics=("clip_i",), feature_stats=(gen, ref))
    finally:
        b.runner.image_encoder = rec.inner
    off = call(b, metrics=("clip_i",))
    assert gen.n == 5 * S and ref.n == 5 * S
    assert torch.equal(res.videos, off.videos) and torch.equal(res.clip_i, off.clip_i) and torch.equal(res.target_embeds, off.target_embeds)
    # the rows the runner handed to `generated`: the last forward of the call, the one clip_i is the cosine of (done once)
    fed = rec.embeds[-1]
    assert tuple(fed.shape) == (S * 5, b.E) and torch.equal(rec.embeds[0].reshape(S, 5, -1), res.target_embeds)
    cos = torch.nn.functional.cosine_similarity(fed.reshape(S, 5, -1).float(), res.target_embeds.float(), dim=-1)
    assert torch.equal(cos, res.clip_i), "clip_i and feature_stats did not share one forward"
    assert sum(1 for e in rec.embeds if e.shape[0] == S * 5) == 2            # the targets and the generated frames, no third forward
    # means of exactly those rows, at the finalize budget (4 eps relative per element) plus the order of the sums: the kernel
    # adds the n terms x - k (|x - k| <= 2 max|x|) one after the other, error <= (n - 1) eps max|x| after the division by n, and
    # the float64 mean it is compared with may round as much again
    for st, rows in ((gen, fed.reshape(S * 5, -1).double()), (ref, res.target_embeds.reshape(S * 5, -1).double())):
        want = rows.mean(dim=0)
        tol = 4.0 * O.EPS * want.abs() + 2.0 * rows.shape[0] * O.EPS * rows.abs().max()
        diff = (st.mean() - want).abs()
        print(f"story statistics: worst |mean - mean of the rows fed| {float(diff.max()):.2e}, allowed {float(tol.min()):.2e}")
        assert bool((diff <= tol).all()), float(diff.max())
    # plumbing, loosely: a separate forward of the test's own gives the same rows up to the last-bit differences of f16 rows
    # between two runs that tests/test_story_metrics_gpu.py allows (2^-10 relative on single elements)
    px = b.runner.clip_processor(images=res.videos.reshape(S * 5, *res.videos.shape[2:])).pixel_values
    e = b.vision(px).image_embeds.reshape(S * 5, -1).double()
    assert float((gen.mean() - e.mean(dim=0)).abs().max()) <= 2.0 ** -10 * float(e.abs().max())
    r = frechet_distance(gen, ref)
    print(f"story CLIP-FD over {gen.n} frames at E = {b.E}: {r.distance:.6g}, ranks {r.rank_a}/{r.rank_b}, sweeps {r.sweeps}")
    assert np.isfinite(r.distance) and r.rank_a <= 5 * S - 1 and r.rank_b <= 5 * S - 1
    only = call(b, feature_stats=(gen, ref))
    assert only.clip_i is None and gen.n == 10 * S
    with pytest.raises(ValueError, match="uint8"):
        call(b, feature_stats=(gen, ref), output_type="tensor")
    with pytest.raises(ValueError, match="stage 2"):
        call(b, feature_stats=(gen, ref), stage2=False)
