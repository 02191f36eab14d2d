"""GPU: rcdm_cholesky_pivoted_f64 and the factor="cholesky" route of rcdms_amd.frechet, in guarded buffers (tests/guard.py).

  exact       integer factors L0 (tests/frechet_chol_oracle.py): from L0 L0^T the kernel returns L0 bit for bit, full and with the
              first d // 2 columns kept, at d = 1, 2, 17, 33, 70 and at nb, nb + 1, 2 nb for the panel width nb = 16 (the
              rank-deficient form stops inside a panel at d = 17 and 70, and exactly at a panel's edge at d = 32 and 33); the
              identity and the zero matrix.  The input sits in poison and is bit-identical afterwards, the output was NaN and its pad columns still are, the workspace
              was all-ones bytes and nothing past its stated size is touched.
  residual    |F F^T - S|_max <= 4 d 2^-52 max diag on every golden covariance: backward-stable Cholesky's bound.  The numpy
              model's residual on the same inputs is at most 0.10 d 2^-52 max diag.
  distance    within the budget of tests/frechet_oracle.py of the 60-digit goldens, the nine older and the three new cases, with
              the Cholesky model's own error table (measured against mpmath, never against the kernel); the model's ranks; the
              two routes against each other within the sum of their budgets.
  block       the singular-value run sees the rank_b (rounded up to even) x rank_a block only.
  cache       one factor per method; an update drops both.
  default     frechet_distance(a, b) is bit for bit what it was, whatever the other route has cached."""
import numpy as np
import pytest
import torch

from tests import frechet_chol_oracle as C
from tests import frechet_oracle as O
from tests import guard as G
from tests.test_story_gpu import DEV

pytestmark = pytest.mark.gpu

NB = C.NB
CANARY = 256            # bytes after the workspace the entry was told about


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def factor_on_device(sigma, ld=None, ldf=None, nb=0):
    """The entry point on guarded buffers.  -> (F (d, d) numpy, rank)."""
    from rcdms_amd import hip
    d = sigma.shape[0]
    ld, ldf = d + 3 if ld is None else ld, d + 5 if ldf is None else ldf
    av, ah = G.guarded_in(torch.from_numpy(np.ascontiguousarray(sigma, np.float64)), ld, device=DEV, guard_rows=8)
    fv, fh = G.guarded_out(d, d, ldf, torch.float64, device=DEV, guard_rows=8)
    desc = hip.CholeskyDesc(ld, ldf, d, nb)
    need = hip.cholesky_workspace_bytes(desc)
    assert need > 0
    ws = torch.full((need + CANARY,), 0xFF, dtype=torch.uint8, device=DEV)       # NaN doubles, -1 integers
    rank = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    hip.cholesky_pivoted_f64(desc, av.data_ptr(), fv.data_ptr(), rank[1:].data_ptr(), ws.data_ptr(), need)
    torch.cuda.synchronize()
    G.check_all(ah, fh)
    G.check_written(fh)
    assert bool((ws[need:] == 0xFF).all()), "wrote past the workspace"
    assert rank.tolist()[::2] == [-7, -7]
    return fh.data.cpu().numpy(), int(rank[1])


@pytest.mark.parametrize("d", sorted({1, 2, 17, 33, 70, NB, NB + 1, 2 * NB}))
def test_exact_answers(hiplib, d):
    for name, sigma, want, want_rank in C.exact_cases(d):
        F, rank = factor_on_device(sigma)
        assert rank == want_rank, (name, rank, want_rank)
        assert same_bits(F, want), (name, np.argwhere(F != want)[:4])


@pytest.mark.parametrize("nb", [nb for nb in C.PANELS if nb != NB])
def test_exact_answers_at_the_other_panel_widths(hiplib, nb):
    for d in (nb - 1, nb + 1, 2 * nb):
        for name, sigma, want, want_rank in C.exact_cases(d):
            F, rank = factor_on_device(sigma, nb=nb)
            assert rank == want_rank and same_bits(F, want), (d, name, rank)


def test_hostile_diagonals_and_ties(hiplib):
    F, rank = factor_on_device(np.diag([4.0, -1.0, np.nan, 9.0, 0.0]))
    assert rank == 2 and same_bits(F, C.pivoted_cholesky(np.diag([4.0, -1.0, np.nan, 9.0, 0.0]))[0])
    assert factor_on_device(-np.eye(3))[1] == 0
    cut = 2 * O.EPS
    assert factor_on_device(np.diag([1.0, cut]))[1] == 1 and factor_on_device(np.diag([1.0, np.nextafter(cut, 1.0)]))[1] == 2
    # d <= nb: no trailing update, every operation is the model's own, and the tie-break decides the column order
    sigma = C.tie_covariance()
    F, rank = factor_on_device(sigma, ld=15, ldf=15)
    want, want_rank, _ = C.pivoted_cholesky(sigma)
    assert rank == want_rank == 15 and same_bits(F, want)


@pytest.mark.parametrize("name", C.CASES)
def test_factor_residual(hiplib, name):
    g = C.load(name)
    for key in ("cov_a", "cov_b"):
        sigma = g[key]
        d = sigma.shape[0]
        unit = d * O.EPS * np.diag(sigma).max()
        for nb in (0, 32):
            F, rank = factor_on_device(sigma, nb=nb)
            model, model_rank, _ = C.pivoted_cholesky(sigma, nb or NB)
            res, mres = np.abs(F @ F.T - sigma).max(), np.abs(model @ model.T - sigma).max()
            print(f"{name} {key} nb {nb or NB}: rank {rank}, residual {res / unit:.3f} d eps max diag (model {mres / unit:.3f}), "
                  f"same bits as the model: {same_bits(F, model)}")
            assert rank == model_rank and not F[:, rank:].any()
            assert res <= 4.0 * unit
    again = factor_on_device(sigma, nb=32)[0]
    assert same_bits(again, F), "the same input gave other bits"


def stats_of(x):
    from rcdms_amd.frechet import FeatureStats
    return FeatureStats(x.shape[1], DEV).update(torch.from_numpy(x).to(DEV))


@pytest.fixture(scope="module")
def results(hiplib):
    """case -> (golden, the Cholesky route's result, the default route's result), each computed once on fresh objects."""
    from rcdms_amd.frechet import frechet_distance
    out = {}
    for name in C.CASES:
        g = C.load(name)
        chol = frechet_distance(stats_of(g["xa"]), stats_of(g["xb"]), factor="cholesky")
        jac = frechet_distance(stats_of(g["xa"]), stats_of(g["xb"])) if name in O.CASES else None
        out[name] = (g, chol, jac)
    return out


@pytest.mark.parametrize("name", C.CASES)
def test_distance_against_the_goldens(results, name):
    g, r, _ = results[name]
    d, s, want = g["xa"].shape[1], float(g["scale"]), float(g["mp_distance"])
    bound = O.budget(d, s, C.MODEL_ERROR[name])
    model = C.distance_from_moments(g["mu_a"], g["cov_a"], g["mu_b"], g["cov_b"])
    err = abs(r.distance - want)
    print(f"{name}: kernel {r.distance:.17g}, mpmath {want:.17g}, |diff| {err:.3e} = {err / (d * O.EPS * s):.2f} d eps s "
          f"(budget {bound / (d * O.EPS * s):.2f}), sweeps {r.sweeps}, ranks {r.rank_a}/{r.rank_b}, block {r.block}")
    assert err <= bound
    assert [r.rank_a, r.rank_b] == [model["rank_a"], model["rank_b"]] == g["model_ranks"].tolist()
    assert r.sweeps[:2] == (0, 0) and 1 <= r.sweeps[2] <= O.MAX_SWEEPS
    assert r.block == model["block"]
    if name == "n_lt_d_both":
        assert r.block == (12, 9)                    # ranks 9 and 11: twelve vectors of length nine, not 24 of 24


@pytest.mark.parametrize("name", O.CASES)
def test_the_two_routes_agree(results, name):
    g, chol, jac = results[name]
    d, s = g["xa"].shape[1], float(g["scale"])
    diff = abs(chol.distance - jac.distance)
    print(f"{name}: |Cholesky route - Jacobi route| {diff:.3e} = {diff / (d * O.EPS * s):.2f} d eps s")
    assert diff <= O.budget(d, s, C.MODEL_ERROR[name]) + O.budget(d, s, O.MODEL_ERROR[name])
    assert (chol.rank_a, chol.rank_b) == (jac.rank_a, jac.rank_b)
    assert (chol.mean_term, chol.trace_a, chol.trace_b) == (jac.mean_term, jac.trace_a, jac.trace_b)
    assert jac.block == (d + (d & 1),) * 2 and min(jac.sweeps) >= 1


def test_rank_zero(hiplib):
    from rcdms_amd.frechet import frechet_distance
    g = C.load("tie")
    const = np.tile(np.linspace(-1.0, 1.0, 15, dtype=np.float32), (7, 1))          # seven identical rows: a zero covariance
    a, b = stats_of(const), stats_of(g["xb"])
    for r in (frechet_distance(a, b, factor="cholesky"), frechet_distance(b, a, factor="cholesky")):
        assert min(r.rank_a, r.rank_b) == 0 and max(r.rank_a, r.rank_b) == 15
        assert r.sqrt_trace == 0.0 and r.sweeps == (0, 0, 0) and r.block is None
        assert r.distance == (r.mean_term + r.trace_a) + r.trace_b and r.trace_a + r.trace_b == float(b.trace().item())
        assert r.mean_term > 0.0


def test_exact_on_diagonal_perfect_squares_both_routes(hiplib):
    """The expectations of tests/test_hip_frechet.py for the default call, unchanged, and the same exact values from the other
    route on the same two objects: neither route's cache leaks into the other."""
    from rcdms_amd.frechet import FeatureStats, frechet_distance
    d = 17
    rng = np.random.RandomState(d)
    ra, rb = rng.randint(0, 9, size=d), rng.randint(0, 9, size=d)
    ra[1], rb[2], rb[d - 1] = 0, 0, 0
    ra[0], rb[0] = 8, 5
    mu_a, mu_b = rng.randint(-5, 6, size=d).astype(np.float64), rng.randint(-5, 6, size=d).astype(np.float64)
    a = FeatureStats.from_moments(mu_a, np.diag((ra * ra).astype(np.float64)), device=DEV)
    b = FeatureStats.from_moments(mu_b, np.diag((rb * rb).astype(np.float64)), device=DEV)
    first = frechet_distance(a, b)
    chol = frechet_distance(a, b, factor="cholesky")
    again = frechet_distance(a, b)
    assert first.sweeps == (1, 1, 1) and again.sweeps == (0, 0, 1)
    ranks = (int((ra != 0).sum()), int((rb != 0).sum()))
    for r in (first, chol, again):
        assert (r.rank_a, r.rank_b) == ranks
        assert r.mean_term == float(((mu_a - mu_b) ** 2).sum()) and r.trace_a == float((ra * ra).sum()) and r.trace_b == float((rb * rb).sum())
        assert r.sqrt_trace == float((ra * rb).sum())
        assert r.distance == float(((mu_a - mu_b) ** 2).sum() + ((ra - rb) ** 2).sum())
    assert chol.sweeps == (0, 0, 1) and chol.block == (ranks[1] + (ranks[1] & 1), ranks[0])


def test_factor_cache_is_per_method(hiplib):
    from rcdms_amd.frechet import frechet_distance
    g = O.load("n_lt_d_one")
    a, ref = stats_of(g["xa"]), stats_of(g["xb"])
    default = frechet_distance(a, ref)
    fa, rank_a, _ = a.factor("cholesky")
    assert a.factor("cholesky")[0] is fa and ref._factor_chol is None              # kept; the other object is untouched
    assert a.factor()[0] is not fa and a.factor("jacobi")[0] is a.factor()[0] and a.factor()[2] == 0
    assert float(fa[:, rank_a:].abs().max()) == 0.0 and not torch.equal(fa, a.factor()[0])      # P L, not the eigen columns
    first = frechet_distance(a, ref, factor="cholesky")
    fb = ref._factor_chol[0]
    second = frechet_distance(a, ref, factor="cholesky")
    assert ref._factor_chol[0] is fb and a._factor_chol[0] is fa and second == first                       # both reused
    # the default route is bit for bit what it was before the other one ran, from its own cache and from scratch
    cached = frechet_distance(a, ref)
    fresh = frechet_distance(stats_of(g["xa"]), stats_of(g["xb"]))
    assert cached.sweeps[:2] == (0, 0) and cached.distance == default.distance and cached.sqrt_trace == default.sqrt_trace
    assert fresh == default
    ref.update(torch.from_numpy(g["xa"][:3]).to(DEV))
    assert ref._factor is None and ref._factor_chol is None
    third = frechet_distance(a, ref, factor="cholesky")
    assert third.distance != first.distance and a._factor_chol[0] is fa and ref._factor_chol[0] is not fb
    merged = stats_of(g["xa"][:5])
    merged.factor("cholesky")
    merged.merge(stats_of(g["xa"][5:]))
    assert merged._factor_chol is None and merged._factor is None
