"""CPU: the denoising objective before a GPU runs it.  DDPMScheduler's tables against the closed form and its add_noise against
the written-out expression; the numpy model of tests/objective_oracle.py against exact rationals within the a-priori bound;
the shared core csrc/objective_core.h compiled into tools/objective_host.cpp, which must give the model's bits on every case;
that the shared inputs tell the plausible mistakes apart; and the argument checks of the new entry points, which need no
device."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import objective_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcdm_diffuse_assemble", "rcdm_eps_sqerr_workspace_bytes", "rcdm_eps_sqerr")
SCHEDULES = {
    "linear": dict(beta_start=0.0001, beta_end=0.02, beta_schedule="linear"),
    "scaled_linear": dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"),
    "trained_betas": dict(trained_betas=[0.01 * (1 + (i % 7)) for i in range(50)], num_train_timesteps=50),
}


def default_table():
    from rcdms_amd.scheduler import DDPMScheduler
    return DDPMScheduler(**SCHEDULES["scaled_linear"]).noise_table().numpy()


# ------------------------------------------------------------------------------------------------ the scheduler
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_scheduler_tables_against_closed_form(name):
    from rcdms_amd.scheduler import DDPMScheduler
    kw = SCHEDULES[name]
    s = DDPMScheduler(**kw)
    T = s.config.num_train_timesteps
    ac, tab = s.alphas_cumprod, s.noise_table()
    assert ac.dtype == torch.float32 and ac.shape == (T,) and tab.dtype == torch.float32 and tab.shape == (T, 2)
    # the closed form in float64: beta_i exactly on its line, the running product of 1 - beta_i
    if name == "trained_betas":
        betas = np.asarray(kw["trained_betas"], np.float64)
    elif name == "linear":
        betas = np.linspace(kw["beta_start"], kw["beta_end"], T)
    else:
        betas = np.linspace(kw["beta_start"] ** 0.5, kw["beta_end"] ** 0.5, T) ** 2
    want = np.cumprod(1.0 - betas)
    # float32: beta_i, 1 - beta_i and the product each round once per step (beta_i's own few roundings are scaled by beta_i)
    rel = 3 * np.arange(1, T + 1) * 2.0 ** -24
    got = ac.double().numpy()
    assert np.all(np.abs(got - want) <= rel * want)
    # the table IS the two written-out expressions of the scheduler's own alphas_cumprod ...
    assert torch.equal(tab[:, 0], ac ** 0.5) and torch.equal(tab[:, 1], (1 - ac) ** 0.5)
    # ... each a correctly rounded square root, up to one float32 unit
    assert np.all(np.abs(tab[:, 0].double().numpy() - np.sqrt(got)) <= 2.0 ** -23 * np.sqrt(got))
    one_minus = (1 - ac).double().numpy()
    assert np.all(np.abs(tab[:, 1].double().numpy() - np.sqrt(one_minus)) <= 2.0 ** -23 * np.sqrt(one_minus))
    try:
        import diffusers
    except ImportError:
        diffusers = None
    if diffusers is not None:
        ref = diffusers.DDPMScheduler(**kw)
        assert torch.equal(ref.alphas_cumprod, ac)


def test_scheduler_refuses_other_schedules_and_keeps_config():
    from rcdms_amd.scheduler import DDPMScheduler
    with pytest.raises(NotImplementedError):
        DDPMScheduler(beta_schedule="squaredcos_cap_v2")
    s = DDPMScheduler()
    assert s.config.num_train_timesteps == 1000 and s.config.beta_schedule == "linear" and s.config.beta_end == 0.02
    assert s.noise_table("cpu") is s.noise_table("cpu")


def test_add_noise_is_the_written_out_expression():
    from rcdms_amd.scheduler import DDPMScheduler
    s = DDPMScheduler(**SCHEDULES["scaled_linear"])
    g = O.case(3, 5, 3, 5, s.noise_table().numpy())
    x0, noise, t = torch.tensor(g["x0"]), torch.tensor(g["noise"]), torch.tensor(g["t"])
    got = s.add_noise(x0, noise, t)
    ac = s.alphas_cumprod
    for b in range(3):
        want = ac[t[b]] ** 0.5 * x0[b] + (1 - ac[t[b]]) ** 0.5 * noise[b]
        assert torch.equal(got[b].view(torch.int32), want.view(torch.int32))
    model = O.noised(g["x0"], g["noise"], g["t"], s.noise_table().numpy())
    assert np.array_equal(got.numpy().view(np.int32), model.view(np.int32))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("B,F,H,W", O.GEOMETRIES)
def test_model_sums_within_the_bound_of_the_rationals(B, F, H, W):
    g = O.case(B, F, H, W, default_table())
    for offs in (None, g["offs"]):
        got = O.sqerr(g["eps"], g["noise"], offs, O.OFFS_SCALE)
        exact = O.sqerr_exact(g["eps"], g["noise"], offs, O.OFFS_SCALE)
        for b in range(B):
            for f in range(F):
                err = abs(O.Fraction(float(got[b, f])) - exact[b][f])
                assert err <= O.Fraction(O.bound(exact[b][f], H * W)), (b, f, float(err), O.bound(exact[b][f], H * W))
    assert O.addition_chain(256) == 11 and O.addition_chain(272) == 12 and O.addition_chain(1) == 11


def test_model_sums_on_small_integers_are_exact():
    B, F, H, W = 3, 5, 17, 16
    rng = np.random.default_rng(5)
    noise = rng.integers(-3, 4, (B, 4, F, H, W)).astype(np.float32)
    offs = rng.integers(-1, 2, (B, 4, F)).astype(np.float32)
    eps = O.eps_rows(B, F, H, W, 5, integers=True)
    got = O.sqerr(eps, noise, offs, 2.0)
    e = eps.view(np.float16).astype(np.int64)[:, :4].reshape(B, F, H * W, 4)
    n = np.moveaxis(noise.astype(np.int64) + 2 * offs.astype(np.int64)[:, :, :, None, None], 1, -1).reshape(B, F, H * W, 4)
    want = ((e - n) ** 2).sum(axis=(2, 3))
    assert O.same_bits(got, want.astype(np.float64)) and want.max() > 1000


def test_inputs_tell_the_mistakes_apart():
    """Without this the GPU test could not tell a contracted kernel, a dropped offset, a fifth channel or a shifted frame from
    the right one."""
    table = default_table()
    for B, F, H, W in O.GEOMETRIES:
        g = O.case(B, F, H, W, table)
        for offs in (None, g["offs"]):
            three = O.rows(g["x0"], g["noise"], offs, O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], 16)
            fused = O.rows(g["x0"], g["noise"], offs, O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], 16, form="fma")
            per_story = (three != fused).reshape(B, -1).sum(axis=1)
            assert np.all(per_story >= 1), (B, F, H, W, offs is None, per_story)
            assert np.array_equal(three[:, 4:], fused[:, 4:])
        right = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE)
        for variant in ("no_offs", "chan4") + (("neighbour",) if F > 1 else ()):
            wrong = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE, variant=variant)
            assert np.all(wrong.view(np.int64) != right.view(np.int64)), (B, F, H, W, variant)


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/objective_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("objective") / "objective_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "objective_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


def _dump(tmp_path, **arrays):
    paths = {}
    for name, a in arrays.items():
        paths[name] = str(tmp_path / f"{name}.raw")
        np.ascontiguousarray(a).tofile(paths[name])
    return paths


def run_rows(host_tool, tmp_path, g, t, table, offs, ld, c_pad):
    B, _, F, H, W = g["x0"].shape
    p = _dump(tmp_path, x0=g["x0"], noise=g["noise"], t=np.asarray(t, np.int64), table=table, mask=g["mask"], masked=g["masked"])
    args = [p[k] for k in ("x0", "noise", "t", "table", "mask", "masked")]
    if offs is not None:
        args.append(_dump(tmp_path, offs=offs)["offs"])
    r = subprocess.run([host_tool, "rows", *map(str, (B, F, H, W, ld, c_pad, table.shape[0])), repr(float(np.float32(O.OFFS_SCALE))), *args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([int(v, 16) for v in r.stdout.split()], np.uint16).reshape(-1, ld)


def run_sqerr(host_tool, tmp_path, eps, noise, offs, scale, ld):
    B, _, F, H, W = noise.shape
    padded = np.full((eps.shape[0], ld), 0x7533, np.uint16)             # 3.0e4-ish in the columns nobody may read
    padded[:, :eps.shape[1]] = eps
    p = _dump(tmp_path, eps=padded, noise=noise)
    args = [p["eps"], p["noise"]] + ([_dump(tmp_path, offs=offs)["offs"]] if offs is not None else [])
    r = subprocess.run([host_tool, "sqerr", *map(str, (B, F, H, W, ld)), repr(float(np.float32(scale))), *args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return np.array([int(v, 16) for v in r.stdout.split()], np.uint64).view(np.float64).reshape(B, F)


@pytest.mark.parametrize("k", range(len(O.GEOMETRIES)))
def test_host_tool_has_the_models_bits(host_tool, tmp_path, k):
    B, F, H, W = O.GEOMETRIES[k]
    ld, c_pad = O.ROW_SHAPES[k % 3]
    table = default_table()
    g = O.case(B, F, H, W, table)
    for offs in (None, g["offs"]):
        got = run_rows(host_tool, tmp_path, g, g["t"], table, offs, ld, c_pad)
        want = O.rows(g["x0"], g["noise"], offs, O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], c_pad)
        assert np.array_equal(got[:, :c_pad], want) and np.all(got[:, c_pad:] == 0xFFFF)
        assert np.all(got[:, 9:c_pad] == 0)
        sums = run_sqerr(host_tool, tmp_path, g["eps"][:, :4], g["noise"], offs, O.OFFS_SCALE, [4, 8, 24][k % 3])
        assert O.same_bits(sums, O.sqerr(g["eps"], g["noise"], offs, O.OFFS_SCALE))


def test_host_tool_out_of_range_timesteps_and_nan(host_tool, tmp_path):
    B, F, H, W = 3, 5, 3, 5
    table = default_table()
    g = O.case(B, F, H, W, table)
    base = O.rows(g["x0"], g["noise"], g["offs"], O.OFFS_SCALE, g["t"], table, g["mask"], g["masked"], 16)
    per = F * H * W
    for bad in (-1, table.shape[0]):
        t = g["t"].copy()
        t[1] = bad
        got = run_rows(host_tool, tmp_path, g, t, table, g["offs"], 24, 16)
        assert np.array_equal(got[:, :16], O.rows(g["x0"], g["noise"], g["offs"], O.OFFS_SCALE, t, table, g["mask"], g["masked"], 16))
        assert np.all(got[per:2 * per, :4] == O.F16_NAN) and np.array_equal(got[per:2 * per, 4:16], base[per:2 * per, 4:])
        assert np.array_equal(got[:per, :16], base[:per]) and np.array_equal(got[2 * per:, :16], base[2 * per:])
    eps = g["eps"].copy()
    row = (1 * F + 3) * H * W + 7                                       # story 1, frame 3
    eps[row, 2] = O.F16_NAN
    sums = run_sqerr(host_tool, tmp_path, eps[:, :4], g["noise"], g["offs"], O.OFFS_SCALE, 8)
    nan = np.isnan(sums)
    assert nan[1, 3] and nan.sum() == 1
    clean = O.sqerr(g["eps"], g["noise"], g["offs"], O.OFFS_SCALE)
    assert np.array_equal(sums.view(np.int64)[~nan], clean.view(np.int64)[~nan])


def test_host_tool_refusals(host_tool, tmp_path):
    p = str(tmp_path / "x.raw")
    np.zeros(3, np.float32).tofile(p)
    run = lambda *a: subprocess.run([host_tool, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run("rows", "1", "1", "1", "1", "20", "16", "10", "0", p, p, p, p, p, p).returncode == 2       # ld no multiple of 8
    assert run("rows", "1", "1", "1", "1", "16", "8", "10", "0", p, p, p, p, p, p).returncode == 2        # c_pad below 16
    assert run("rows", "1", "1", "1", "1", "16", "16", "10", "0", p, p, p, p, p, p).returncode == 2       # files of the wrong size
    assert run("sqerr", "1", "1", "1", "1", "6", "0", p, p).returncode == 2                               # ld no multiple of 4
    assert run("sqerr", "0", "1", "1", "1", "4", "0", p, p).returncode == 2
    r = run("nothing")
    assert r.returncode == 2 and b"usage" in r.stderr


# ------------------------------------------------------------------------------------------------ the Python layer
def _result(t, seen, sq, per=64):
    from rcdms_amd.objective import ObjectiveResult
    return ObjectiveResult(sq_err=torch.tensor(np.array(sq), dtype=torch.float64), loss=None, per_story=None,
                           timesteps=torch.tensor(t), seen=torch.tensor(np.array(seen)), loss_seen=None, loss_unseen=None,
                           frame_elements=per)


def test_loss_log_folds_in_row_order(tmp_path):
    from rcdms_amd.objective import LossLog
    rng = np.random.default_rng(3)
    t = [0, 99, 100, 999, 450, 1000, -1]
    seen = rng.random((7, 5)) < 0.4
    seen[0], seen[1] = True, False
    sq = rng.random((7, 5)) * 100
    whole = LossLog("cpu").append(_result(t, seen, sq))
    parts = LossLog("cpu")
    for lo, hi in ((0, 2), (2, 3), (3, 7)):
        parts.append(_result(t[lo:hi], seen[lo:hi], sq[lo:hi]))
    a, b = whole.result(bins=10), parts.result(bins=10)
    for k in ("edges", "stories", "loss", "loss_seen", "loss_unseen"):
        assert np.array_equal(getattr(a, k).view(np.int64), getattr(b, k).view(np.int64)), k
    assert a.stories.tolist() == [2, 1, 0, 0, 1, 0, 0, 0, 0, 1]                  # 1000 and -1 fall outside every bin
    want = (sq[0].sum() + sq[1].sum()) / (10 * 64)
    assert abs(a.loss[0] - want) <= 16 * O.U * want                             # nine additions in either order
    assert abs(a.loss_seen[0] - sq[0].sum() / (5 * 64)) <= 8 * O.U * a.loss_seen[0]
    assert abs(a.loss_unseen[0] - sq[1].sum() / (5 * 64)) <= 8 * O.U * a.loss_unseen[0]
    assert np.isnan(a.loss[2]) and np.isnan(a.loss_seen[2])
    assert whole.result(bins=3).edges.tolist() == [0, 334, 667, 1000] and whole.result(bins=3).stories.tolist() == [3, 1, 1]
    whole.save(tmp_path / "log.npz")
    back = LossLog.load(tmp_path / "log.npz", "cpu")
    assert len(back) == 7 and np.array_equal(back.result(bins=10).loss.view(np.int64), a.loss.view(np.int64))
    with pytest.raises(ValueError):
        whole.append(_result([1], [[True] * 4], [[1.0] * 4]))
    with pytest.raises(ValueError):
        LossLog("cpu").result()
    for k in range(70):                                                          # past the first capacity: the buffer grows
        parts.append(_result([k], [seen[0]], [sq[0]]))
    assert len(parts) == 77 and parts.result(bins=10).stories.sum() == 75


def test_frame_labels_and_refusals():
    from rcdms_amd.objective import DenoisingObjective, frame_labels
    mask = torch.zeros(2, 1, 5, 3, 3)
    mask[0, 0, :2] = 1
    mask[1, 0, 4] = 1
    assert frame_labels(mask).tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 0, 1]]
    mask[1, 0, 2, 1, 1] = 1
    with pytest.raises(ValueError, match="please check mask label"):
        frame_labels(mask)
    mask[1, 0, 2] = 0.5
    with pytest.raises(ValueError, match="please check mask label"):
        frame_labels(mask)
    with pytest.raises(ValueError):
        DenoisingObjective(None, noise_offset=-1.0)
    with pytest.raises(TypeError):
        DenoisingObjective(None, scheduler=object())
    obj = DenoisingObjective(None)
    assert obj.scheduler.config.beta_schedule == "scaled_linear" and obj.scheduler.config.beta_start == 0.00085


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
    assert lib.rcdm_version() == 0x000300
    from rcdms_amd import build
    assert "objective.hip" in build.SOURCES
    ws = lib.rcdm_eps_sqerr_workspace_bytes
    assert ws(3, 5, 17, 16) == 3 * 5 * 2 * 8 and ws(1, 1, 1, 1) == 8 and ws(4, 5, 64, 64) == 4 * 5 * 16 * 8
    assert ws(0, 1, 1, 1) == 0 and ws(1, 1, 1 << 16, 1 << 15) == 0


def test_argument_validation_without_gpu():
    """The entry points refuse bad shapes and buffers before touching the device."""
    hip, lib = _lib()
    EINVAL, ESHAPE, EWORKSPACE = -1, -2, -4
    x0, n, o, t, tab, m, md, out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000      # never dereferenced

    def fill(x0=x0, n=n, o=o, t=t, tab=tab, T=1000, m=m, md=md, B=3, F=5, H=16, W=16, out=out, ld=64, c_pad=64):
        return lib.rcdm_diffuse_assemble(x0, n, o, 0.1, t, tab, T, m, md, B, F, H, W, out, ld, c_pad, 0)

    for kw in (dict(x0=0), dict(n=0), dict(t=0), dict(tab=0), dict(m=0), dict(md=0), dict(out=0), dict(T=0), dict(B=0), dict(F=0),
               dict(H=0), dict(W=0), dict(x0=x0 + 2), dict(o=o + 2), dict(t=t + 4), dict(out=out + 8)):
        assert fill(**kw) == EINVAL, kw
    for kw in (dict(c_pad=8, ld=8), dict(c_pad=20, ld=24), dict(c_pad=16, ld=20), dict(c_pad=64, ld=56), dict(c_pad=1032, ld=1032),
               dict(B=1 << 10, F=1 << 10, H=1 << 6, W=1 << 5)):
        assert fill(**kw) == ESHAPE, kw

    def sq(eps=out, ld=8, n=n, o=o, B=3, F=5, H=17, W=16, blocks=0, res=x0, ws=m, nb=3 * 5 * 2 * 8):
        return lib.rcdm_eps_sqerr(eps, ld, n, o, 0.1, B, F, H, W, blocks, res, ws, nb, 0)

    for kw in (dict(eps=0), dict(n=0), dict(res=0), dict(blocks=-1), dict(blocks=65536), dict(B=0), dict(eps=out + 4), dict(n=n + 1),
               dict(o=o + 2), dict(res=x0 + 4), dict(ws=m + 4)):
        assert sq(**kw) == EINVAL, kw
    for kw in (dict(ld=2), dict(ld=6), dict(B=1 << 10, F=1 << 10, H=1 << 6, W=1 << 5)):
        assert sq(**kw) == ESHAPE, kw
    assert sq(ws=0) == EWORKSPACE and sq(nb=3 * 5 * 2 * 8 - 8) == EWORKSPACE
