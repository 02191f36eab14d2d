"""GPU tests of the LayerNorm kernels on rows that lie far from zero (tests/ln_cond.py: inputs, float64 reference, budgets):
rcdm_layernorm (both forms of the row-group kernel, and the wave-per-row kernel behind RCDM_LN_WAVEROW in a child process),
the LayerNorm epilogue of rcdm_gemm_ln, and the deferred form rcdm_gemm_lnx — its statistics, read through a probe consumer,
and its outputs through plain, GEGLU and row-vector consumers.  Every operand sits in a guarded buffer (tests/guard.py).

The probe.  A consumer's epilogue forms y = rstd acc - (mean rstd) S in fp32 and rounds it to f16,
so a statistic is only visible through an f16 — 11 bits, where the budgets need 17.  The probe
therefore asks questions whose answer is ONE rounding decision.  Its A rows are the case's rows followed by 40 columns of
per-row constants, its W' is zero on the case's columns (Lnx.C stays C: the statistics are the producer's), and colsum is the
caller's:
  rstd   T = a midpoint between two neighbouring f16 values near 16 rstd64.  For a threshold d the column "+d" accumulates
         a = T / ((1 - d) rstd64) (two f16 pieces, weights 1 and 2^-7: 22 bits) with S = 0, so the stored half lies above T
         exactly when rstd / rstd64 - 1 > -d; the column "-d", a = T / ((1 + d) rstd64), lies below T exactly when it is < d.
         Thresholds are LEVELS x the row's budget; the smallest level whose two columns both answer "inside" brackets the
         row's error, and level 1 is the assertion.  Resolution RES_RSTD = 2^-21 (the 22-bit a, the fp32 product), added to
         the budget explicitly.
  mean   one column accumulates 64 fl32(mean64) (three f16 pieces) with S = 64: it returns 64 rstd (mean64 - mean), small, so
         its f16 rounding is relative to the error itself.  Resolution: the fp32 roundings of a, of mean rstd and of
         (mean rstd) S, 3 x 2^-24 |mean64| rstd64 — up to 4.9e-5 sigma at ratio 274 —, added to the budget explicitly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ln_cond as L
from tests.guard import check_all
from tests.test_hip_kernels import DEV, gin, gout, gvec, gw

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))   # noqa: E731
PRODUCER_VARIANTS = [1, 2, 3, 4, 5, 10]
CONSUMER_VARIANTS = [-1, 1, 2, 3, 4, 5, 6, 7, 9, 10]
EPS = L.EPS

_inputs = {}


def case_rows(shape, case):
    if (shape, case) not in _inputs:
        _inputs[(shape, case)] = L.make_input(*shape, case)
    return _inputs[(shape, case)]


def t16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).half()


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---- rcdm_layernorm ---------------------------------------------------------------------------------------------------------
LATE_SHAPE = (24613, 64)       # more than 3 x 256 blocks of 32 rows: the row-group kernel's late-parameter form
LN_FORMS = {(300, 64): (8, 1, True), (97, 200): (8, 4, True), (1000, 640): (16, 5, True), (640, 1280): (32, 5, True),
            LATE_SHAPE: (8, 1, False)}


def ln_form(M, C):
    """norm.hip's dispatch rule: (lanes per row, 16-byte chunks per lane, affine parameters requested early)."""
    nchunks = C // 8
    lpr = 8 if nchunks <= 40 else 16 if nchunks <= 80 else 32 if nchunks <= 160 else 64
    rows_per_block = 4 * (64 // lpr)
    return lpr, min((nchunks + lpr - 1) // lpr, 5), (M + rows_per_block - 1) // rows_per_block <= 3 * 256


def run_layernorm(hip, shape, case, with_pe):
    M, C = shape
    x = case_rows(shape, case)
    kinds = L.row_kinds(M, case)
    gamma, beta = L.affine(C)
    rpf, frames = 20, 5
    pe = (0.5 * np.random.default_rng([37, C]).standard_normal((frames, C))).astype(np.float32)
    shift = pe[(np.arange(M) // rpf) % frames] if with_pe else None
    xd, gd, bd, pd = gin(t16(x), C + 8), gvec(t32(gamma)), gvec(t32(beta)), gvec(t32(pe))
    y = gout(M, C, C + 16)
    d = hip.LayerNormDesc(M, C, C + 8, C + 16, EPS, rpf, frames)
    hip.layernorm(d, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), pd.data_ptr() if with_pe else 0, y.data_ptr())
    torch.cuda.synchronize()
    check_all(y, xd, gd, bd, pd)
    return L.assert_plain_output(host(y[:, :C]), x, gamma, beta, kinds, f"rcdm_layernorm {shape} {case} pe {with_pe}", shift=shift)


@pytest.mark.parametrize("with_pe", [False, True], ids=["plain", "pe"])
@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("shape", L.SHAPES + [LATE_SHAPE], ids=IDS)
def test_layernorm(hiplib, shape, case, with_pe):
    from rcdms_amd import hip
    assert not int(os.environ.get("RCDM_LN_WAVEROW", "0") or 0), "this test is about the row-group kernel"
    assert ln_form(*shape) == LN_FORMS[shape]
    run_layernorm(hip, shape, case, with_pe)


def test_layernorm_wave_per_row_kernel(hiplib):
    """layernorm_kernel runs only with RCDM_LN_WAVEROW=1, which the library reads once per process: every case x shape, with and
    without the table, in one child process."""
    env = dict(os.environ, RCDM_LN_WAVEROW="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_hip_ln_cond"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "wave-per-row: worst" in r.stdout


# ---- rcdm_gemm_ln -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("shape", [(300, 64), (97, 200), (330, 320)], ids=IDS)
def test_gemm_ln(hiplib, shape, case):
    """A = 0: the stored row is the residual, so `out` carries the case bit for bit and the epilogue normalises exactly it."""
    from rcdms_amd import hip
    M, C = shape
    K = 64
    x = case_rows(shape, case)
    kinds = L.row_kinds(M, case)
    gamma, beta = L.affine(C)
    g = torch.Generator().manual_seed(M + C)
    Ad, Wd, Rd = gin(torch.zeros(M, K).half()), gw(torch.randn(C, K, generator=g) * K ** -0.5), gin(t16(x))
    gd, bd = gvec(t32(gamma)), gvec(t32(beta))
    out, y = gout(M, C, C + 8), gout(M, C, C + 8)
    d = hip.GemmDesc(M, C, K, K, C + 8, C, 4, 1, 0, 1.0, 1, 0)
    ln = hip.LnFuse(gd.data_ptr(), bd.data_ptr(), 0, y.data_ptr(), C + 8, 1, 1, EPS)
    hip.gemm_ln(d, ln, Ad.data_ptr(), Wd.data_ptr(), 0, Rd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, y, Ad, Wd, Rd, gd, bd)
    assert torch.equal(out[:, :C].cpu(), t16(x)), "the stored rows are not the case"
    L.assert_plain_output(host(y[:, :C]), x, gamma, beta, kinds, f"rcdm_gemm_ln {shape} {case}")


# ---- rcdm_gemm_lnx: placing the rows ----------------------------------------------------------------------------------------
class Placed:
    """The case's rows stored by a statistics-producing launch (A = 0, no bias, residual = the case) and its slots."""

    def __init__(self, hip, x, variant=-1, dup=0):
        M, C = x.shape
        K = 64
        self.M, self.C, self.dup = M, C, dup
        hip.set_igemm_variant(variant)
        try:
            d = hip.GemmDesc(M, C, K, K, C, C, 4, 1, 0, 1.0, 1, dup)
            self.parts = hip.gemm_stat_parts(d)
            assert self.parts > 0
            self.rows = gout(M + dup, C)
            self.stat_h = gout(1, (M + dup) * self.parts * 2, dtype=torch.float32, guard_rows=1)
            Ad, Wd, Rd = gin(torch.zeros(M, K).half()), gw(torch.zeros(C, K)), gin(t16(x))
            lx = hip.Lnx(self.stat_h[0].data_ptr(), self.parts, M + dup, 0, 0, 0, 0, EPS, 0)
            hip.gemm_lnx(d, lx, Ad.data_ptr(), Wd.data_ptr(), 0, 0, Rd.data_ptr(), self.rows.data_ptr(), 0, 0)
            torch.cuda.synchronize()
        finally:
            hip.set_igemm_variant(-1)
        check_all(self.rows, self.stat_h, Ad, Wd, Rd)
        want = t16(x)
        assert torch.equal(self.rows[:M].cpu(), want), "the stored rows are not the case"
        assert not dup or torch.equal(self.rows[dup:dup + M].cpu(), want), "the dup rows are not the case"
        assert torch.isfinite(self.stat_h[0]).all(), "a statistics slot was not written"

    def stat_ptr(self, row0=0):
        return self.stat_h[0].data_ptr() + 8 * row0

    @property
    def stat_rows(self):
        return self.M + self.dup


_placed = {}


def placed_auto(hip, shape, case):
    """The automatic producer's rows and slots of (shape, case): placed once, shared by the tests of this module, read-only."""
    if (shape, case) not in _placed:
        _placed[(shape, case)] = Placed(hip, case_rows(shape, case))
    return _placed[(shape, case)]


# ---- rcdm_gemm_lnx: the statistics probe ------------------------------------------------------------------------------------
LEVELS = [0.25, 0.5, 1.0, 4.0, 16.0, 64.0, 256.0, 1024.0]
RES_RSTD = 2.0 ** -21
PROBE_N, PROBE_EXTRA = 24, 40
MEAN_COL, MEAN_GAIN = 2 * len(LEVELS), 64.0


def _f16_down(v):
    h = v.astype(np.float16)
    return np.where(h.astype(np.float64) > v, np.nextafter(h, np.float16(-np.inf)), h)


class Probe:
    """Host side of the probe for one (shape, case): the 40 extra A columns, W', colsum and what the answers mean."""

    def __init__(self, x, kinds):
        M, C = x.shape
        self.x, self.kinds, self.M, self.C = x, kinds, M, C
        self.mean64, self.var64, self.rstd64 = L.reference(x, EPS)
        const = kinds == "constant"
        self.budget = np.full(M, L.RSTD_REL + RES_RSTD)
        self.budget[const] = L.const_rstd_budget(self.mean64[const], EPS) + RES_RSTD
        lo = _f16_down(16.0 * self.rstd64)
        self.T = (lo.astype(np.float64) + np.nextafter(lo, np.float16(np.inf)).astype(np.float64)) / 2.0
        extra = np.zeros((M, PROBE_EXTRA))
        W = np.zeros((PROBE_N, C + PROBE_EXTRA))
        for i, lv in enumerate(LEVELS):
            d = lv * self.budget
            for j, a in enumerate((self.T / ((1.0 - d) * self.rstd64), self.T / ((1.0 + d) * self.rstd64))):   # "+d", "-d"
                col = 2 * i + j
                a = a.astype(np.float32).astype(np.float64)
                hi = L.f16(a).astype(np.float64)
                extra[:, 2 * col], extra[:, 2 * col + 1] = hi, L.f16((a - hi) * 128.0)
                W[col, C + 2 * col], W[col, C + 2 * col + 1] = 1.0, 2.0 ** -7
        m = self.mean64.astype(np.float32).astype(np.float64)
        p0 = L.f16(m).astype(np.float64)
        p1 = L.f16((m - p0) * 128.0).astype(np.float64)
        p2 = L.f16((m - p0 - p1 / 128.0) * 16384.0).astype(np.float64)
        assert (p0 + p1 / 128.0 + p2 / 16384.0 == m).all()
        extra[:, 32:35] = np.stack([p0, p1, p2], axis=1)
        W[MEAN_COL, C + 32:C + 35] = MEAN_GAIN, MEAN_GAIN / 128.0, MEAN_GAIN / 16384.0
        assert (L.f16(W) == W).all() and (L.f16(extra) == extra).all()
        self.A = np.concatenate([x.astype(np.float64), extra], axis=1)
        self.W = W
        self.S = np.zeros(PROBE_N)
        self.S[MEAN_COL] = MEAN_GAIN
        self._dev = None

    def device(self):
        if self._dev is None:
            self._dev = (gin(t16(self.A)), gw(t16(self.W).float()), gvec(t32(self.S)))
        return self._dev

    def figures(self, out):
        """out [M][PROBE_N] (float64 of the stored halfs) -> worst figure of each statistics budget as a fraction of it (rstd:
        the smallest level that brackets every row's error)."""
        assert np.isfinite(out).all(), "non-finite probe output"
        lvl = np.full(self.M, np.inf)
        for i, lv in reversed(list(enumerate(LEVELS))):
            ok = (out[:, 2 * i] > self.T) & (out[:, 2 * i + 1] < self.T)
            lvl = np.where(ok & (lvl == (LEVELS[i + 1] if i + 1 < len(LEVELS) else np.inf)), lv, lvl)
        dm = np.abs(out[:, MEAN_COL]) / (MEAN_GAIN * self.rstd64)            # |mean64 - mean|
        res = 3.0 * 2.0 ** -24 * np.abs(self.mean64)
        const = self.kinds == "constant"
        sig = np.sqrt(np.where(const, 1.0, self.var64))
        bud = np.where(const, 2.0 * L.ulp32(self.mean64), L.MEAN_SIG * sig) + res
        fm = dm / (bud * (1.0 + 2.0 ** -10))
        pick = lambda v, sel: float(v[sel].max()) if sel.any() else 0.0   # noqa: E731
        return {"rstd": pick(lvl, ~const), "mean": pick(fm, ~const), "const_rstd": pick(lvl, const), "const_mean": pick(fm, const)}


_probes = {}


def probe_of(shape, case):
    if (shape, case) not in _probes:
        _probes[(shape, case)] = Probe(case_rows(shape, case), L.row_kinds(shape[0], case))
    return _probes[(shape, case)]


def run_probe(hip, pr, placed, cvariant=-1, stat_row0=0, both_sides=False):
    M, C = pr.M, pr.C
    Ad, Wd, Sd = pr.device()
    K = C + PROBE_EXTRA
    out = gout(M, PROBE_N, PROBE_N + 8)
    d = hip.GemmDesc(M, PROBE_N, K, K, PROBE_N + 8, 0, 0, 1, 0, 1.0, 1, 0)
    extra = []
    hip.set_igemm_variant(cvariant)
    try:
        so, sp = 0, 0
        if both_sides:
            sp = hip.gemm_stat_parts(d, consumer=True)
            assert sp > 0
            s2 = gout(1, M * sp * 2, dtype=torch.float32, guard_rows=1)
            so = s2[0].data_ptr()
            extra.append(s2)
        lx = hip.Lnx(so, sp, M if both_sides else 0, placed.stat_ptr(stat_row0), placed.parts, placed.stat_rows, Sd.data_ptr(), EPS, C)
        hip.gemm_lnx(d, lx, Ad.data_ptr(), Wd.data_ptr(), 0, 0, 0, out.data_ptr(), 0, 0)
        torch.cuda.synchronize()
    finally:
        hip.set_igemm_variant(-1)
    check_all(out, Ad, Wd, Sd, placed.stat_h, *extra)
    if both_sides:
        assert torch.isfinite(extra[0][0]).all(), "a statistics slot of the two-sided call was not written"
    return pr.figures(host(out[:, :PROBE_N]))


@pytest.mark.parametrize("case", L.CASES)
@pytest.mark.parametrize("shape", L.SHAPES, ids=IDS)
def test_lnx_statistics(hiplib, shape, case):
    """(rstd, mean rstd) as every consumer tile forms them from every producer tile's slots, read through the probe."""
    from rcdms_amd import hip
    M, C = shape
    x = case_rows(shape, case)
    pr = probe_of(shape, case)
    runs = []
    auto = placed_auto(hip, shape, case)
    for cv in CONSUMER_VARIANTS:
        runs.append((f"consumer {cv}", run_probe(hip, pr, auto, cv)))
    for pv in PRODUCER_VARIANTS:
        runs.append((f"producer {pv}", run_probe(hip, pr, Placed(hip, x, pv))))
    runs.append(("dup_rows producer, dup half", run_probe(hip, pr, Placed(hip, x, -1, dup=M), stat_row0=M)))
    runs.append(("consumer and producer at once", run_probe(hip, pr, auto, both_sides=True)))
    worst = {k: max(f[k] for _, f in runs) for k in runs[0][1]}
    print(f"lnx statistics {shape} {case}: of the budgets (rstd: bracketing level): rstd {worst['rstd']:.3g}, mean {worst['mean']:.3f}, "
          f"constant rows' rstd {worst['const_rstd']:.3g}, constant rows' mean {worst['const_mean']:.3f}")
    bad = [name for name, f in runs if max(f.values()) > 1.0]
    assert not bad, f"{shape} {case}: outside the statistics budgets (worst figures {worst}) with: " + ", ".join(bad)


# ---- rcdm_gemm_lnx: outputs -------------------------------------------------------------------------------------------------
OUT_N = 256
_weights = {}


def weights(N, C):
    if (N, C) not in _weights:
        _weights[(N, C)] = L.consumer_weights(N, C)
    return _weights[(N, C)]


@pytest.mark.parametrize("form", ["plain", "geglu", "rowvec64", "rowvec20"])
@pytest.mark.parametrize("case", ["r64", "r128", "r256", "spread", "mixed", "constant"])
@pytest.mark.parametrize("shape", [(1000, 640), (640, 1280)], ids=IDS)
def test_lnx_outputs(hiplib, shape, case, form):
    """Every consumer tile on the automatic producer's rows and slots, against the float64 LayerNorm -> Linear and the budgets
    of tests/ln_cond.py; finiteness everywhere; GEGLU on constant rows: finiteness only.

    Bias and row vector are in the accumulators BEFORE the one rounding to f16 in every tile kernel — through the column tables
    where a tile meets at most two samples, row by row where rows_per_sample is below the tile's row count (rowvec20 on every
    tile, rowvec64 on the tiles of 128 rows and more) —: added after it, they cost a second rounding, 2^-11 |y - rowvec|, which
    alone is twice what the budget grants where y is near zero (measured 1.3 .. 1.9 x the budget before they moved)."""
    from rcdms_amd import hip
    M, C = shape
    x = case_rows(shape, case)
    kinds = L.row_kinds(M, case)
    const, control = kinds == "constant", kinds == "control"
    exact = ~const & ~control
    pl = placed_auto(hip, shape, case)
    N = 2 * OUT_N if form == "geglu" else OUT_N
    w = weights(N, C)
    epi, rps, ldt, rowvec_d, bias_d, shift = 1, 1, 0, 0, 0, None
    keep = []
    if form == "geglu":
        Wf, bf = gin(t32(w["Wp"])), gvec(t32(w["bp"]))
        Wd = gout(N, C)
        bias_t = gout(1, N, dtype=torch.float32, guard_rows=1)
        hip.pack_geglu_rows(Wf.data_ptr(), bf.data_ptr(), N, C, Wd.data_ptr(), bias_t.data_ptr())
        torch.cuda.synchronize()
        Sd = gvec(Wd[:, :C].float().sum(dim=1))
        bias_d, epi = bias_t.data_ptr(), 1 | 8
        keep += [Wf, bf, bias_t]
        full = L.consumer64(x, w)
        tol_full = L.consumer_budget(full, w, x, kinds)
        h64, g64 = full[:, :OUT_N], full[:, OUT_N:]
        y64 = h64 * L.gelu64(g64)
        tol = L.geglu_budget(h64, g64, tol_full[:, :OUT_N], tol_full[:, OUT_N:])
    else:
        Wd, Sd = gw(t16(w["Wp"]).float()), gvec(t32(w["S"]))
        if form.startswith("rowvec"):
            rpf, frames = int(form[6:]), 5
            pe = np.random.default_rng([41, C]).choice([0.0, 0.25, -0.25, 0.5, -0.5], (frames, C))
            nsamp = (M + rpf - 1) // rpf
            tab = np.stack([w["bp"] + w["W"] @ pe[s % frames] for s in range(nsamp)]).astype(np.float32)
            shift = (tab.astype(np.float64) - w["bp"][None, :])[np.arange(M) // rpf]
            tab_d = gvec(t32(tab))
            rowvec_d, rps, ldt, epi = tab_d.data_ptr(), rpf, N, 2
            keep.append(tab_d)
        else:
            bias_t = gvec(t32(w["bp"]))
            bias_d = bias_t.data_ptr()
            keep.append(bias_t)
        y64 = L.consumer64(x, w, shift=shift)
        tol = L.consumer_budget(y64, w, x, kinds, shift=shift)
    worst = {"exact rows": 0.0, "constant rows": 0.0, "control rows": 0.0}
    bad = []
    for cv in CONSUMER_VARIANTS:
        out = gout(M, OUT_N, OUT_N + 8)
        d = hip.GemmDesc(M, N, C, C, OUT_N + 8, 0, epi, rps, ldt, 1.0, 1, 0)
        lx = hip.Lnx(0, 0, 0, pl.stat_ptr(), pl.parts, pl.stat_rows, Sd.data_ptr(), EPS, C)
        hip.set_igemm_variant(cv)
        try:
            hip.gemm_lnx(d, lx, pl.rows.data_ptr(), Wd.data_ptr(), bias_d, rowvec_d, 0, out.data_ptr(), 0, 0)
            torch.cuda.synchronize()
        finally:
            hip.set_igemm_variant(-1)
        check_all(out, pl.rows, pl.stat_h, Sd, *keep)
        y = host(out[:, :OUT_N])
        assert np.isfinite(y).all(), f"consumer {cv}: non-finite output"
        fig = {"exact rows": float((np.abs(y - y64)[exact] / tol[exact]).max()) if exact.any() else 0.0,
               "constant rows": float((np.abs(y - y64)[const] / tol[const]).max()) if const.any() and form != "geglu" else 0.0,
               "control rows": L.control_close(y[control], y64[control])}
        for k, v in fig.items():
            worst[k] = max(worst[k], v)
            if v > 1.0:
                bad.append(f"consumer {cv}: {k} at {v:.3f}")
    print(f"lnx outputs {shape} {case} {form}: of the budgets: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not bad, f"{shape} {case} {form}: outside the output budgets: " + "; ".join(bad)


if __name__ == "__main__":    # the child process of test_layernorm_wave_per_row_kernel
    assert os.environ.get("RCDM_LN_WAVEROW") == "1"
    from rcdms_amd import hip as _hip
    _hip.load()
    _worst = 0.0
    for _shape in L.SHAPES:
        for _case in L.CASES:
            for _pe in (False, True):
                _worst = max(_worst, run_layernorm(_hip, _shape, _case, _pe))
    print(f"wave-per-row: worst output error {_worst:.3f} of its budget")
