"""Exact-answer cases for the row chains and the fused feed-forward (rcdm_rowchain, rcdm_ff_fused, rowff.hip, and the packers
pack_pgemm_kernel / pack_ff_stream_kernel behind them): operands on which every value the kernel rounds to f16 is a small
integer, so the token rows and the tail's output have to come back bit for bit, whatever the order of the sums and wherever
the roundings sit.  Shared by tests/test_rowchain_exact_host.py (CPU: the conditions hold, and a model that misplaces one
term is rejected) and tests/test_hip_rowchain_exact.py (GPU).  Needs numpy only.

Why it is exact (all of it asserted by check_case on the reference before any launch):

  integers    A product of f16 values holding small integers is exact, an fp32 sum of integers is exact in any order while the
              sum of the magnitudes stays below 2^24, and f16 holds every integer of magnitude <= 2048.  Every value the
              kernel rounds to f16 — tok, the LayerNorm output y, q | k | v, the GEGLU product h, the feed-forward
              accumulator, its sum with b2 and the residual, the trailing projection at both of its roundings — is such an
              integer in the reference (h: an integer times 16, below 2^15).  No rounding point matters then.
  LayerNorm   tok[r] = m_r + v_r s_r with s_r a +-1 row of exactly 160 of each sign, v_r in {1, 2, 4}, m_r in {0, +-16 v_r,
              +-64 v_r}: the mean is m_r, the variance v_r^2, the normalised row s_r / sqrt(1 + eps / v_r^2).  With integer
              gamma, beta and pe the true y lies within a relative 5e-6 of the integer s gamma + beta (+ pe), and any fp32
              evaluation whose relative error is below 2^-13 rounds it to that integer — provided the integer is not 0 (the
              true value would be an f16 subnormal), which is why beta is 0 wherever |gamma| = 1.
  GELU        at a gate pre-activation x >= 16 gelu(x) = x, at x <= -16 it is -0, at 0 it is 0: for the polynomial forms of
              rowff.hip / common.h (exp2(-0.72 x^2) underflows) and for erf alike.  The gate pre-activations are drawn from
              {0} and the multiples of 16.

The model (model()) is float64 with the kernel's f16 roundings where the kernel has them; on these operands no rounding
changes anything, on the random operands of the tolerance suites it is the reference arithmetic.  It takes a `mutate`
argument: one misplaced term each (MUTATIONS), for the host test to show that exact equality catches it and how much of it
close() of tests/test_hip_kernels.py lets through on that suite's random operands.

Deliberately NOT pinned here, and left to the tolerance tests (tests/test_hip_rowff.py, tests/test_hip_motion_fused.py): the
pe row map of the frame-major tail (tail 4 runs without pe here), GELU between its saturated ends (pinned value by value by
tests/act_sweep.py / tests/test_hip_act_sweep.py), and LayerNorm on rows that are not two-valued (on two-valued f16 rows
even E[x^2] - mean^2 in fp32 is exact: see MUTATIONS["ln_var_e2"])."""
import math

import numpy as np

from tests import attn_exact as AX
from tests.gemm_exact import acts, close_accepts, gen, ints, signs   # noqa: F401  (close_accepts: for the host test)

C, EPS, BLOCK_ROWS, GN_GROUPS, HEADS, D, F = 320, 1e-5, 160, 32, 8, 40, 5
NK, NOF = C // 32, C // 16
SEL_T = AX.sel_t(D)             # 76 = ceil(12 sqrt 40)


def f16r(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def is_f16(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.isfinite(x).all() and (f16r(x) == x).all())


def is_int(x, bound=2048):
    x = np.asarray(x, dtype=np.float64)
    return bool((x == np.rint(x)).all() and np.abs(x).max() <= bound)


def frag_channels(i):
    """The 16 channels of output fragment i of an N = C GEMM in the P layout (rowff.hip: D row r of fragment i <-> channel
    32 (i >> 1) + 8 (r >> 2) + 4 (i & 1) + (r & 3))."""
    r = np.arange(16)
    return 32 * (i >> 1) + 8 * (r >> 2) + 4 * (i & 1) + (r & 3)


def gelu(x):
    """The exact erf GELU in float64 (attention.py's GEGLU: F.gelu)."""
    u, inv = np.unique(np.asarray(x, dtype=np.float64), return_inverse=True)
    e = np.array([math.erf(t / math.sqrt(2.0)) for t in u])
    return (0.5 * u * (1.0 + e))[inv].reshape(np.shape(x))


# ---- operands -----------------------------------------------------------------------------------------------------------
def signed_perm(g, mult, shift):
    """W[n][(mult n + shift) % C] = +-1: a signed permutation whose every output fragment draws from many k-steps."""
    assert math.gcd(mult, C) == 1
    W = np.zeros((C, C))
    W[np.arange(C), (mult * np.arange(C) + shift) % C] = signs(g, C)
    return W


LN_COMBOS = [(v, k) for v in (1, 2, 4) for k in (0, 16, -16, 64, -64)]


def two_valued_rows(g, M):
    """(T, s): T[r] = v_r (k_r + s_r), s_r a +-1 row with 160 of each sign; the first 15 rows take every (v, k) once."""
    idx = np.concatenate([g.permutation(15), g.integers(0, 15, size=max(M - 15, 0))])[:M]
    v = np.array([LN_COMBOS[i][0] for i in idx], dtype=np.float64)
    k = np.array([LN_COMBOS[i][1] for i in idx], dtype=np.float64)
    s = g.permuted(np.tile(np.repeat([1.0, -1.0], C // 2), (M, 1)), axis=1)
    return (v * k)[:, None] + v[:, None] * s, s


def ln_params(g, kind, frames):
    """(gamma, beta, pe).  "C": |gamma| in {3, 4}, beta and pe in {-1, 0, 1} (1 <= |y| <= 6); "rich": |gamma| in {1, 2}, beta in
    {-1, 0, 1} where |gamma| = 2 (else 0: y is never 0); "plain": gamma +-1, beta 0; "one": gamma 1, beta 0."""
    if kind == "C":
        gamma, beta = g.choice(np.array([-4.0, -3.0, 3.0, 4.0]), size=C), ints(g, 1, C)
    elif kind == "rich":
        gamma = g.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=C)
        beta = ints(g, 1, C) * (np.abs(gamma) == 2)
    elif kind == "plain":
        gamma, beta = signs(g, C), np.zeros(C)
    else:
        assert kind == "one", kind
        gamma, beta = np.ones(C), np.zeros(C)
    pe = None
    if frames:
        assert kind == "C", "pe rides only where |gamma| >= 3"
        pe = ints(g, 1, frames, C)
        assert len(np.unique(pe, axis=0)) == frames
    return gamma, beta, pe


def head_cycle(g):
    """sig: a permutation of the channels of order 5 that keeps every 40-channel head block (eight 5-cycles per head, the
    channels of a cycle scattered over the head's 8-channel pieces)."""
    sig = np.empty(C, dtype=np.int64)
    for h in range(HEADS):
        p = g.permutation(D)
        inv = np.argsort(p)
        sig[h * D:(h + 1) * D] = h * D + p[(inv + 8) % D]
    x = np.arange(C)
    for _ in range(5):
        x = sig[x]
    assert (x == np.arange(C)).all() and (sig != np.arange(C)).all() and (sig // D == np.arange(C) // D).all()
    return sig


def on_set(P, phase):
    unit = np.arange(4 * C)
    return (unit % 32 + unit // 32) % P == phase


# ---- the cases ----------------------------------------------------------------------------------------------------------
DEFAULTS = dict(form="chain", tail=3, M=160, stage="res", ln="rich", pe_frames=0, rpf=1, gn_rows=0, ff=None, att=None, b=0, hw=0,
                alias=None)


def S(name, **kw):
    assert not set(kw) - set(DEFAULTS), kw
    return dict(DEFAULTS, name=name, **kw)


HID4 = lambda ph: ("hid", 4, ph)        # hidden-dense, every fourth hidden unit on (needs the plain LayerNorm)
HID16 = lambda ph: ("hid", 16, ph)      # ... every sixteenth (the richer LayerNorm)
GATE = ("gate",)

# A. stage A in every reachable instantiation (HAS_A x A_RES x LN_PE x TAIL; tail 4: section E), tok aliasing res, the dense
#    no-residual form whose LayerNorm is not exact (out by close())
CASES_A = [
    S("A-t1-res", tail=1, M=480), S("A-t1-res-pe", tail=1, M=333, ln="C", pe_frames=5, rpf=64),
    S("A-t1-perm", tail=1, M=176, stage="perm"), S("A-t1-perm-pe", tail=1, M=160, stage="perm", ln="C", pe_frames=8, rpf=20),
    S("A-t3-res", tail=3, M=333), S("A-t3-res-pe", tail=3, M=480, ln="C", pe_frames=8, rpf=20),
    S("A-t3-perm", tail=3, M=16, stage="perm"), S("A-t3-perm-pe", tail=3, M=176, stage="perm", ln="C", pe_frames=5, rpf=64),
    S("A-t0-res", tail=0, M=176, ff=HID16(3)), S("A-t0-perm", tail=0, M=333, stage="perm", ln="plain", ff=GATE),
    S("A-t2-res", tail=2, M=160, ln="plain", ff=HID4(1)),
    S("A-t3-dense", tail=3, M=333, stage="dense"), S("A-t0-dense", tail=0, M=176, stage="dense", ln="plain", ff=HID4(2)),
    S("A-t3-tok-over-res", tail=3, M=333, alias="tok"), S("A-t0-in-place", tail=0, M=480, ff=HID16(9), alias="tok+out"),
    S("A-t2-tok-over-res", tail=2, M=333, ln="plain", ff=GATE, alias="tok"),
]
# B. the GroupNorm apply in the prologue, statistics supplied: 176 rows per sample (blocks of 160 rows straddle samples, also
#    in the middle of the tensor) and 160
CASES_B = [
    S("B-176-t3", tail=3, M=480, stage="perm", gn_rows=176), S("B-160-t1", tail=1, M=480, stage="perm", gn_rows=160),
    S("B-176-t0", tail=0, M=480, stage="perm", ln="plain", ff=HID4(0), gn_rows=176),
    S("B-176-t3-pe", tail=3, M=480, stage="perm", ln="C", pe_frames=5, rpf=64, gn_rows=176),
    S("B-176-t3-dense", tail=3, M=480, stage="dense", gn_rows=176),
]
# C. LayerNorm + pe -> tail GEMM: frames in {5, 8}, rows per frame 64 (the frame changes inside a block) and 20 (inside a wave)
CASES_C = [
    S("C-t3-f5-r64", tail=3, M=480, ln="C", pe_frames=5, rpf=64), S("C-t3-f8-r20", tail=3, M=333, ln="C", pe_frames=8, rpf=20),
    S("C-t1-f8-r64", tail=1, M=176, stage="perm", ln="C", pe_frames=8, rpf=64), S("C-t1-f5-r20", tail=1, M=160, ln="C", pe_frames=5, rpf=20),
    S("C-t3-f5-r20", tail=3, M=16, stage="perm", ln="C", pe_frames=5, rpf=20),
]
# D. the feed-forward: rcdm_ff_fused and tails 0 / 2; hidden-dense through EVERY phase (each hidden unit on in exactly one
#    launch), gate-dense
CASES_D = (
    [S(f"D-ff-hid4-{ph}", form="ff", tail=0, stage=None, M=333, ln="plain", ff=HID4(ph)) for ph in range(4)]
    + [S(f"D-ff-hid16-M{M}", form="ff", tail=0, stage=None, M=M, ff=HID16((M // 16) % 16)) for M in (16, 160, 176, 480)]
    + [S("D-ff-gate-M480", form="ff", tail=0, stage=None, M=480, ln="plain", ff=GATE), S("D-ff-gate-M16", form="ff", tail=0, stage=None, M=16, ln="plain", ff=GATE)]
    + [S(f"D-t0-hid16-{ph}", tail=0, M=333, ff=HID16(ph)) for ph in range(16)]
    + [S(f"D-t2-hid4-{ph}", tail=2, M=480, ln="plain", ff=HID4(ph)) for ph in range(4)]
    + [S("D-t2-hid16", tail=2, M=176, ff=HID16(5)), S("D-t2-gate", tail=2, M=333, ln="plain", ff=GATE), S("D-t0-gate", tail=0, M=160, ln="plain", ff=GATE)]
)
# E. tail 4 (no pe: the pe row map of the frame-major blocks stays with tests/test_hip_motion_fused.py): (b, hw) = (1, 32) one
#    full block, (1, 48) a block with a dead group of five waves, (2, 48) a block whose two groups lie in different samples
CASES_E = [
    S("E-unity-1-32", tail=4, att="unity", b=1, hw=32, alias="engine"), S("E-unity-1-48", tail=4, att="unity", b=1, hw=48, stage="perm", gn_rows=48),
    S("E-unity-2-48", tail=4, att="unity", b=2, hw=48),
    S("E-select-1-32", tail=4, att="select", b=1, hw=32, stage="perm", ln="one"), S("E-select-1-48", tail=4, att="select", b=1, hw=48, ln="one"),
    S("E-select-2-48", tail=4, att="select", b=2, hw=48, stage="perm", ln="one", gn_rows=48),
]
for _s in CASES_E:
    _s["M"], _s["rpf"] = _s["b"] * F * _s["hw"], _s["hw"]
# F. one case of A - D at M = 480, launched twice
CASES_F = ["A-t1-res", "B-176-t3", "C-t3-f5-r64", "D-t2-hid4-0"]

ALL_CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E
BY_NAME = {s["name"]: s for s in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

_cache = {}


def case(name):
    """Operands and reference of a case, built once, shared, never modified."""
    if name not in _cache:
        _cache[name] = build(BY_NAME[name])
    return _cache[name]


def _seed(spec):
    return [sum(map(ord, spec["name"])), spec["M"], spec["tail"]]


def build(spec):
    g = np.random.default_rng(_seed(spec))
    M, tail = spec["M"], spec["tail"]
    c = dict(spec, frames=max(spec["pe_frames"], 1), exact_ln=spec["stage"] != "dense")
    if tail == 4:
        c["frames"] = F
    gamma, beta, pe = ln_params(g, spec["ln"], spec["pe_frames"])
    c.update(ln_g=gamma, ln_b=beta, pe=pe)

    # ---- the token rows the LayerNorm is to see
    if spec["att"]:
        b, hw = spec["b"], spec["hw"]
        T0, s0 = two_valued_rows(g, b * hw)                      # one row per (sample, pixel)
        T0, s0 = T0.reshape(b, 1, hw, C), s0.reshape(b, 1, hw, C)
        if spec["att"] == "unity":                               # the five frames of a pixel share their row
            T, s = np.repeat(T0, F, axis=1), np.repeat(s0, F, axis=1)
        else:                                                    # frame f: the row of frame 0 through sig^f
            c["sig"] = sig = head_cycle(g)
            idx, Ts, ss = np.arange(C), [], []
            for _ in range(F):
                Ts.append(T0[..., idx])
                ss.append(s0[..., idx])
                idx = sig[idx]
            T, s = np.concatenate(Ts, axis=1), np.concatenate(ss, axis=1)
        T, s = T.reshape(M, C), s.reshape(M, C)
    else:
        T, s = two_valued_rows(g, M)
    rows = np.arange(M)

    # ---- stage A
    c["res"] = None
    if spec["stage"] is None:
        a = T
    else:
        c["ba"] = ints(g, 8, C)
        if spec["stage"] == "perm":
            c["wa"] = W = signed_perm(g, 37, 11)
            n, col = np.nonzero(W)
            a = np.zeros((M, C))
            a[:, col] = W[n, col] * (T[:, n] - c["ba"][n])
        else:
            a, c["wa"] = acts(g, M, C), signs(g, C, C)
            if spec["stage"] == "res":
                c["res"] = T - (a @ c["wa"].T + c["ba"])
            else:
                T = s = None
    c["T"], c["s"], c["a_applied"] = T, s, a
    if c["exact_ln"]:
        c["y_int"] = s * gamma + beta + (pe[(rows // spec["rpf"]) % c["frames"]] if pe is not None else 0.0)

    # ---- GroupNorm prologue: x such that the applied row is a
    c["gn"] = None
    if spec["gn_rows"]:
        assert c["res"] is None
        nsamp = -(-M // spec["gn_rows"])
        stat = np.stack([ints(g, 16, nsamp, GN_GROUPS), g.choice(np.array([0.5, 1.0, 2.0]), size=(nsamp, GN_GROUPS))], axis=2)
        gg, gb = signs(g, C), ints(g, 1, C)
        smp, grp = rows // spec["gn_rows"], np.arange(C) // (C // GN_GROUPS)
        a = stat[smp][:, grp, 0] + (a - gb) / (stat[smp][:, grp, 1] * gg)
        c["gn"] = dict(stat=stat, gamma=gg, beta=gb, rows=spec["gn_rows"])
    c["a"] = a

    # ---- the tail's weights
    if tail in (1, 3):
        c["wt"] = signs(g, tail * C, C)
    elif tail == 4:
        wt = signs(g, 3 * C, C)
        if spec["att"] == "unity":
            wt[:C] *= np.repeat(g.choice(np.array(AX.GAINS, dtype=np.float64), size=HEADS), D)[:, None]
        else:
            wt[:2 * C] = 0.0
            wt[np.arange(C), c["sig"]] = SEL_T                   # q_f = t (y_f o sig) = t y_(f+1) = t k_(f+1)
            wt[C + np.arange(C), np.arange(C)] = 1.0             # k_f = y_f
            wt[2 * C + np.arange(C), g.integers(0, C, size=C)] *= 2.0   # one +-2 per row of the v block: every v is odd
        c["wt"] = wt
    else:
        kind = spec["ff"][0]
        w1, b1 = np.zeros((8 * C, C)), np.zeros(8 * C)
        if kind == "hid":
            P, phase = spec["ff"][1:]
            w1[:4 * C] = signs(g, 4 * C, C)
            b1[:4 * C] = ints(g, 8, 4 * C)
            b1[4 * C:] = np.where(on_set(P, phase), 16.0, -16.0)
            w2 = signs(g, C, 4 * C) / 16.0
        else:
            assert spec["ln"] == "plain", "gate-dense needs y = +-1"
            w1[4 * C:] = 8.0 * signs(g, 4 * C, C)
            b1[:4 * C] = signs(g, 4 * C) / 16.0
            b1[4 * C:] = 16.0 * ints(g, 1, 4 * C)
            w2 = signs(g, C, 4 * C)
        c.update(w1=w1, b1=b1, w2=w2, b2=ints(g, 8, C))
        if tail == 2:
            c.update(wz=signed_perm(g, 93, 7), bz=ints(g, 8, C), zres=np.zeros((M, C)))
            pre = model(c)["ff"] @ c["wz"].T + c["bz"]
            z = ints(g, 16, M, C)
            c["zres"] = np.where(np.abs(pre + z) > 2048, -np.sign(pre) * np.abs(z), z)
    c["ref"] = model(c)
    return c


# ---- the model ----------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "stage_a_zero_kstep": "k-step 4 of stage A reads zeros in one wave (wave 3 of block 0; wave 0 of a one-wave launch)",
    "tail_stale_fragment": "the last k-step of the tail GEMM's second 160-column group reads fragment 3 of the first group's",
    "b1p_swap_pair": "hidden and gate bias of the 16-pair of hidden units 112..127 change places in b1p",
    "ff_b_next_group": "the B chunk (units 16..31) of feed-forward group 5 uses group 6's W1 rows",
    "pe_row_off_by_one": "the pe row is ((row + 1) / rpf) % frames: the last row of every frame takes the next frame's",
    "gn_sample_plus_one": "waves 5..9 of a block that straddles two GroupNorm samples use sample index + 1",
    "ln_var_e2": "LayerNorm in fp32 with the variance as E[x^2] - mean^2",
    "proj_skip_residual": "the operand of the trailing projection lacks the + tok residual in P-layout fragment 5",
    "att_v_next_frame": "in tail 4, frame f reads v of frame f + 1",
}


def _ln_fp32(tok, gamma, beta_pe, eps, e2, rstd_factor=1.0):
    """The LayerNorm as an fp32 kernel evaluates it (1.0f / C multiplied, not divided): two passes, or (e2) the variance
    as E[x^2] - mean^2.  Returns the unrounded fp32 y."""
    f = np.float32
    t = tok.astype(f)
    inv = f(1.0) / f(C)
    mean = (t.sum(axis=1, dtype=f) * inv)[:, None]
    if e2:
        var = (t * t).sum(axis=1, dtype=f)[:, None] * inv - mean * mean
    else:
        d = t - mean
        var = (d * d).sum(axis=1, dtype=f)[:, None] * inv
    rstd = (f(1.0) / np.sqrt(var + f(eps), dtype=f)) * f(rstd_factor)
    return (t - mean) * rstd * gamma.astype(f) + beta_pe.astype(f)


def model(c, mutate=None):
    """The chain in float64 with the kernel's f16 roundings.  Returns tok, y64 (before its rounding), y, out and the
    tail's intermediates."""
    assert mutate is None or mutate in MUTATIONS, mutate
    M, tail = c["M"], c["tail"]
    rows = np.arange(M)
    a = c["a"]
    m = {}
    if c["gn"] is not None:
        gn = c["gn"]
        nsamp = gn["stat"].shape[0]
        smp = rows // gn["rows"]
        if mutate == "gn_sample_plus_one":
            first = (rows // BLOCK_ROWS) * BLOCK_ROWS
            straddles = first // gn["rows"] != np.minimum(first + BLOCK_ROWS - 1, M - 1) // gn["rows"]
            hit = straddles & (rows % BLOCK_ROWS >= BLOCK_ROWS // 2)
            assert hit.any()
            smp = np.where(hit, np.minimum(smp + 1, nsamp - 1), smp)
        grp = np.arange(C) // (C // GN_GROUPS)
        mean, rstd = gn["stat"][smp][:, grp, 0], gn["stat"][smp][:, grp, 1]
        a = f16r(a * (rstd * gn["gamma"]) + (-(mean * rstd) * gn["gamma"] + gn["beta"]))     # gn_apply's scale / shift form
        m["a_applied"] = a
    if c["form"] == "ff":
        tok = a
    else:
        if mutate == "stage_a_zero_kstep":
            w = 3 if M > 64 else 0
            a = a.copy()
            a[16 * w:16 * w + 16, 32 * 4:32 * 5] = 0.0
        tok = a @ c["wa"].T + c["ba"]
        if c["res"] is not None:
            tok = tok + c["res"]
    m["tok"] = tok = f16r(tok)

    # ---- LayerNorm (+ pe)
    frames, rpf = c["frames"], c["rpf"]
    fr = (((rows + 1) if mutate == "pe_row_off_by_one" else rows) // rpf) % frames
    bpe = np.broadcast_to(c["ln_b"], (M, C)) + (c["pe"][fr] if c["pe"] is not None else 0.0)
    if mutate == "ln_var_e2":
        m["y64"] = _ln_fp32(tok, c["ln_g"], bpe, EPS, True).astype(np.float64)
    else:
        mean = tok.mean(axis=1, keepdims=True)
        var = ((tok - mean) ** 2).mean(axis=1, keepdims=True)
        m["y64"] = (tok - mean) / np.sqrt(var + EPS) * c["ln_g"] + bpe
    m["y"] = y = f16r(m["y64"])

    if tail in (1, 3):
        out = y @ c["wt"].T
        if mutate == "tail_stale_fragment":
            cols = 160 + frag_channels(3)
            ks = slice(32 * (NK - 1), C)
            out[:, cols] += y[:, ks] @ (c["wt"][cols - 160, ks] - c["wt"][cols, ks]).T
        m["out"] = f16r(out)
    elif tail == 4:
        b, hw = c["b"], c["hw"]
        m["qkv"] = qkv = f16r(y @ c["wt"].T)
        rg = lambda x: x.reshape(b, F, hw, HEADS, D).transpose(0, 2, 3, 1, 4)        # [b][pixel][head][frame][d]
        q, k, v = rg(qkv[:, :C]), rg(qkv[:, C:2 * C]), rg(qkv[:, 2 * C:])
        sc = np.einsum("bphfd,bphgd->bphfg", q, k) * D ** -0.5
        m["scores"] = sc
        p = np.exp(sc - sc.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        if mutate == "att_v_next_frame":
            v = np.roll(v, -1, axis=3)
        o = np.einsum("bphfg,bphgd->bphfd", p, v)
        m["out"] = f16r(o.transpose(0, 3, 1, 2, 4).reshape(M, C))
    else:
        w1, b1 = c["w1"], c["b1"]
        if mutate == "b1p_swap_pair":
            b1 = b1.copy()
            b1[112:128], b1[4 * C + 112:4 * C + 128] = c["b1"][4 * C + 112:4 * C + 128], c["b1"][112:128]
        if mutate == "ff_b_next_group":
            w1 = w1.copy()
            for base in (0, 4 * C):
                w1[base + 32 * 5 + 16:base + 32 * 6] = c["w1"][base + 32 * 6 + 16:base + 32 * 7]
        pre = y @ w1.T + b1
        m["hidden"], m["gate"] = hidden, gate = pre[:, :4 * C], pre[:, 4 * C:]
        m["h"] = h = f16r(hidden * gelu(gate))
        m["acc"] = acc = h @ c["w2"].T
        m["acc_abs"] = np.abs(h) @ np.abs(c["w2"]).T
        m["ff"] = ff = f16r(f16r(acc) + c["b2"] + tok)           # the epilogue's two roundings
        if tail == 0:
            m["out"] = ff
        else:
            x2 = ff
            if mutate == "proj_skip_residual":
                ch = frag_channels(5)
                x2 = ff.copy()
                x2[:, ch] = f16r(f16r(acc) + c["b2"])[:, ch]
            m["zpre"] = x2 @ c["wz"].T + c["bz"]
            m["out"] = f16r(f16r(m["zpre"]) + c["zres"])          # nn.Linear rounded, then the block's residual add
    return m


# ---- the conditions -----------------------------------------------------------------------------------------------------
def check_inputs(c, m):
    """Everything the kernel reads as f16 is an f16 value, the fp32 vectors hold what they are meant to hold, and the
    GroupNorm prologue turns x into the integer rows of stage A."""
    for k in ("a", "res", "zres", "wa", "wt", "w1", "w2", "wz"):
        if c.get(k) is not None:
            assert is_f16(c[k]), f"{k}: not f16 values"
    if c["gn"] is not None:
        st = c["gn"]["stat"]
        assert is_int(st[..., 0], 16) and np.isin(st[..., 1], (0.5, 1.0, 2.0)).all()
        assert (m["a_applied"] == c["a_applied"]).all() and is_int(c["a_applied"], 1024)
        assert len(np.unique(st.reshape(-1, 2), axis=0)) >= 30, "the (mean, rstd) pairs do not tell samples and groups apart"
    if c["stage"] in ("res", "dense"):
        assert np.isin(c["a_applied"], (-2, -1, 1, 2)).all() and (np.abs(c["wa"]) == 1).all()
    if c["res"] is not None:
        assert is_int(c["res"], 1400), f"residual of magnitude {np.abs(c['res']).max()}"


def check_tok(c, m):
    assert is_int(m["tok"]), "a token value is not an integer <= 2048"
    if c["exact_ln"]:
        assert (m["tok"] == c["T"]).all(), "stage A does not produce the two-valued rows"


def check_ln(c, m):
    """The rows are two-valued with 160 of each, y rounds to the integer s gamma + beta (+ pe), which is never 0, and an
    evaluation that is off by a relative 2^-13 still rounds to it."""
    s, T = c["s"], c["T"]
    assert (np.abs(s) == 1).all() and (s.sum(axis=1) == 0).all()
    v = np.abs(T - T.mean(axis=1, keepdims=True))
    assert (v == v[:, :1]).all() and np.isin(v[:, 0], (1, 2, 4)).all() and np.isin(T.mean(axis=1) / v[:, 0], (0, 16, -16, 64, -64)).all()
    yi = c["y_int"]
    assert is_int(yi, 6) and np.abs(yi).min() >= 1
    assert (m["y"] == yi).all(), "the float64 LayerNorm does not round to the integer"
    err = np.abs(m["y64"] - yi)
    assert (err <= 5.1e-6 * np.abs(c["ln_g"])).all()
    below = np.abs(yi) - np.abs(f16r(np.nextafter(np.abs(yi).astype(np.float16), np.float16(0))))    # f16 spacing towards 0
    assert (err + 2.0 ** -13 * np.abs(yi) < below / 2).all()
    if c["pe"] is not None:
        assert 1 <= np.abs(yi).min() and np.abs(yi).max() <= 6


def check_gemm_tail(c, m):
    assert is_int(m["out"], 1920)


def check_ff(c, m):
    """Gate pre-activations 0 or multiples of 16 (gelu = relu there), h an f16 value, GEMM2 a sum of integers far below 2^24,
    the accumulator and its sum with b2 and the residual integers <= 2048."""
    gate, hidden, h = m["gate"], m["hidden"], m["h"]
    assert (gate == 16 * np.rint(gate / 16)).all() and np.abs(gate).max() <= 2560 + 16
    assert (gelu(gate) == np.maximum(gate, 0)).all()
    if c["ff"][0] == "hid":
        assert is_int(hidden, 2047) and (np.abs(gate) == 16).all()
        assert (h == np.where(gate > 0, 16 * hidden, 0)).all() and is_f16(16 * hidden)
    else:
        assert (np.abs(hidden) == 1 / 16).all()
        assert is_int(h, 161) and (h == hidden * np.maximum(gate, 0)).all()
    assert is_int(m["acc"]) and m["acc_abs"].max() < 2 ** 24
    assert is_int(m["acc"] + c["b2"] + m["tok"]) and (m["ff"] == m["acc"] + c["b2"] + m["tok"]).all()
    return dict(max_hidden=float(np.abs(hidden).max()), max_h=float(np.abs(h).max()), max_ff=float(np.abs(m["ff"]).max()),
                max_terms=float(m["acc_abs"].max()), zero_gates=float((gate == 0).mean()))


def check_projection(c, m):
    assert is_int(m["zpre"]) and is_int(m["zpre"] + c["zres"]) and is_int(c["zres"], 16)
    assert (np.abs(c["wz"]).sum(axis=1) == 1).all() and (np.abs(c["wz"]).sum(axis=0) == 1).all()
    assert (m["out"] == m["ff"] @ c["wz"].T + c["bz"] + c["zres"]).all()


def att_expected(c, m):
    """What tail 4 has to return: unity — the row's own v; selection — v of frame (f + 1) % 5 of the same pixel."""
    b, hw = c["b"], c["hw"]
    v = m["qkv"][:, 2 * C:].reshape(b, F, hw, C)
    if c["att"] == "select":
        v = np.roll(v, -1, axis=1)
    return v.reshape(c["M"], C)


def check_att(c, m):
    b, hw = c["b"], c["hw"]
    assert is_int(m["qkv"])
    v = m["qkv"][:, 2 * C:].reshape(b, F, hw, C)
    tokf = m["tok"].reshape(b, F, hw, C)
    if c["att"] == "unity":
        assert (v == v[:, :1]).all() and (tokf == tokf[:, :1]).all() and is_int(v, 1920)
        assert len(np.unique(tokf[:, 0].reshape(b * hw, C), axis=0)) == b * hw, "pixels share a token row"
        gap = 0.0
    else:
        sc = m["scores"]                                         # [b][pixel][head][f][f']
        pi = (np.arange(F) + 1) % F
        sel = sc[..., np.arange(F), pi]
        rest = sc.copy()
        rest[..., np.arange(F), pi] = -np.inf
        gap = float((sel - rest.max(axis=-1)).min())
        assert gap >= AX.MIN_GAP, f"the selected score leads by {gap}"
        assert (v % 2 == 1).all() and np.abs(v).min() >= 1, "a v that is even (a true zero would carry the residue of the other frames)"
        assert (m["qkv"][:, :C] == SEL_T * np.roll(m["qkv"][:, C:2 * C].reshape(b, F, hw, C), -1, axis=1).reshape(-1, C)).all()
    assert (m["out"] == att_expected(c, m)).all(), "the float64 attention does not return the expected v rows"
    return gap


def check_case(c):
    """Every condition of the case, on the reference alone.  Returns a few figures for the host test to print."""
    m = c["ref"]
    info = {}
    check_inputs(c, m)
    check_tok(c, m)
    if not c["exact_ln"]:
        return info                      # A(i): tok bit for bit, the rest by close()
    check_ln(c, m)
    assert is_int(m["out"]), "an expected output is not an integer <= 2048"
    if c["tail"] in (1, 3):
        check_gemm_tail(c, m)
    elif c["tail"] == 4:
        info["gap"] = check_att(c, m)
    else:
        info.update(check_ff(c, m))
        if c["tail"] == 2:
            check_projection(c, m)
    info["max_out"] = float(np.abs(m["out"]).max())
    return info


# ---- the tolerance suites' usual operands, for the pass shares of the host test ---------------------------------------------
def randn_case(tail, M=320, res=True, pe_frames=0, rpf=64, gn_rows=0, form="chain", b=0, hw=0):
    """What tests/test_hip_rowff.py / tests/test_hip_motion_fused.py feed the kernels at C = 320: f16-rounded normal rows,
    weights * K^-0.5, gamma = 1 + 0.2 N, small biases."""
    g = np.random.default_rng([99, tail, M, pe_frames, gn_rows])
    n = lambda *shape: g.standard_normal(shape)
    c = dict(DEFAULTS, name="randn", form=form, tail=tail, M=M, rpf=rpf if (pe_frames or tail == 4) else 1, pe_frames=pe_frames,
             frames=F if tail == 4 else max(pe_frames, 1), b=b, hw=hw, exact_ln=False, gn=None, res=None)
    c.update(ln_g=1.0 + 0.2 * n(C), ln_b=0.1 * n(C), pe=0.3 * n(pe_frames, C) if pe_frames else None)
    if form == "ff":
        c["a"] = f16r(n(M, C) * 1.5 + 0.3)
    else:
        c.update(a=f16r(n(M, C)), wa=f16r(n(C, C) * C ** -0.5), ba=0.1 * n(C), res=f16r(n(M, C) * 1.5) if res else None)
    if gn_rows:
        x = f16r(n(M, C) * 2.0 + 0.5)
        nsamp = -(-M // gn_rows)
        stat = np.zeros((nsamp, GN_GROUPS, 2))
        for s_ in range(nsamp):
            xs = x[s_ * gn_rows:(s_ + 1) * gn_rows].reshape(-1, GN_GROUPS, C // GN_GROUPS)
            stat[s_, :, 0] = xs.mean(axis=(0, 2))
            stat[s_, :, 1] = 1.0 / np.sqrt(xs.var(axis=(0, 2)) + 1e-6)
        c.update(a=x, res=None, gn=dict(stat=stat, gamma=1.0 + 0.2 * n(C), beta=0.3 * n(C), rows=gn_rows))
    if tail in (1, 3, 4):
        c["wt"] = f16r(n((3 if tail == 4 else tail) * C, C) * C ** -0.5)
    else:
        c.update(w1=f16r(n(8 * C, C) * C ** -0.5), b1=0.1 * n(8 * C), w2=f16r(n(C, 4 * C) * (4 * C) ** -0.5), b2=0.1 * n(C))
        if tail == 2:
            c.update(wz=f16r(n(C, C) * C ** -0.5), bz=0.1 * n(C), zres=f16r(n(M, C)))
    return c
