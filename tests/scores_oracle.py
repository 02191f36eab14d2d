"""The figures of rcdms_amd.scores restated for the tests and for tools/mint_scores_golden.py.

  label counts     `label_state`: the int64 state [n | tp, fp, fn per class | H[t][e]] by Python-int arithmetic over boolean
                   arrays; `rule=` swaps in one plausible mistake (">=" for ">", a NaN predicting 1, a label read as `== 1`).
                   `figures`: every figure of the state as the correctly rounded float64 of an exact Fraction — independent of
                   rcdms_amd.scores.label_scores, which works in float64.  `mean_tolerance`: what a float64 mean of k values in
                   [0, 1] may be off by, summed in any order: k 2^-53 (k - 1 additions and a division).
  Inception Score  `evaluate`: csrc/scores_core.h operation for operation.  Per row m, s, log s, h with the sums over classes
                   as 64 strided partial sums and a tree (`lane_sum`); per split P_c and the sum of h in chunks of 256 positions,
                   ascending; g(P / n_k) over the classes through 256 strided partial sums and a tree; KL = Hs / n_k - G.  No
                   ndarray.sum in any reduction.  exp and log are numpy's: the device's and libm's may differ in the last
                   places, which `bound` allows for.  `two_pass`: the definition, mean_rows KL(p_row || p_mean), in plain numpy.
  bound            `bound`: an a-priori absolute bound B on KL_k of ANY evaluation that follows the rules, given that exp and
                   log err by at most ULPS units in the last place per call.  ULPS = 2 is an ASSUMPTION: no accuracy figure
                   for the device's float64 exp / log is found in the ROCm documentation that ships with the toolkit; the
                   C standard library's are below 1.  With u = 2^-53, eps = 2 u ULPS (relative error of one exp / log),
                   g(j) = j u / (1 - j u) (a chain of j additions), D = the largest max - min of a row, L = ceil(C / 64) + 6:
                     d = z - m       exact when the two float32 exponents are within 29, else one rounding: |dd| <= u D;
                     e = exp(d)      relative eta_e = eps + 1.01 u D;       s = sum e (all >= 0): relative eta_e + g(L);
                     log s           in [0, ln C]: absolute a_ls = 1.01 (eta_e + g(L)) + eps ln C;
                     logp = d - logs absolute a_lp = a_ls + u (2 D + ln C)          (dd, and the rounding of the difference);
                     p = exp(logp)   relative eta_p = 1.01 a_lp + eps;
                     h = sum p logp  (all <= 0, |h| <= ln C, sum p = 1): absolute a_h = ln C (eta_p + u + g(L)) + a_lp;
                     Hs / n_k        chains of Ls = min(n_k, 256) + chunks additions, a division: a_h + ln C (g(Ls) + u);
                     pbar = P / n_k  relative eta_pb = eta_p + g(Ls) + u;
                     G = sum g(pbar) d(p log p) = (log p + 1) dp, sum pbar |log pbar| <= ln C, the log and the product, the
                                     chain of LG = ceil(C / 256) + 8: (ln C + 1) eta_pb + ln C (eps + u) + g(LG) ln C;
                     KL              the last difference: u ln C.
                   B = 1.01 x the sum (second-order terms) + 1e-300 (a pbar that underflows).  Nothing in it comes from a
                   kernel's output.
  cases            ISC_CASES / LABEL_CASES, the goldens tools/mint_scores_golden.py writes (tests/golden/isc_*.npz with KL at
                   60 digits, tests/golden/scores_*.npz with the integer states)."""
import math
import os
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ULPS = 2.0                      # assumed: see `bound` above
WAVE, LANES, CHUNK = 64, 256, 256
LABEL_ROWS = 256                # sc::LABEL_ROWS: rows per block of the count launch, what its workspace is sized by
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ------------------------------------------------------------------------------------------------ label counts
LABEL_SHAPES = [(c, n) for c in (1, 7, 9, 64) for n in (1, 63, 64, 65, 255, 256, 257, 1000)]
LABEL_CASES = {
    "c1_n5": "C 1, N 5: the smallest state",
    "c7_n257": "C 7, N 257: a never-present class, empty rows, logits at the threshold, NaN, labels 0 / 1 / 255",
    "c9_n1000": "C 9, N 1000: per-class thresholds",
    "c64_n300": "C 64, N 300: the widest state",
}


def state_len(C):
    return 1 + 3 * C + (C + 1) * (C + 1)


def label_inputs(C, n, seed, thresholds=False):
    """Logits on a grid of 1/4 (exact in float16) with the edge cases planted, labels in {0, 1, 255}.  Class C - 1 is never
    present (for C > 1); every fifth row is all-negative with no labels.  -> (float32 logits, uint8 labels, float32 thresholds or
    None).  Integer draws only: the same arrays on every machine."""
    rng = np.random.RandomState(seed)
    thr = (rng.randint(-4, 5, C) / 4.0).astype(np.float32) if thresholds else None
    z = (rng.randint(-12, 13, (n, C)) / 4.0).astype(np.float32)
    y = rng.randint(0, 3, (n, C)).astype(np.uint8)
    y[y == 2] = 255
    y[rng.randint(0, 2, (n, C)) == 0] = 0
    t = np.zeros(C, np.float32) if thr is None else thr
    at = rng.randint(0, 6, (n, C))
    z = np.where(at == 0, t[None, :], z).astype(np.float32)          # exactly at the threshold: predicts 0
    z[at == 1] = np.nan                                              # predicts 0
    if C > 1:
        y[:, C - 1] = 0
    z[::5] = t[None, :] - np.float32(1.5)
    y[::5] = 0
    return z, y, thr


def label_state(logits, labels, thresholds=None, rule=None):
    """int64 state by Python-int arithmetic.  rule: None (the project's), or one mistake: "ge", "nan1", "label1"."""
    z = np.asarray(logits).astype(np.float32)
    n, C = z.shape
    t = np.zeros(C, np.float32) if thresholds is None else np.asarray(thresholds, np.float32)
    with np.errstate(invalid="ignore"):
        pred = z >= t[None, :] if rule == "ge" else z > t[None, :]
    if rule == "nan1":
        pred = pred | np.isnan(z)
    lab = np.asarray(labels) == 1 if rule == "label1" else np.asarray(labels) != 0
    state = [0] * state_len(C)
    state[0] = n
    for c in range(C):
        state[1 + 3 * c + 0] = int(np.count_nonzero(pred[:, c] & lab[:, c]))
        state[1 + 3 * c + 1] = int(np.count_nonzero(pred[:, c] & ~lab[:, c]))
        state[1 + 3 * c + 2] = int(np.count_nonzero(~pred[:, c] & lab[:, c]))
    for r in range(n):
        tt = int(np.count_nonzero(pred[r] & lab[r]))
        e = int(np.count_nonzero(pred[r] != lab[r]))
        state[1 + 3 * C + tt * (C + 1) + e] += 1
    return np.array(state, np.int64)


def predictions(logits, thresholds=None):
    z = np.asarray(logits).astype(np.float32)
    t = np.zeros(z.shape[1], np.float32) if thresholds is None else np.asarray(thresholds, np.float32)
    with np.errstate(invalid="ignore"):
        return (z > t[None, :]).astype(np.int64)


def figures(state, C, zero_division=0):
    """Every figure as float(Fraction): correctly rounded from the exact value."""
    v = [int(x) for x in state]
    n = v[0]
    tp, fp, fn = (v[1 + k:1 + 3 * C:3] for k in range(3))
    H = [v[1 + 3 * C + t * (C + 1):1 + 3 * C + (t + 1) * (C + 1)] for t in range(C + 1)]
    zd = Fraction(zero_division)
    div = lambda a, b: zd if b == 0 else Fraction(a, b)
    f1 = [div(2 * tp[c], 2 * tp[c] + fp[c] + fn[c]) for c in range(C)]
    sup = [tp[c] + fn[c] for c in range(C)]
    out = {
        "frame_accuracy": Fraction(sum(H[t][0] for t in range(C + 1)), n),
        "f1_micro": div(2 * sum(tp), 2 * sum(tp) + sum(fp) + sum(fn)),
        "f1_macro": sum(f1) / C,
        "f1_weighted": zd if sum(sup) == 0 else sum(s * f for s, f in zip(sup, f1)) / sum(sup),
        "f1_samples": sum(H[t][e] * div(2 * t, 2 * t + e) for t in range(C + 1) for e in range(C + 1)) / n,
        "hamming": Fraction(sum(fp) + sum(fn), n * C),
    }
    out = {k: float(x) for k, x in out.items()}
    out["precision"] = np.array([float(div(tp[c], tp[c] + fp[c])) for c in range(C)])
    out["recall"] = np.array([float(div(tp[c], tp[c] + fn[c])) for c in range(C)])
    out["f1"] = np.array([float(x) for x in f1])
    out["support"] = np.array(sup, np.int64)
    return out


def mean_tolerance(k):
    return k * U


def load_labels(name):
    with np.load(os.path.join(GOLDEN, f"scores_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ Inception Score
ISC_CLASSES, ISC_SPLITS = (2, 7, 1000, 1008), (1, 3, 10)
GRID32, GRID16 = 12, 8           # logits are integers / 2^grid: below 8 in magnitude (float32), below 8 and float16-exact


def isc_rows(splits):
    return sorted({splits, 23, 257})


# name -> (C, N, splits, variant): the full grid, then the variants
ISC_CASES = {f"c{c}_n{n}_s{s}": (c, n, s, None) for c in ISC_CLASSES for s in ISC_SPLITS for n in isc_rows(s)}
ISC_CASES.update({
    "f16_c100_n23_s3": (100, 23, 3, "f16"),              # float16-representable logits
    "span80_c64_n23_s3": (64, 23, 3, "span80"),          # logits across +-80
    "order_c7_n257_s10": (7, 257, 10, "order"),          # rows through shuffled_order(257, 5)
    "equal_c7_n23_s3": (7, 23, 3, "equal"),              # identical rows: KL is 0
})
ORDER_SEED = 5


def isc_logits(C, N, variant=None):
    """The logits of a case.  Integer draws scaled by a power of two: the same float32 values on every machine.  The grid cases
    share one matrix per (C, N), whatever the splits."""
    rng = np.random.RandomState(1000 * C + N)
    if variant == "f16":
        z = rng.randint(-2047, 2048, (N, C)) / 2.0 ** GRID16
        assert np.array_equal(z.astype(np.float16).astype(np.float64), z)
    elif variant == "span80":
        z = rng.randint(-80 * 1024, 80 * 1024 + 1, (N, C)) / 1024.0
    elif variant == "equal":
        z = np.tile(rng.randint(-32767, 32768, (1, C)) / 2.0 ** GRID32, (N, 1))
    else:
        z = rng.randint(-32767, 32768, (N, C)) / 2.0 ** GRID32
        z[np.arange(N), rng.randint(0, C, N)] += rng.randint(0, 4, N) * 2.0         # some rows confident, some flat
    out = z.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), z)
    return out


def isc_order(name):
    C, N, splits, variant = ISC_CASES[name]
    return np.random.RandomState(ORDER_SEED).permutation(N).astype(np.int32) if variant == "order" else None


def load_isc(name):
    """-> dict: logits (regenerated, and checked against the file where the file carries them), order, splits, kl_digits
    (strings, 50 digits), bound, model."""
    C, N, splits, variant = ISC_CASES[name]
    z = isc_logits(C, N, variant)
    with np.load(os.path.join(GOLDEN, f"isc_c{C}.npz")) as f:
        if f"{name}/logits" in f.files:
            assert np.array_equal(f[f"{name}/logits"], z), f"{name}: the generator no longer gives the file's logits"
        return {"logits": z, "order": isc_order(name), "splits": splits, "kl_digits": f[f"{name}/kl_digits"],
                "bound": f[f"{name}/bound"], "model": f[f"{name}/model"]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def lane_sum(terms, lanes):
    """(R, K) -> (R,): `lanes` partial sums, lane l adding columns l, l + lanes, ... in ascending order from +0.0, then the tree
    part[l] += part[l + s], s = lanes / 2 .. 1."""
    R, K = terms.shape
    steps = -(-K // lanes)
    pad = np.zeros((R, steps * lanes))
    pad[:, :K] = terms
    pad = pad.reshape(R, steps, lanes)
    part = np.zeros((R, lanes))
    for k in range(steps):
        part = part + pad[:, k]
    s = lanes // 2
    while s:
        part = part[:, :s] + part[:, s:2 * s]
        s //= 2
    return part[:, 0]


def row_stats(z):
    """z (N, C) float64 -> m, logs, h (N,) and p (N, C), as sc's row rules form them."""
    m = z.max(axis=1)                                     # exact, whatever the order
    d = z - m[:, None]
    logs = np.log(lane_sum(np.exp(d), WAVE))
    lp = d - logs[:, None]
    p = np.exp(lp)
    return m, logs, lane_sum(p * lp, WAVE), p


def split_bounds(N, splits):
    return [(k * N // splits, (k + 1) * N // splits) for k in range(splits)]


def chunks(rows):
    return -(-rows // CHUNK)


def evaluate(logits, splits, order=None):
    """-> KL_k (splits,) float64 by the model."""
    z = np.asarray(logits).astype(np.float64)
    N, C = z.shape
    _, _, h, p = row_stats(z)
    rows = np.arange(N) if order is None else np.asarray(order)
    out = np.empty(splits)
    for k, (b0, b1) in enumerate(split_bounds(N, splits)):
        nk = float(b1 - b0)
        P, H = np.zeros(C), 0.0
        for p0 in range(b0, b1, CHUNK):
            Pc, Hc = np.zeros(C), 0.0
            for pos in range(p0, min(p0 + CHUNK, b1)):
                Pc = Pc + p[rows[pos]]
                Hc = Hc + h[rows[pos]]
            P, H = P + Pc, H + Hc
        pbar = P / nk
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(pbar == 0.0, 0.0, pbar * np.log(pbar))
        out[k] = H / nk - lane_sum(g[None, :], LANES)[0]
    return out


def two_pass(logits, splits, order=None):
    """The definition: per split, mean over rows of sum_c p (log p - log pbar), p = softmax; plain numpy."""
    z = np.asarray(logits).astype(np.float64)
    z = z if order is None else z[np.asarray(order)]
    lp = z - z.max(axis=1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(axis=1, keepdims=True))
    p = np.exp(lp)
    out = []
    for b0, b1 in split_bounds(z.shape[0], splits):
        pb = p[b0:b1].mean(axis=0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(p[b0:b1] == 0.0, 0.0, p[b0:b1] * (lp[b0:b1] - np.log(pb)))
        out.append(t.sum(axis=1).mean())
    return np.array(out)


def bound(logits, splits):
    """B per split (the docstring has the derivation): a function of the inputs and ULPS alone."""
    z = np.asarray(logits).astype(np.float64)
    N, C = z.shape
    D = float((z.max(axis=1) - z.min(axis=1)).max())
    assert D * U < 2.0 ** -20, "the bound is first-order in u D"
    lnC, eps = math.log(C), 2.0 * U * ULPS
    g = lambda j: j * U / (1.0 - j * U)
    L = -(-C // WAVE) + 6
    eta_e = eps + 1.01 * U * D
    a_ls = 1.01 * (eta_e + g(L)) + eps * lnC
    a_lp = a_ls + U * (2.0 * D + lnC)
    eta_p = 1.01 * a_lp + eps
    a_h = lnC * (eta_p + U + g(L)) + a_lp
    LG = -(-C // LANES) + 8
    out = []
    for b0, b1 in split_bounds(N, splits):
        nk = b1 - b0
        Ls = min(nk, CHUNK) + chunks(nk)
        eta_pb = eta_p + g(Ls) + U
        out.append(1.01 * (a_h + lnC * (g(Ls) + U) + (lnC + 1.0) * eta_pb + lnC * (eps + U) + g(LG) * lnC + U * lnC) + 1e-300)
    return np.array(out)


def one_hot_rows(C, N, margin):
    """Row r: `margin` at class r mod C, 0 elsewhere."""
    z = np.zeros((N, C), np.float32)
    z[np.arange(N), np.arange(N) % C] = margin
    return z


def one_hot_kl(C, margin, mp):
    """KL of a split whose rows cycle through all C classes equally often, at mpmath precision: the mean is uniform, so
    KL = p1 log p1 + (C - 1) p0 log p0 + log C with p1 = e^L / (e^L + C - 1), p0 = 1 / (e^L + C - 1)."""
    e = mp.exp(mp.mpf(margin))
    p1, p0 = e / (e + C - 1), 1 / (e + C - 1)
    return p1 * mp.log(p1) + (C - 1) * p0 * mp.log(p0) + mp.log(C)


def isc(kl):
    """(mean, std, scores) of exp(kl) as rcdms_amd.scores forms them: in order, population spread."""
    scores = [math.exp(float(v)) for v in kl]
    total = 0.0
    for v in scores:
        total = total + v
    mean = total / len(scores)
    sq = 0.0
    for v in scores:
        sq = sq + (v - mean) * (v - mean)
    return mean, math.sqrt(sq / len(scores)), tuple(scores)
