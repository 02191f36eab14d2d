"""Inputs on which attention has ONE right answer in f16, and a numpy model of the kernels' softmax: shared by
tests/test_attn_exact_host.py (CPU: the assertions reject what they are for) and tests/test_hip_attn_exact.py (GPU: the
kernels satisfy them).  Needs numpy only.

Two constructions:

  unity       V[k][h*d + j] = c_j for every key, c_j = (-1)^j 2^((j mod 5) - 2): softmax weights sum to one, so out == c_j
              whatever Q and K are.  Exact in f16 when the row sum that normalises is the sum of the probabilities the P V
              product multiplied (a power-of-two scale commutes with every rounding), off by one f16 ulp under most rows when
              it is the sum of the unrounded ones (round-toward-zero loses a relative ~3e-4 of every row).
  selection   K rows are pairwise distinct +-1 vectors, Q_i = t K_pi(i), t = ceil(12 sqrt d): the selected key's scaled score
              is ahead of every other key's by >= 2 t / sqrt(d) >= 24 (one differing coordinate), every other probability is
              below 2^-24 / 2^6 and rounds (toward zero) to 0 in f16, so out[i] == V[pi(i)] bit for bit.  V rows are
              +-[0.25, 4): what fp32 residue a kernel may carry (no P rounding in the temporal kernel, the flash kernels'
              rescale across key tiles) is <= Lk * e^-24 * 4 < 2e-7, far below half an f16 ulp of 0.25 (6e-5)."""
import math

import numpy as np

LOG2E = 1.4426950408889634
GAINS = (1, 3)
MIN_GAP = 24.0

# ---- shapes of the unity tests: one table per entry point, read by the host and the GPU test alike -------------------
BATCH, HEADS = 2, 2
FLASH_D = (8, 16, 24, 32, 40, 48, 64, 80, 88, 104, 112, 120, 128, 152, 160)
FLASH_LK = (85, 320)
FLASH_LQ = 130
FALLBACK_D = (32, 160)                  # no spare column in the padded head dim: the row sum comes off the VALU
FALLBACK_LK = (1, 63, 64, 65, 1000)
FALLBACK_LQ = (1, 33)
MASKED_D = (32, 40, 64, 160)
MASKED_L = (97, 150)
MASKED_MODES = ("causal", "pad", "causal+pad")
XATTN_D = (8, 16, 32, 40, 48, 80, 96, 160)
XATTN_LK = (1, 32, 33, 85, 91, 96)
XATTN_LQ = (33, 300)
WIDE_D = (192, 256, 320, 384, 448, 512)
WIDE_LK = (16, 200, 1000)
WIDE_LQ = 130
TEMPORAL_D = (8, 40, 160)
TEMPORAL_FRAMES = (1, 2, 3, 4, 5, 6, 7, 8)
TEMPORAL_PIXELS = 33


def unity_cases():
    """(entry, d, Lq, Lk, mode) of every unity launch; mode is None or one of MASKED_MODES.  Temporal: Lq = Lk = frames, one
    attention problem per (sample, pixel)."""
    out = []
    out += [("flash", d, FLASH_LQ, lk, None) for d in FLASH_D for lk in FLASH_LK]
    out += [("flash", d, lq, lk, None) for d in FALLBACK_D for lk in FALLBACK_LK for lq in FALLBACK_LQ]
    out += [("masked", d, L, L, m) for d in MASKED_D for L in MASKED_L for m in MASKED_MODES]
    out += [("xattn", d, lq, lk, None) for d in XATTN_D for lk in XATTN_LK for lq in XATTN_LQ]
    out += [("wide", d, WIDE_LQ, lk, None) for d in WIDE_D for lk in WIDE_LK]
    out += [("temporal", d, f, f, None) for d in TEMPORAL_D for f in TEMPORAL_FRAMES]
    return out


def falls_back(entry, d):
    """The launches whose kernel has no ones-column to take the row sum from (flash_attn_kernel / xattn_kernel at d = 32
    and d = 160): where an unrounded row sum shows."""
    return entry in ("flash", "masked", "xattn") and d in FALLBACK_D


def _seed(entry, d, Lq, Lk, mode, gain):
    names = {"flash": 1, "masked": 2, "xattn": 3, "wide": 4, "temporal": 5}
    modes = {None: 0, "causal": 1, "pad": 2, "causal+pad": 3}
    return np.random.default_rng([names[entry], d, Lq, Lk, modes[mode], int(gain)])


def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def is_f16_exact(x):
    x = np.asarray(x)
    with np.errstate(over="ignore"):
        return bool(np.all(np.isfinite(x)) and np.array_equal(x.astype(np.float16).astype(x.dtype), x))


# ---- unity ------------------------------------------------------------------------------------------------------------
def unity_column(d):
    """c_j, j < d: powers of two that differ from column to column (a column mix-up shows), signs alternating."""
    j = np.arange(d)
    return ((-1.0) ** j * 2.0 ** ((j % 5) - 2)).astype(np.float32)


def unity_v(rows, heads, d):
    """V rows [rows][heads * d]: column j of every head holds c_j in every row."""
    return np.broadcast_to(np.tile(unity_column(d), heads), (rows, heads * d)).copy()


def unity_qk(entry, d, Lq, Lk, mode, gain, batch=BATCH, heads=HEADS):
    """Q [batch][Lq][heads*d] = f16(gain * N(0, 1)), K [batch][Lk][heads*d] = f16(N(0, 1)), float32 holding f16 values: scaled
    scores ~ gain * N(0, 1)."""
    g = _seed(entry, d, Lq, Lk, mode, gain)
    q = f16(gain * g.standard_normal((batch, Lq, heads * d))).astype(np.float32)
    k = f16(g.standard_normal((batch, Lk, heads * d))).astype(np.float32)
    return q, k


def unity_mask(d, L, mode, batch=BATCH):
    """(key_valid [batch][L] uint8 or None, causal).  Padding hides a random half of the keys of every batch entry — key 0
    included when the mask is not causal, whole runs of them — and every query keeps at least one visible key."""
    causal = "causal" in mode
    valid = None
    if "pad" in mode:
        g = np.random.default_rng([7, d, L, int(causal)])
        valid = (g.random((batch, L)) < 0.5).astype(np.uint8)
        valid[0, 40:75] = 0                   # a run across the 64-key tile boundary
        if causal:
            valid[:, 0] = 1                   # query 0 sees key 0 only
        else:
            valid[:, 0] = 0
            valid[1, :66] = 0                 # the whole first key tile of one batch entry
            valid[:, L - 3] = 1
    return valid, causal


def visible(valid_b, causal, Lq, Lk):
    """[Lq][Lk] bool: what rcdm.h says a query sees (key_valid of ONE batch entry, or None)."""
    vis = np.ones((Lq, Lk), dtype=bool)
    if valid_b is not None:
        vis &= (np.asarray(valid_b) != 0)[None, :]
    if causal:
        vis &= np.arange(Lk)[None, :] <= np.arange(Lq)[:, None]
    return vis


def unity_mismatches(out, heads, d):
    """out [rows][heads * d] float16 -> number of elements whose BITS differ from c_j's."""
    out = np.asarray(out)
    assert out.dtype == np.float16 and out.ndim == 2 and out.shape[1] == heads * d, (out.dtype, out.shape)
    want = np.tile(unity_column(d), heads).astype(np.float16)
    return int((out.view(np.uint16) != want.view(np.uint16)[None, :]).sum())


# ---- the kernels' softmax, in numpy ------------------------------------------------------------------------------------
def rtz_f16(p):
    """fp32 >= 0 -> f16 rounded toward zero (v_cvt_pkrtz_f16_f32), subnormals kept."""
    p = np.asarray(p, dtype=np.float32)
    h = p.astype(np.float16)                                  # round to nearest even
    up = h.astype(np.float32) > p
    return np.where(up, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def model_attention(q, k, v, scale, consistent, vis=None):
    """One head: q [Lq][d], k [Lk][d], v [Lk][d] (float32 holding f16 values) -> (out [Lq][d] float16, rounded P [Lq][Lk]).
    p = exp2(s c - max) in fp32 rounded toward zero to f16; P V and the row sum accumulated key by key in fp32;
    consistent: divided by the sum of the ROUNDED p (what the ones-column of V gives, and attn_wide.hip's VALU sum), else
    by the sum of the unrounded p; the quotient rounded to nearest f16.  A query that sees nothing gives a zero row."""
    Lq, Lk = q.shape[0], k.shape[0]
    c = np.float32(scale * LOG2E)
    s = (q.astype(np.float64) @ k.astype(np.float64).T).astype(np.float32) * c
    if vis is not None:
        s = np.where(vis, s, np.float32(-np.inf))
    m = s.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, np.float32(0))
    p = np.exp2((s - m).astype(np.float32)).astype(np.float32)
    pr = rtz_f16(p)
    prf = pr.astype(np.float32)
    num = np.zeros((Lq, v.shape[1]), dtype=np.float32)
    l_r = np.zeros(Lq, dtype=np.float32)
    l_u = np.zeros(Lq, dtype=np.float32)
    for key in range(Lk):
        num += prf[:, key, None] * v[key][None, :]
        l_r += prf[:, key]
        l_u += p[:, key]
    l = l_r if consistent else l_u
    with np.errstate(divide="ignore"):
        inv = np.where(l > 0, np.float32(1) / l, np.float32(0)).astype(np.float32)
    return (num * inv[:, None]).astype(np.float16), pr


def model_rows(q, k, v, heads, d, consistent, valid=None, causal=False):
    """The row layout of the C ABI: q [batch][Lq][heads*d], k, v [batch][Lk][heads*d] -> out [batch*Lq][heads*d] float16 and
    the rounded probabilities of every (batch, head), flattened."""
    batch, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    out = np.empty((batch, Lq, heads * d), dtype=np.float16)
    ps = []
    for b in range(batch):
        vis = None if valid is None and not causal else visible(None if valid is None else valid[b], causal, Lq, Lk)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            o, pr = model_attention(q[b][:, sl], k[b][:, sl], v[b][:, sl], d ** -0.5, consistent, vis)
            out[b][:, sl] = o
            ps.append(pr[vis] if vis is not None else pr.reshape(-1))
    return out.reshape(batch * Lq, heads * d), np.concatenate(ps)


# ---- selection ---------------------------------------------------------------------------------------------------------
def sel_t(d):
    return math.ceil(12 * math.sqrt(d))


def distinct_pm1(g, n, d):
    """n pairwise distinct +-1 rows of length d (n <= 2^d)."""
    assert n <= 2 ** min(d, 30), (n, d)
    while True:
        bits = g.integers(0, 2, size=(n, d))
        if len(np.unique(bits, axis=0)) == n:
            return (2.0 * bits - 1.0).astype(np.float32)


def sel_values(g, shape):
    """V: +-f16(U[0.25, 4)), float32."""
    return (f16(g.uniform(0.25, 4.0, size=shape)).astype(np.float32) * g.choice(np.float32([-1, 1]), size=shape)).astype(np.float32)


def must_hit(Lk):
    """Keys every selection test selects at least once: 0, Lk - 1 and both sides of every 32-key (hence 64-key) boundary."""
    ks = {0, Lk - 1}
    for b in range(32, Lk, 32):
        ks |= {b - 1, b}
    return sorted(ks)


def selection_inputs(seed, batch, heads, Lq, Lk, d):
    """q [batch][Lq][heads*d], k, v [batch][Lk][heads*d] (float32 holding f16 values), pi [batch][heads][Lq]."""
    g = np.random.default_rng([11] + list(seed))
    C = heads * d
    q = np.empty((batch, Lq, C), dtype=np.float32)
    k = np.empty((batch, Lk, C), dtype=np.float32)
    v = sel_values(g, (batch, Lk, C))
    pi = np.empty((batch, heads, Lq), dtype=np.int64)
    hit = must_hit(Lk)
    assert Lq >= len(hit), "too few queries to select every boundary key"
    for b in range(batch):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            kk = distinct_pm1(g, Lk, d)
            p = g.integers(0, Lk, size=Lq)
            p[g.permutation(Lq)[:len(hit)]] = hit
            k[b][:, sl] = kk
            q[b][:, sl] = sel_t(d) * kk[p]
            pi[b, h] = p
    return q, k, v, pi


def masked_selection_inputs(seed, batch, heads, L, d, pad, causal):
    """Self-attention shapes (Lq = Lk = L) under a mask.  pi(i) is a key query i sees; wherever the mask leaves room an
    INVISIBLE DECOY is planted as well: an exact copy of K_pi(i) with another V row, at a padded position and, when the mask
    is causal, behind the query.  A kernel that drops the mask returns the mean of the two V rows.
    Returns q, k, v, key_valid ([batch][L] uint8 or None), pi, planted ([batch][heads][L] bool: query i has a decoy)."""
    g = np.random.default_rng([13, int(pad), int(causal)] + list(seed))
    C = heads * d
    valid = None
    if pad:
        valid = np.ones((batch, L), dtype=np.uint8)
        for b in range(batch):
            valid[b, 20 + 7 * b:L - 6] = g.random(L - 6 - 20 - 7 * b) < 0.35     # most of the middle padded out
            valid[b, 33] = 0
    q = np.empty((batch, L, C), dtype=np.float32)
    k = np.empty((batch, L, C), dtype=np.float32)
    v = sel_values(g, (batch, L, C))
    pi = np.empty((batch, heads, L), dtype=np.int64)
    planted = np.zeros((batch, heads, L), dtype=bool)
    for b in range(batch):
        vis = visible(None if valid is None else valid[b], causal, L, L)
        # decoy positions: every padded key; without padding, every third key of the upper half (invisible to the queries in
        # front of it only)
        decoys = np.flatnonzero(valid[b] == 0) if pad else np.arange(L // 2, L, 3)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            kk = distinct_pm1(g, L, d)
            src = {}                                          # decoy position j -> the key it copies
            for j in decoys:
                cand = [c for c in range(j) if c not in src and (valid is None or valid[b, c])]
                if cand:
                    src[int(j)] = int(g.choice(cand))
                    kk[j] = kk[src[int(j)]]
            copies = {}
            for j, c in src.items():
                copies.setdefault(c, []).append(j)
            p = np.empty(L, dtype=np.int64)
            free = list(g.permutation(L))
            want = [x for x in must_hit(L)]
            for i in range(L):
                # admissible: visible, not itself a decoy, and no copy of it visible to this query
                adm = [c for c in np.flatnonzero(vis[i]) if c not in src and not any(vis[i, j] for j in copies.get(int(c), ()))]
                assert adm, "a query with nothing to select"
                strong = [c for c in adm if any((not causal) or j > i for j in copies.get(int(c), ()))]
                forced = [c for c in adm if c in want]
                if forced and g.random() < 0.5:
                    c = int(g.choice(forced))
                    want.remove(c)
                elif strong:
                    c = int(g.choice(strong))
                else:
                    c = int(g.choice(adm))
                p[i] = c
                planted[b, h, i] = bool(copies.get(c))
            k[b][:, sl] = kk
            q[b][:, sl] = sel_t(d) * kk[p]
            pi[b, h] = p
    return q, k, v, valid, pi, planted


def selection_gap(q, k, heads, d, pi, valid=None, causal=False):
    """Smallest lead, in float64, of the selected key's scaled score over every other VISIBLE key's, over all queries."""
    batch, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    gap = np.inf
    for b in range(batch):
        vis = visible(None if valid is None else valid[b], causal, Lq, Lk)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = (q[b][:, sl].astype(np.float64) @ k[b][:, sl].astype(np.float64).T) * d ** -0.5
            rows = np.arange(Lq)
            assert vis[rows, pi[b, h]].all(), "a selected key is not visible"
            sel = s[rows, pi[b, h]]
            s = np.where(vis, s, -np.inf)
            s[rows, pi[b, h]] = -np.inf
            if Lk > 1:
                gap = min(gap, float((sel - s.max(axis=1)).min()))
    return gap


def selection_expected(v, heads, d, pi):
    """out [batch*Lq][heads*d] float16 = V[pi(i)] per head."""
    batch, Lq = pi.shape[0], pi.shape[2]
    out = np.empty((batch, Lq, heads * d), dtype=np.float16)
    for b in range(batch):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            out[b][:, sl] = v[b][pi[b, h]][:, sl].astype(np.float16)
    return out.reshape(batch * Lq, heads * d)


# (d, Lq, Lk): one ragged and one production-like shape per head-dim family of each entry point
SEL_FLASH = [(32, 130, 333), (40, 130, 333), (104, 130, 333), (160, 130, 333),     # ragged; d = 40 with Lk >= 256: the MSUB kernel
             (32, 256, 256), (40, 256, 256), (104, 257, 257), (160, 256, 256)]     # 16x16 latents, the CLIP vision tower's 257 tokens
SEL_XATTN = [(40, 300, 85), (160, 64, 96)]
SEL_WIDE = [(192, 130, 203), (512, 256, 1024)]                                     # the VAE mid block at 32x32 latents
SEL_TEMPORAL = [(8, 3), (40, 5), (160, 8)]                                         # (d, frames)
SEL_MASKED = [(64, 97, True, True), (40, 150, True, False), (160, 97, False, True), (32, 150, True, True)]   # (d, L, pad, causal)


def sel_case(entry, d, Lq, Lk):
    """q, k, v, pi of one unmasked selection launch of `entry` (flash / xattn / wide)."""
    return selection_inputs(({"flash": 1, "xattn": 3, "wide": 4}[entry], d, Lq, Lk), BATCH, HEADS, Lq, Lk, d)


def sel_temporal_case(d, frames):
    """The same in the temporal kernel's terms: one attention problem of `frames` keys per (sample, pixel)."""
    return selection_inputs((5, d, frames), BATCH * TEMPORAL_PIXELS, HEADS, frames, frames, d)


def sel_masked_case(d, L, pad, causal):
    return masked_selection_inputs((d, L), BATCH, HEADS, L, d, pad, causal)


# ---- temporal layout ---------------------------------------------------------------------------------------------------
def temporal_rows(x, b, frames, pixels):
    """[b*pixels][frames][C] attention problems -> the kernel's rows [(b frames) pixels][C] ("(b d) f c -> (b f) d c")."""
    C = x.shape[-1]
    return x.reshape(b, pixels, frames, C).transpose(0, 2, 1, 3).reshape(b * frames * pixels, C)
