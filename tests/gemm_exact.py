"""Exact-answer cases for the implicit-GEMM family (igemm.hip, igemm16.hip, igemm8.hip, wino.hip and the split-K reduce
passes): integer operands whose answer has to come back bit for bit on every tile variant, split count and slab format.

Why it is exact.  Activations are drawn from {+-1, +-2}, weights from {+-1} (nothing is zero: every product matters), bias
and row vector from the integers of +-8, the residual from +-16.  f16 x f16 products of such integers are exact, fp32
accumulation of integers below 2^24 is exact in any order, an f16 slab holds every integer of magnitude <= 2048, and an
integer epilogue with a power-of-two out_scale rounds nothing.  For the Winograd form B^T d B of integers is an integer
(<= 4 max|d| in magnitude), G g G^T of +-1 taps is a multiple of 1/4, f16 holds multiples of 1/4 exactly below 512, and
A^T M A is additions only.

What is here (numpy, float64 holding integers — exact far beyond the sizes used — so the products run through BLAS):
  * generators for the operands;
  * the references: GEMM, conv3x3 (stride 1 / 2, nearest-2x upsample, pad_after_only, + a 1x1 second input) and the epilogue
    in the library's order (acc + bias + rowvec + residual) * scale;
  * a model of the slab decomposition: a launch is a Problem — the A and W matrices with their columns in the kernels' k order
    (conv: 64-channel chunk outer, tap inner; a second input's k-steps behind the nine taps') and the column range of every
    k-step of 64 — and Problem.partials(splits) forms the partial sum of every (row, column, split) from the planner's split
    count (hip.gemm_plan_query / hip.conv3x3_plan_query: nk_per_split = ceil(nk / splits)).  For Winograd, wino_model forms the
    sixteen transform-domain partials (+ the four parity entries of a second input) per (tile, channel, split);
  * the conditions, asserted on the reference alone before any launch (check_* below): a case that violates one is an error
    of the test, never a skip.

The models take a `mutate` argument: one misplaced term each, for tests/test_gemm_exact_host.py to show that the exact
comparison catches it (and how much of it the tolerance of tests/test_hip_kernels.py lets through).  No GPU needed."""
import numpy as np

BK = 64

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


# ---- operands ---------------------------------------------------------------------------------------------------------
def gen(seed):
    return np.random.default_rng(seed)


def acts(g, *shape):
    return g.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape)


def signs(g, *shape):
    return g.choice(np.array([-1.0, 1.0]), size=shape)


def ints(g, bound, *shape):
    return g.integers(-bound, bound + 1, size=shape).astype(np.float64)


# ---- the slab decomposition of the GEMM / conv kernels ------------------------------------------------------------------
class Problem:
    """A [M][Ktot] and W [N][Ktot] with the columns in k order, steps[ks] = (lo, hi): the columns of k-step ks."""

    def __init__(self, A, W, steps, nk1=None):
        assert A.shape[1] == W.shape[1] == steps[-1][1]
        self.A, self.W, self.steps = A, W, steps
        self.nk1 = nk1          # first k-step of a second input (None: no second input)

    @property
    def nk(self):
        return len(self.steps)

    def acc(self):
        return self.A @ self.W.T

    def slices(self, splits):
        """k-step ranges [(first, last + 1)] of the split-K slices: nk_per_split = ceil(nk / splits) (igemm_plan.hip)."""
        per = -(-self.nk // splits)
        out = [(s * per, min(self.nk, (s + 1) * per)) for s in range(splits)]
        assert all(b > a for a, b in out), f"{splits} splits of {self.nk} k-steps leave an empty slice: not what the planner plans"
        return out

    def step_sum(self, lo_step, hi_step, skip=()):
        tot = np.zeros((self.A.shape[0], self.W.shape[0]))
        for ks in range(lo_step, hi_step):
            if ks in skip:
                continue
            lo, hi = self.steps[ks]
            tot += self.A[:, lo:hi] @ self.W[:, lo:hi].T
        return tot

    def partials(self, splits, mutate=None):
        """[splits][M][N].  mutate = "drop_last_step_of_middle_split": slice splits // 2 loses its last k-step."""
        sl = self.slices(splits)
        skip = ()
        if mutate == "drop_last_step_of_middle_split":
            assert splits >= 3
            skip = (sl[splits // 2][1] - 1,)
        else:
            assert mutate is None, mutate
        return np.stack([self.step_sum(a, b, skip) for a, b in sl])


def reduce_slabs(partials, slab_dtype=None):
    """The reduce pass: the fixed-order fp32 sum of the slabs, each rounded to the slab's format first."""
    acc = np.zeros(partials.shape[1:], dtype=np.float32)
    for p in partials:
        with np.errstate(over="ignore", invalid="ignore"):
            acc = acc + (p.astype(slab_dtype).astype(np.float32) if slab_dtype is not None else p.astype(np.float32))
    return acc.astype(np.float64)


def k_steps(K, base=0):
    return [(base + c, base + min(K, c + BK)) for c in range(0, K, BK)]


def gemm_problem(A, W, mutate=None):
    """rcdm_gemm: k-steps of 64 columns, the last one K % 64 wide.  mutate = "drop_k_tail": the tail step reads zeros."""
    A, W = np.array(A, dtype=np.float64), np.array(W, dtype=np.float64)
    if mutate == "drop_k_tail":
        tail = A.shape[1] % BK
        assert tail
        A[:, -tail:] = 0
    else:
        assert mutate is None, mutate
    return Problem(A, W, k_steps(A.shape[1]))


def conv_patches(x, stride=1, up=0, pad_after_only=0):
    """x [n][H][W][C] -> [n * Ho * Wo][9][C]: the nine taps (ky, kx row-major) of every output pixel, zeros outside the
    (nearest-2x upsampled, if up) image; padding 1 on every side, or (pad_after_only, stride 2) one row / column after."""
    if up:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    n, H, W, C = x.shape
    before = 0 if pad_after_only else 1
    xp = np.zeros((n, H + 2, W + 2, C))
    xp[:, before:before + H, before:before + W] = x
    Ho = Wo = None
    taps = []
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + H:stride, kx:kx + W:stride]      # ceil(H / stride) rows: (H - 1) // stride + 1
            Ho, Wo = v.shape[1:3]
            taps.append(v.reshape(n * Ho * Wo, C))
    return np.stack(taps, axis=1), Ho, Wo


def conv_problem(x, w, stride=1, up=0, pad_after_only=0, x2=None, w2=None, mutate=None):
    """rcdm_conv3x3 / rcdm_conv3x3_add1x1 as the kernels walk it: k-step ks = (64-channel chunk ks // 9, tap ks % 9), the
    second input's chunks behind them.  x [n][H][W][C], w [c_out][c_in][3][3], x2 [n][H][W][C2], w2 [c_out][C2].
    mutate: "drop_c_tail" (the c_in % 64 chunk reads zeros), "double_border_tap" (the centre tap of the image's first row is
    counted twice), "swap_second_input_with_last_tap" (the A columns of the second input's first k-step and of the last
    tap's last chunk change places, the weights stay)."""
    P, Ho, Wo = conv_patches(np.asarray(x, dtype=np.float64), stride, up, pad_after_only)
    P = P.copy()
    M, _, C = P.shape
    N = w.shape[0]
    w9 = np.asarray(w, dtype=np.float64).reshape(N, C, 9).transpose(0, 2, 1)     # [N][tap][C]
    if mutate == "drop_c_tail":
        assert C % BK
        P[:, :, C - C % BK:] = 0
    elif mutate == "double_border_tap":
        first_row = (np.arange(M) % (Ho * Wo)) < Wo
        P[first_row, 4] *= 2
    else:
        assert mutate in (None, "swap_second_input_with_last_tap"), mutate
    a_cols, w_cols, steps = [], [], []
    col = 0
    for c0 in range(0, C, BK):
        c1 = min(C, c0 + BK)
        for tap in range(9):
            a_cols.append(P[:, tap, c0:c1])
            w_cols.append(w9[:, tap, c0:c1])
            steps.append((col, col + c1 - c0))
            col += c1 - c0
    nk1 = None
    if x2 is not None:
        nk1 = len(steps)
        x2r = np.asarray(x2, dtype=np.float64).reshape(M, -1)
        a_cols.append(x2r)
        w_cols.append(np.asarray(w2, dtype=np.float64))
        steps += k_steps(x2r.shape[1], col)
    A, Wm = np.concatenate(a_cols, axis=1), np.concatenate(w_cols, axis=1)
    if mutate == "swap_second_input_with_last_tap":
        assert nk1 is not None and steps[nk1][1] - steps[nk1][0] == steps[nk1 - 1][1] - steps[nk1 - 1][0]
        (a0, a1), (b0, b1) = steps[nk1 - 1], steps[nk1]
        A[:, a0:a1], A[:, b0:b1] = A[:, b0:b1].copy(), A[:, a0:a1].copy()
    p = Problem(A, Wm, steps, nk1)
    p.Ho, p.Wo = Ho, Wo
    return p


UP2_TAPS = {0: ([0], [1, 2]), 1: ([0, 1], [2])}    # phase parity -> the 3x3 rows (columns) that land on source offset 0 / 1


def up2_pack(w):
    """rcdm_pack_conv3x3_up2 in numpy: [phase 2a + b][c_out][tap 2r + c][c_in], each entry the sum of the 3x3 taps that land on
    source pixel (y + a - 1 + r, x + b - 1 + c): at most four +-1 taps, exact in f16."""
    N, C = w.shape[:2]
    out = np.zeros((4, N, 4, C))
    for a in (0, 1):
        for b in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    out[2 * a + b, :, 2 * r + c] = w[:, :, UP2_TAPS[a][r]][:, :, :, UP2_TAPS[b][c]].sum(axis=(2, 3))
    return out


def up2_problems(x, w):
    """upsample = 2 (four 2x2 phase convolutions over the source grid): one Problem per phase over the source pixels, k-step
    ks = (chunk ks // 4, tap ks % 4); and out_rows[phase][source pixel] = the output row of the upsampled image."""
    x = np.asarray(x, dtype=np.float64)
    n, H, W, C = x.shape
    assert C % BK == 0
    wp = up2_pack(np.asarray(w, dtype=np.float64))
    xp = np.zeros((n, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    probs, rows = [], []
    img, y, xx = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
    for a in (0, 1):
        for b in (0, 1):
            a_cols, w_cols, steps = [], [], []
            col = 0
            for c0 in range(0, C, BK):
                for r in (0, 1):
                    for c in (0, 1):
                        a_cols.append(xp[:, a + r:a + r + H, b + c:b + c + W, c0:c0 + BK].reshape(n * H * W, BK))
                        w_cols.append(wp[2 * a + b, :, 2 * r + c, c0:c0 + BK])
                        steps.append((col, col + BK))
                        col += BK
            probs.append(Problem(np.concatenate(a_cols, axis=1), np.concatenate(w_cols, axis=1), steps))
            rows.append((img * 4 * H * W + (2 * y + a) * 2 * W + 2 * xx + b).reshape(-1))
    return probs, rows


def epilogue(acc, bias=None, rowvec=None, rows_per_sample=1, residual=None, scale=1.0):
    """(acc + bias + rowvec[row // rows_per_sample] + residual) * scale, the library's order."""
    out = acc.copy()
    if bias is not None:
        out = out + bias[None, :]
    if rowvec is not None:
        out = out + rowvec[np.arange(out.shape[0]) // rows_per_sample]
    if residual is not None:
        out = out + residual
    return out * scale


# ---- Winograd F(2x2, 3x3) ---------------------------------------------------------------------------------------------------
def wino_slices(nk, splits):
    per = -(-nk // splits)
    return [(min(nk, s * per) * BK, min(nk, (s + 1) * per) * BK) for s in range(splits)]   # (an empty slice: lo == hi)


def wino_model(x, w, splits, x2=None, w2=None, operand_dtype=np.float16, slab_dtype=None, mutate=None):
    """The three launches of rcdm_conv3x3_wino.  x [n][H][W][K] (already through the GroupNorm map, if any: the padding is
    zeros AFTER it), w [N][K][3][3], x2 [n][H][W][K2], w2 [N][K2].  V = B^T d B and U = G g G^T are rounded to operand_dtype
    (None: kept), the slabs [entry][split][tile][N] to slab_dtype (None: kept).  Returns (out [n * H * W][N], slabs, V, U);
    slabs[e] for e < 16 is position (e // 4, e % 4), 16 + 2a + b the second input's parity entry (a, b).
    mutate: "swap_positions" (V of position (1, 2) and (2, 1) change places), "wrong_parity_pixel" (entry (0, 1) of the second
    input reads pixel (1, 0) of the tile)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, H, W, K = x.shape
    N = w.shape[0]
    th, tw = H // 2, W // 2
    T = n * th * tw
    xp = np.zeros((n, H + 2, W + 2, K))
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.zeros((n, th, tw, 4, 4, K))
    for i in range(4):
        for j in range(4):
            d[:, :, :, i, j] = xp[:, i:i + H:2, j:j + W:2][:, :th, :tw]
    d = d.reshape(T, 4, 4, K)
    V = np.einsum("ik,tklc,jl->ijtc", BT, d, BT)                 # [4][4][T][K]
    U = np.einsum("ik,ockl,jl->ijoc", G, w, G)                   # [4][4][N][K]
    with np.errstate(over="ignore"):
        if operand_dtype is not None:
            V, U = V.astype(operand_dtype).astype(np.float64), U.astype(operand_dtype).astype(np.float64)
    if mutate == "swap_positions":
        V = V.copy()
        V[1, 2], V[2, 1] = V[2, 1].copy(), V[1, 2].copy()
    else:
        assert mutate in (None, "wrong_parity_pixel"), mutate
    E = 20 if x2 is not None else 16
    slabs = np.zeros((E, splits, T, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for s, (lo, hi) in enumerate(wino_slices(K // BK, splits)):
            for e in range(16):
                slabs[e, s] = V[e // 4, e % 4][:, lo:hi] @ U[e // 4, e % 4][:, lo:hi].T
        if x2 is not None:
            x2 = np.asarray(x2, dtype=np.float64)
            w2 = np.asarray(w2, dtype=np.float64)
            K2 = x2.shape[-1]
            for s, (lo, hi) in enumerate(wino_slices(K2 // BK, splits)):
                for a in (0, 1):
                    for b in (0, 1):
                        pa, pb = (1, 0) if (mutate == "wrong_parity_pixel" and (a, b) == (0, 1)) else (a, b)
                        rows = x2[:, pa::2, pb::2].reshape(T, K2)
                        slabs[16 + 2 * a + b, s] = rows[:, lo:hi] @ w2[:, lo:hi].T
        stored = slabs.astype(slab_dtype).astype(np.float32) if slab_dtype is not None else slabs.astype(np.float32)
        m = np.zeros((E, T, N), dtype=np.float32)
        for s in range(splits):                                   # the fixed-order fp32 sum of the output transform
            m = m + stored[:, s]
        m = m.astype(np.float64)
        Y = np.einsum("ai,ijtn,bj->tabn", AT, m[:16].reshape(4, 4, T, N), AT)      # [T][2][2][N]
        if x2 is not None:
            Y = Y + m[16:].reshape(2, 2, T, N).transpose(2, 0, 1, 3)
    out = Y.reshape(n, th, tw, 2, 2, N).transpose(0, 1, 3, 2, 4, 5).reshape(n * H * W, N)
    return out, slabs, V, U


# ---- the conditions -----------------------------------------------------------------------------------------------------
def check_output(ref):
    """Every expected output round-trips through f16."""
    assert np.isfinite(ref).all()
    assert (ref.astype(np.float16).astype(np.float64) == ref).all(), "an expected output is not an f16 value"


def check_partials(partials):
    """Every split-K partial is an integer of magnitude <= 2048: exact in an f16 slab (and far below 2^24: exact in fp32)."""
    assert (partials == np.rint(partials)).all(), "a partial sum is not an integer"
    assert np.abs(partials).max() <= 2048, f"a partial sum of magnitude {np.abs(partials).max()}: not exact in an f16 slab"
    return float(np.abs(partials).max())


def check_wino(slabs, V, U):
    """Every transform-domain partial is a multiple of 1/4 of magnitude < 512, V holds integers and U multiples of 1/4 that f16
    keeps: the operand roundings and the f16 slabs change nothing."""
    for name, a in (("V", V), ("U", U), ("slab", slabs)):
        assert (4 * a == np.rint(4 * a)).all(), f"{name}: not a multiple of 1/4"
        assert np.abs(a).max() < 512, f"{name}: magnitude {np.abs(a).max()}"
    assert (V == np.rint(V)).all()
    return float(np.abs(slabs).max())


def f16_half_spacing(v):
    """Half the spacing of f16 at |v| (v an array): the rounding error bound of storing v in an f16 slab."""
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(v).astype(np.float16)).astype(np.float64) / 2


def slab_error_bound(partials, result):
    """Sum over the splits of half the f16 spacing at each partial, plus half the spacing at the result (the output
    rounding): what f16 slabs may cost a sum whose partials cancel.  partials [splits][...], result [...]."""
    return f16_half_spacing(partials).sum(axis=0) + f16_half_spacing(result)


def close_accepts(got, ref, rel=2e-3, abs_frac=4e-3):
    """Elementwise: would close() of tests/test_hip_kernels.py accept got against ref?"""
    tol = abs_frac * np.abs(ref).max() + rel * np.abs(ref)
    return np.abs(got - ref) <= tol


# ---- the cases (shared by tests/test_gemm_exact_host.py and tests/test_hip_gemm_exact.py) -----------------------------------
EPI_BIAS, EPI_ROWVEC, EPI_RESIDUAL = 1, 2, 4

# rcdm_gemm: (M, N, K, epilogue, split_k, out_scale)
GEMM_CASES = [
    (130, 72, 200, 1 | 4, 3, 1.0),         # K tail of 8 channels (200 = 3 * 64 + 8), split 3 -> slices of 2 / 2 k-steps
    (300, 320, 320, 1 | 2 | 4, 1, 1.0),    # rows_per_sample = 150 straddling a tile; bias | rowvec | residual
    (300, 320, 320, 1 | 2 | 4, 2, 2.0),    # ... through slabs, out_scale 2
    (161, 168, 704, 1, 3, 1.0),            # one row and one 8-column chunk past a 160 tile; 11 k-steps as 4 / 4 / 3
    (161, 168, 704, 1, 4, 1.0),            # ... as 3 / 3 / 3 / 2
    (257, 264, 128, 0, 2, 1.0),            # past a 256 tile, split 2
    (260, 64, 64, 1 | 2 | 4, 1, 1.0),      # row vector with 100 rows per sample
    (130, 72, 200, 1 | 4, 3, 0.5),         # out_scale 0.5
    (300, 320, 320, 1, 0, 1.0),            # heuristic split
]
# rcdm_conv3x3 / rcdm_conv3x3_add1x1: (n_img, H, W, c_in, c_out, stride, upsample, pad_after_only, split_k, c_in2)
CONV_CASES = [
    (6, 10, 6, 72, 72, 1, 0, 0, 1, 0),     # c_in tail, M and N tails
    (5, 16, 16, 64, 64, 2, 0, 0, 1, 0),    # stride 2
    (5, 16, 16, 64, 64, 2, 0, 1, 1, 0),    # ... pad_after_only
    (5, 8, 8, 128, 64, 1, 1, 0, 1, 0),     # nearest-2x upsample folded into the loader
    (2, 8, 8, 320, 320, 1, 0, 0, 4, 0),    # split 4: 45 k-steps as 12 / 12 / 12 / 9
    (10, 8, 8, 192, 64, 1, 0, 0, 3, 0),    # 2.5 images per 160-row tile, split 3
    (6, 10, 6, 72, 72, 1, 0, 0, 3, 0),     # the c_in tail through slabs
]
ADD1X1_CASES = [
    (6, 10, 6, 128, 72, 1, 0, 0, 1, 64),
    (2, 8, 8, 320, 320, 1, 0, 0, 4, 640),  # 55 k-steps as 14 / 14 / 14 / 13: the second input's ten sit in the last slab
]
# rcdm_conv3x3 with upsample = 2: (n_img, H, W, c_in, c_out, variant, split_k); -1 needs a shape that fills the chip
UP2_CASES = [
    (5, 16, 16, 64, 96, 6, 0), (5, 16, 16, 64, 96, 6, 3),
    (5, 16, 16, 64, 96, 7, 0), (5, 16, 16, 64, 96, 7, 3),
    (5, 16, 16, 64, 96, 8, 0), (5, 16, 16, 64, 96, 8, 3),
    (10, 8, 8, 192, 64, 6, 3),             # image borders inside a tile
    (40, 16, 16, 64, 320, -1, 0), (40, 16, 16, 64, 320, -1, 3),
]
# rcdm_conv3x3_wino: (n_img, H, W, c_in, c_in2, c_out, epilogue, split_k, out_scale, gn)
WINO_CASES = [
    (2, 4, 4, 64, 0, 64, 0, 0, 1.0, False),            # 8 tiles: one partly filled row tile
    (2, 8, 8, 128, 0, 192, 1 | 4, 3, 1.0, False),      # forced split 3 of 2 k-steps: planned as 2
    (10, 6, 10, 64, 0, 64, 1, 0, 1.0, False),
    (2, 8, 8, 128, 64, 320, 0, 2, 1.0, False),         # the second input has one k-step: its second slice is empty
    (2, 8, 8, 128, 64, 320, 1 | 2 | 4, 2, 0.5, False),
    (2, 8, 8, 128, 0, 64, 1, 2, 1.0, True),            # GroupNorm prologue as the exact affine map 2 x + 3
]
GN_GAMMA, GN_BETA = 2.0, 3.0

_cache = {}


def _cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _cache:
            _cache[k] = fn(*key)
        return _cache[k]
    return wrapper


def gemm_rows_per_sample(M):
    return 150 if M == 300 else 100


@_cached
def gemm_case(M, N, K, epi, scale):
    """Operands, Problem and expected output of a rcdm_gemm case (computed once, shared, never modified)."""
    g = gen(1000 + M + N + K)
    rps = gemm_rows_per_sample(M)
    c = dict(A=acts(g, M, K), W=signs(g, N, K), bias=ints(g, 8, N), rowvec=ints(g, 8, -(-M // rps), N), res=ints(g, 16, M, N), rps=rps)
    c["problem"] = gemm_problem(c["A"], c["W"])
    c["ref"] = epilogue(c["problem"].acc(), c["bias"] if epi & 1 else None, c["rowvec"] if epi & 2 else None, rps,
                        c["res"] if epi & 4 else None, scale)
    check_output(c["ref"])
    return c


@_cached
def conv_case(n_img, H, W, cin, cout, stride, up, pao, cin2, epi, scale):
    g = gen(2000 + n_img + H + cin + cout + stride + up + pao + cin2)
    c = dict(x=acts(g, n_img, H, W, cin), w=signs(g, cout, cin, 3, 3), bias=ints(g, 8, cout), rowvec=ints(g, 8, n_img, cout))
    if cin2:
        c["x2"], c["w2"] = acts(g, n_img, H, W, cin2), signs(g, cout, cin2)
    p = conv_problem(c["x"], c["w"], stride, up, pao, c.get("x2"), c.get("w2"))
    c["problem"], c["rps"] = p, p.Ho * p.Wo
    c["res"] = ints(g, 16, n_img * p.Ho * p.Wo, cout)
    c["ref"] = epilogue(p.acc(), c["bias"] if epi & 1 else None, c["rowvec"] if epi & 2 else None, c["rps"],
                        c["res"] if epi & 4 else None, scale)
    check_output(c["ref"])
    return c


@_cached
def up2_case(n_img, H, W, cin, cout):
    g = gen(3000 + n_img + H + cin + cout)
    c = dict(x=acts(g, n_img, H, W, cin), w=signs(g, cout, cin, 3, 3), bias=ints(g, 8, cout))
    c["problems"], c["rows"] = up2_problems(c["x"], c["w"])
    ref = np.zeros((4 * n_img * H * W, cout))
    for p, r in zip(c["problems"], c["rows"]):
        ref[r] = p.acc()
    # the definition: nearest-2x upsample, then the nine-tap convolution
    assert (ref == conv_problem(c["x"], c["w"], 1, 1).acc()).all(), "the phase form is not the upsampled convolution"
    c["ref"] = ref + c["bias"][None, :]
    check_output(c["ref"])
    return c


@_cached
def wino_case(n_img, H, W, cin, cin2, cout, epi, scale, gn):
    g = gen(4000 + n_img + H + cin + cin2 + cout)
    c = dict(x=acts(g, n_img, H, W, cin), w=signs(g, cout, cin, 3, 3), bias=ints(g, 8, cout), rowvec=ints(g, 8, n_img, cout),
             res=ints(g, 16, n_img * H * W, cout), rps=H * W)
    if cin2:
        c["x2"], c["w2"] = acts(g, n_img, H, W, cin2), signs(g, cout, cin2)
    c["x_eff"] = c["x"] * GN_GAMMA + GN_BETA if gn else c["x"]
    p = conv_problem(c["x_eff"], c["w"], 1, 0, 0, c.get("x2"), c.get("w2"))      # the nine-tap definition; zero padding after the map
    c["acc"] = p.acc()
    c["ref"] = epilogue(c["acc"], c["bias"] if epi & 1 else None, c["rowvec"] if epi & 2 else None, c["rps"],
                        c["res"] if epi & 4 else None, scale)
    check_output(c["ref"])
    return c


def wino_check(c, splits):
    """The model of the three launches at this split count: conditions hold, f16 operands and f16 slabs leave the answer exact."""
    for slab in (None, np.float16):
        out, slabs, V, U = wino_model(c["x_eff"], c["w"], splits, c.get("x2"), c.get("w2"), np.float16, slab)
        assert (out == c["acc"]).all(), "the Winograd model is not the nine-tap convolution"
    return check_wino(slabs, V, U)


# ---- slab range: partials that cancel, partials beyond f16 ------------------------------------------------------------------
CANCEL_M, CANCEL_N, CANCEL_K = 130, 72, 128
WINO_CANCEL_LEVELS = (4, 70)       # pixel level A: the largest transform-domain partial is 64 channels * 4 A * 9/4 = 576 A


@_cached
def cancel_gemm_case(P):
    """K = 128 as two k-steps, split 2, all-ones weights: row m's partials are (P, -P + r[m]) with r = -8 .. 8.  Every operand
    is an f16 value (P / 64 = 32, 625, 1280), every sum an integer below 2^24."""
    assert P % 64 == 0
    M, N, K = CANCEL_M, CANCEL_N, CANCEL_K
    r = (np.arange(M) % 17 - 8).astype(np.float64)
    A = np.concatenate([np.full((M, 64), P / 64), np.full((M, 64), -P / 64)], axis=1)
    A[np.arange(M), 64 + np.arange(M) % 64] += r
    assert (A.astype(np.float16).astype(np.float64) == A).all()
    c = dict(A=A, W=np.ones((N, K)), r=np.repeat(r[:, None], N, axis=1))
    c["problem"] = gemm_problem(A, c["W"])
    assert (c["problem"].acc() == c["r"]).all()
    check_output(c["r"])
    return c


@_cached
def cancel_wino_case(A):
    """2 images of 8x8, 128 -> 64 channels, split 2, all-ones taps: the first 64 channels carry +A, the second 64 carry
    -A + (integers of +-2), so the two slices' transform-domain sums cancel to small values."""
    g = gen(5000 + A)
    x = np.concatenate([np.full((2, 8, 8, 64), float(A)), -float(A) + ints(g, 2, 2, 8, 8, 64)], axis=3)
    c = dict(x=x, w=np.ones((64, 128, 3, 3)))
    c["acc"] = conv_problem(x, c["w"]).acc()
    check_output(c["acc"])
    return c


def wino_slab_error_bound(slabs, result, n_img=2, H=8, W=8):
    """slab_error_bound for the Winograd form: output (a, b) of a tile is the sum of the positions (i, j) with
    A^T[a][i] A^T[b][j] != 0 (coefficients +-1), each the sum of its splits' slabs; rows in the image's pixel order."""
    E, S, T, N = slabs.shape
    hs = f16_half_spacing(slabs[:16]).sum(axis=1).reshape(4, 4, T, N)
    per_tile = np.einsum("ai,ijtn,bj->tabn", np.abs(AT), hs, np.abs(AT))
    rows = per_tile.reshape(n_img, H // 2, W // 2, 2, 2, N).transpose(0, 1, 3, 2, 4, 5).reshape(n_img * H * W, N)
    return rows + f16_half_spacing(result)


@_cached
def overflow_wino_case():
    """2 images of 8x8, 64 -> 64 channels.  Image 0 is a checkerboard of +-20000 in every channel (B^T d B reaches 80000 at
    position (2, 2) of every tile: beyond f16), image 1 the same board at +-2.  Channel 2k + 1 carries the taps of channel 2k
    negated, so every nine-tap sum cancels to exactly zero."""
    g = gen(6000)
    y, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    board = np.where((y + xx) % 2 == 0, 1.0, -1.0)
    x = np.stack([20000 * board, 2 * board])[:, :, :, None].repeat(64, axis=3)
    w = signs(g, 64, 32, 3, 3).repeat(2, axis=1)
    w[:, 1::2] *= -1
    assert (x.astype(np.float16).astype(np.float64) == x).all()
    c = dict(x=x, w=w, big_rows=np.arange(2 * 64) < 64)
    c["acc"] = conv_problem(x, w).acc()
    return c
