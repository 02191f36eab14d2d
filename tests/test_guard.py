"""CPU: the guarded-buffer harness (tests/guard.py) against torch stand-ins of a kernel that are wrong on purpose, each in
one of the ways the harness claims to detect.  Every wrong stand-in must be caught by the check meant for it and by no other;
the correct stand-in passes all of them.  Needs no GPU (the stand-ins are torch on the CPU, reading and writing the same
guarded allocations, through the same row stride, as a C-ABI kernel would)."""
import pytest
import torch

from tests import guard as G

DEV = "cpu"
M, N, K = 40, 24, 72
LDA, LDC = K + 16, N + 8
GR = 32


def close(got, ref, rel=2e-3, abs_frac=4e-3):
    """The kernel suites' value assertion (tests/test_hip_kernels.py), restated so this file imports nothing that needs a GPU."""
    got, ref = got.detach().float(), ref.detach().float()
    assert torch.isfinite(got).all(), "non-finite output"
    err = (got - ref).abs()
    assert not (err > abs_frac * ref.abs().max() + rel * ref.abs()).any(), f"max err {err.max():.4g}"


def raw(view):
    """What a kernel sees: the flat allocation behind the view and the element offset of view[0, 0] in it."""
    h = view.guard
    return h.buf.reshape(-1), h.guard_rows * h.ld, h.ld


def load(view, rows, cols, row0=0):
    """rows x cols read through the row stride from the operand's address, as a branch-free loader without a mask would."""
    flat, off, ld = raw(view)
    idx = off + (row0 + torch.arange(rows))[:, None] * ld + torch.arange(cols)[None, :]
    return flat[idx.reshape(-1)].reshape(rows, cols).float()


def store(view, vals, row0=0):
    flat, off, ld = raw(view)
    rows, cols = vals.shape
    idx = off + (row0 + torch.arange(rows))[:, None] * ld + torch.arange(cols)[None, :]
    flat[idx.reshape(-1)] = vals.to(flat.dtype).reshape(-1)


def operands(dtype=torch.float16):
    g = torch.Generator().manual_seed(1)
    A = torch.randn(M, K, generator=g).to(dtype).float()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype).float()
    Ad, _ = G.guarded_in(A.to(dtype), LDA, device=DEV, guard_rows=GR)
    Wd, _ = G.guarded_w(W.to(dtype), device=DEV, guard_rows=GR)
    out, _ = G.guarded_out(M, N, LDC, dtype, device=DEV, guard_rows=GR)
    return A, W, Ad, Wd, out


def gemm_standin(Ad, Wd, out, k_read=K, rows_stored=M, cols_stored=N, rows_skipped=0):
    """out = A W^T.  k_read > K: the K-tail mask of the A loader is missing (W's k-tail is NOT zero-filled either: the next
    weight row's live data stands in for it, as in a dense W[N][K]); the other knobs move the store loop's bounds."""
    a = load(Ad, max(rows_stored, M), k_read)
    w = load(Wd, max(cols_stored, N), k_read)
    c = a @ w.t()
    store(out, c[:rows_stored - rows_skipped, :cols_stored])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_correct_standin_passes_every_check(dtype):
    A, W, Ad, Wd, out = operands(dtype)
    gemm_standin(Ad, Wd, out)
    close(out[:, :N], A @ W.t())
    G.check_written(out)
    G.check_out(out)
    G.check_in(Ad)
    G.check_in(Wd)
    G.check_all(out, Ad, Wd)


def test_gemm_reading_k_plus_8_columns_fails_the_value_assertion():
    """The over-read lands on poison x live data: the value assertion fails; nothing was written out of place, so the
    placement checks stay quiet.  (With zero padding, as the suites had it, this stand-in passes: shown last.)"""
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out, k_read=K + 8)
    with pytest.raises(AssertionError, match="max err|non-finite"):
        close(out[:, :N], A @ W.t())
    G.check_out(out)
    G.check_in(Ad)
    G.check_in(Wd)
    # the habit this replaces: zero padding hides the same stand-in
    Az = torch.zeros(M + 1, LDA, dtype=torch.float16)
    Az[:M, :K] = A.half()
    Wz = torch.zeros(N + 1, K + 8, dtype=torch.float16)
    Wz[:N, :K] = W.half()
    close(Az[:M, :K + 8].float() @ Wz[:N].float().t(), A @ W.t())


def test_masked_over_read_is_harmless_by_design():
    """Poison is finite: an over-read whose partner is masked to zero contributes poison * 0 = 0 and passes."""
    A, W, Ad, Wd, out = operands()
    a = load(Ad, M, K + 8)
    w = load(Wd, N, K + 8)
    w[:, K:] = 0.0
    store(out, a @ w.t())
    close(out[:, :N], A @ W.t())
    G.check_all(out, Ad, Wd)


def test_layernorm_averaging_over_ld_fails_the_value_assertion():
    g = torch.Generator().manual_seed(2)
    C, ld = 64, 72
    x = (torch.randn(M, C, generator=g) * 3 + 1).half()
    xd, _ = G.guarded_in(x, ld, device=DEV, guard_rows=GR)
    ref = torch.nn.functional.layer_norm(x.float(), (C,))
    for width, ok in ((C, True), (ld, False)):
        y, _ = G.guarded_out(M, C, ld, torch.float16, device=DEV, guard_rows=GR)
        row = load(xd, M, width)
        mean, var = row.mean(dim=1, keepdim=True), row.var(dim=1, unbiased=False, keepdim=True)
        store(y, ((row - mean) * torch.rsqrt(var + 1e-5))[:, :C])
        if ok:
            close(y[:, :C], ref)
        else:
            with pytest.raises(AssertionError, match="max err|non-finite"):
                close(y[:, :C], ref)
        G.check_out(y)
        G.check_in(xd)


def test_store_loop_writing_m_plus_1_rows_is_caught_below_row_m():
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out, rows_stored=M + 1)
    close(out[:, :N], A @ W.t())              # the M rows themselves are right: only the guard band can tell
    G.check_written(out)
    with pytest.raises(AssertionError, match="wrote below row M"):
        G.check_out(out)
    G.check_in(Ad)


def test_store_starting_one_row_early_is_caught_above_row_0():
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out)
    store(out, torch.ones(1, N), row0=-1)
    close(out[:, :N], A @ W.t())
    with pytest.raises(AssertionError, match="wrote above row 0"):
        G.check_out(out)


def test_store_writing_ld_columns_is_caught_in_the_pad_columns():
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out, cols_stored=LDC)
    close(out[:, :N], A @ W.t())
    G.check_written(out)
    with pytest.raises(AssertionError, match="wrote outside the C columns"):
        G.check_out(out)
    G.check_in(Wd)


def test_last_16_rows_unwritten_fail_the_value_assertion_and_are_named():
    """A stale right answer in a recycled torch.empty block would hide this; the NaN fill cannot."""
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out, rows_skipped=16)
    with pytest.raises(AssertionError, match="non-finite output"):
        close(out[:, :N], A @ W.t())
    with pytest.raises(AssertionError, match=rf"left {16 * N} elements unwritten.*rows {M - 16}\.\.{M - 1}"):
        G.check_written(out)
    G.check_out(out)                          # nothing out of place


def test_kernel_writing_into_a_read_only_operand_is_caught_by_check_in():
    A, W, Ad, Wd, out = operands()
    gemm_standin(Ad, Wd, out)
    store(Ad, torch.zeros(1, 8), row0=M)       # "normalised in place", one row too far
    with pytest.raises(AssertionError, match="read-only operand changed below row M"):
        G.check_in(Ad)
    flat, off, ld = raw(Wd)
    flat[off + K - 1] = -flat[off + K - 1] - 1.0
    with pytest.raises(AssertionError, match="read-only operand changed inside the operand"):
        G.check_in(Wd)
    G.check_out(out)


def test_guarded_vec_alignment_poison_and_check():
    b = torch.arange(24, dtype=torch.float32)
    bd, h = G.guarded_vec(b, device=DEV)
    assert bd.data_ptr() % 16 == 0 and torch.equal(bd, b)
    assert (h.buf[0, :G.VEC_GUARD].abs() == G.POISON).all() and (h.buf[0, G.VEC_GUARD + 24:].abs() == G.POISON).all()
    G.check_in(bd)
    h.buf[0, G.VEC_GUARD + 24] = 0.0           # a float4 store one element past the end
    with pytest.raises(AssertionError, match="read-only vector operand changed.*index 24 of 24"):
        G.check_in(bd)
    rv, _ = G.guarded_vec(torch.ones(3, 8), device=DEV)
    assert rv.shape == (3, 8)


def test_poison_is_finite_fixed_and_of_both_signs():
    for dtype in (torch.float16, torch.float32):
        x, h = G.guarded_in(torch.zeros(4, 8, dtype=dtype), 16, device=DEV, guard_rows=8)
        x2, h2 = G.guarded_in(torch.zeros(4, 8, dtype=dtype), 16, device=DEV, guard_rows=8)
        assert torch.equal(h.buf, h2.buf), "poison must not depend on generator state"
        p = h.buf[:8].float()
        assert torch.isfinite(p).all() and (p.abs() == G.POISON).all()
        assert 0.25 < (p > 0).float().mean() < 0.75
        assert (h.buf[8:12, 8:].abs() == G.POISON).all() and (h.buf[8:12, :8] == 0).all()
        assert x.shape == (4, 16) and x.data_ptr() == h.buf.data_ptr() + 8 * 16 * x.element_size()


def test_integer_outputs_get_a_byte_pattern():
    for dtype in (torch.uint8, torch.int32):
        out, h = G.guarded_out(5, 8, 16, dtype, device=DEV, guard_rows=4)
        assert (h.buf.view(torch.uint8) == G.INT_FILL).all()
        out[:, :8] = 1
        G.check_out(out)
        out[4, 8] = 1
        with pytest.raises(AssertionError, match="wrote outside the C columns"):
            G.check_out(out)


def test_checks_refuse_the_wrong_kind_and_unguarded_tensors():
    A, W, Ad, Wd, out = operands()
    with pytest.raises(AssertionError):
        G.check_out(Ad)
    with pytest.raises(AssertionError):
        G.check_in(out)
    with pytest.raises(AssertionError, match="not a guarded buffer"):
        G.check_out(torch.zeros(2, 2))
