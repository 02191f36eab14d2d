"""Guarded buffers for the kernel-level tests: what a kernel is handed sits in the middle of a larger allocation whose every
other element is hostile, so a dropped column mask, a row over-run or a skipped tile changes what the test sees.

  inputs   guarded_in / guarded_vec / guarded_w: everything that is not the operand is FINITE POISON (magnitude 3.0e4, a fixed
           pseudo-random sign pattern): the pad columns C..ld, guard_rows rows above and guard_rows rows below.  Finite on
           purpose: an over-read whose partner is masked to zero gives poison * 0 = 0 and passes, only an over-read that
           changes the result fails (through the test's own value assertion).  check_in: the operand, poison included, is
           bit-identical after the call (a kernel wrote into a read-only operand).
  outputs  guarded_out: the same shape filled with NaN (floats) or a fixed byte pattern (integers).  A tile, a ragged tail or a
           split-K slab that is never stored stays NaN and fails the value assertion; check_out: the pad columns and both guard
           bands are bit-for-bit untouched.

guard_rows defaults to 256 = the tallest tile of the library (BM = 256): an error of one whole tile stays inside the test's own
allocation.  A plain module: every helper takes the device, so the CPU tests of tests/test_guard.py run it without a GPU."""
import torch

POISON = 3.0e4          # finite in f16 (max 65504), far outside anything the tests feed a kernel
GUARD_ROWS = 256
VEC_GUARD = 64          # elements of poison on either side of a 1-D operand: 256 bytes of fp32, keeps the 16-byte alignment
INT_FILL = 0x5A         # every byte of an integer output before the call

_BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def _bits(t):
    """Reinterpret as integers of the same width: NaN != NaN, and -0.0 == 0.0, so every comparison here is on the bits."""
    return t.view(_BITS[t.dtype]) if t.dtype in _BITS else t


def poison(numel, dtype, device, salt=0):
    """numel values of +-POISON, the sign a fixed hash of the element index (reproducible, no generator state touched)."""
    i = torch.arange(numel, dtype=torch.int64, device=device) + 7919 * salt
    h = (i * 2654435761) & 0xFFFFFFFF
    sign = 1.0 - 2.0 * (((h >> 13) ^ (h >> 21)) & 1).to(torch.float32)
    return (sign * POISON).to(dtype)


class Handle:
    """One guarded allocation: buf is [guard_rows + rows + guard_rows][ld], the operand is buf[guard_rows:guard_rows + rows, :C]."""

    def __init__(self, buf, rows, C, ld, guard_rows, kind):
        self.buf, self.rows, self.C, self.ld, self.guard_rows, self.kind = buf, rows, C, ld, guard_rows, kind
        self.snapshot = None          # inputs: the whole allocation as it was handed over
        self.fill = None              # outputs: the bit pattern of an untouched element

    @property
    def view(self):
        """rows x ld, the first C columns of each row are the operand; data_ptr() is what the kernel gets."""
        g = self.guard_rows
        v = self.buf[g:g + self.rows]
        v.guard = self
        return v

    @property
    def data(self):
        return self.view[:, :self.C]


def _handle(x):
    h = x if isinstance(x, Handle) else getattr(x, "guard", None)
    assert isinstance(h, Handle), "not a guarded buffer (use the view guarded_in / guarded_out returned, not a slice of it)"
    return h


def guarded_in(t, ld=None, *, device, guard_rows=GUARD_ROWS):
    """t (rows x C, f16 or f32) in the middle of poison: pad columns C..ld, guard_rows rows above and below.
    Returns (view, handle); view is rows x ld on `device`, view.data_ptr() is the operand's address."""
    assert t.dim() == 2, t.shape
    rows, C = t.shape
    ld = C if ld is None else int(ld)
    assert ld >= C and guard_rows >= 0
    total = rows + 2 * guard_rows
    buf = poison(total * ld, t.dtype, device, salt=rows + C).reshape(total, ld)
    buf[guard_rows:guard_rows + rows, :C] = t.to(device)
    h = Handle(buf, rows, C, ld, guard_rows, "in")
    h.snapshot = buf.clone()
    return h.view, h


def guarded_w(W, *, device, guard_rows=GUARD_ROWS):
    """A weight matrix W[N][K] (dense rows) with poisoned guard rows around it: a tile that reads weight rows >= N without
    masking its columns on the way out shows up in the result."""
    return guarded_in(W, W.shape[1], device=device, guard_rows=guard_rows)


def guarded_vec(v, *, device, guard=VEC_GUARD):
    """A 1-D (or dense n-D, flattened) fp32 operand (bias, gamma, beta, colsum, row vectors, ...) at a 16-byte-aligned offset
    inside poison.  Returns (view, handle); the view has v's shape."""
    flat = v.reshape(-1)
    n = flat.numel()
    assert (guard * flat.element_size()) % 16 == 0
    buf = poison(n + 2 * guard, flat.dtype, device, salt=n).reshape(1, -1)
    buf[0, guard:guard + n] = flat.to(device)
    h = Handle(buf, 1, n, n + 2 * guard, 0, "vec")
    h.offset = guard
    h.snapshot = buf.clone()
    view = buf[0, guard:guard + n].view(v.shape)
    assert view.data_ptr() % 16 == 0, "allocator returned a block that is not 16-byte aligned"
    view.guard = h
    return view, h


def guarded_out(rows, C, ld=None, dtype=torch.float16, *, device, guard_rows=GUARD_ROWS):
    """rows x C output inside an allocation filled with NaN (floats) or INT_FILL bytes (integers), pad columns C..ld and
    guard_rows rows above and below.  Returns (view, handle); view is rows x ld."""
    ld = C if ld is None else int(ld)
    assert ld >= C and guard_rows >= 0
    total = rows + 2 * guard_rows
    if dtype.is_floating_point:
        buf = torch.full((total, ld), float("nan"), dtype=dtype, device=device)
    else:
        buf = torch.full((total * ld * torch.empty(0, dtype=dtype).element_size(),), INT_FILL, dtype=torch.uint8,
                         device=device).view(dtype).reshape(total, ld)
    h = Handle(buf, rows, C, ld, guard_rows, "out")
    h.fill = _bits(buf).reshape(-1)[0].clone() if buf.numel() else None
    return h.view, h


def _first(bad):
    r, c = (int(v) for v in bad.nonzero()[0])
    return r, c, int(bad.sum())


def check_out(x):
    """The pad columns and both guard bands of a guarded output are bit-for-bit what they were."""
    h = _handle(x)
    assert h.kind == "out", "check_out on an input: use check_in"
    g, M, C = h.guard_rows, h.rows, h.C
    b = _bits(h.buf)
    bad = b[g:g + M, C:] != h.fill
    if bad.any():
        r, c, n = _first(bad)
        raise AssertionError(f"wrote outside the C columns: {n} elements, first at row {r}, column {C + c} (C = {C}, ld = {h.ld})")
    bad = b[:g] != h.fill
    if bad.any():
        r, c, n = _first(bad)
        raise AssertionError(f"wrote above row 0: {n} elements, first at row {r - g}, column {c}")
    bad = b[g + M:] != h.fill
    if bad.any():
        r, c, n = _first(bad)
        raise AssertionError(f"wrote below row M: {n} elements, first at row {M + r}, column {c} (M = {M})")


def check_written(x):
    """Every element of a guarded float output was stored (none still carries the NaN fill).  The value assertion of a test
    (close()) says the same through its finiteness check; this names the rows."""
    h = _handle(x)
    assert h.kind == "out" and h.buf.dtype.is_floating_point
    bad = _bits(h.data) == h.fill
    if bad.any():
        r, c, n = _first(bad)
        rows = bad.any(dim=1).nonzero().reshape(-1)
        raise AssertionError(f"left {n} elements unwritten, first at row {r}, column {c}; rows {int(rows[0])}..{int(rows[-1])} of {h.rows}")


def check_in(x):
    """A read-only operand, its poison included, is bit-identical after the call.  Not for operands the API documents as
    aliased with an output (in-place residuals, the in-place row kernels)."""
    h = _handle(x)
    assert h.kind in ("in", "vec"), "check_in on an output: use check_out"
    bad = _bits(h.buf) != _bits(h.snapshot)
    if bad.any():
        r, c, n = _first(bad)
        if h.kind == "vec":
            raise AssertionError(f"read-only vector operand changed: {n} elements, first at index {c - h.offset} of {h.C}")
        g = h.guard_rows
        where = ("above row 0" if r < g else "below row M" if r >= g + h.rows else
                 "in the pad columns" if c >= h.C else "inside the operand")
        raise AssertionError(f"read-only operand changed {where}: {n} elements, first at row {r - g}, column {c} "
                             f"(rows = {h.rows}, C = {h.C}, ld = {h.ld})")


def check_all(*xs):
    """check_out / check_in on each guarded buffer by its kind."""
    for x in xs:
        (check_out if _handle(x).kind == "out" else check_in)(x)
