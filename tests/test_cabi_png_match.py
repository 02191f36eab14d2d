"""CPU: the match-mode PNG entry points are declared, exported and bound, and rcdm_png_encode_match refuses what
rcdm_png_encode refuses, with the same codes, before anything is launched (no device is touched: the pointers are never
dereferenced, and on a box without a GPU a launch would come back as RCDM_ELAUNCH, not as the code asserted here)."""
import ctypes

from tests.test_cabi_symbols import declared_symbols

EINVAL, ESHAPE = -1, -2


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in ("rcdm_png_encode_match", "rcdm_png_match_workspace_bytes"):
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)


def test_workspace_and_bound_serve_both_modes():
    hip, lib = _lib()
    for n, h, w in ((1, 1, 1), (5, 105, 107), (1, 1024, 2560), (3, 2, 8192)):
        d = hip.PngDesc(3 * w, 3 * w * h, 0, n, h, w, 3, -1)
        assert hip.png_match_workspace_bytes(d) == hip.png_workspace_bytes(d) > 0 and hip.png_bound(d) > 0
    assert lib.rcdm_png_match_workspace_bytes(None) == 0
    assert hip.png_match_workspace_bytes(hip.PngDesc(15, 0, 0, 1, 5, 5, 4, -1)) == 0
    assert hip.png_match_workspace_bytes(hip.PngDesc(15, 0, 0, 1, 5, 8193, 3, -1)) == 0


def test_encode_match_argument_checks():
    hip, lib = _lib()
    h, w = 3, 5
    good = lambda: hip.PngDesc(3 * w, 3 * w * h, 0, 1, h, w, 3, -1)
    src, ws, dst, sizes = 0x1000, 0x2000, 0x3000, 0x4000     # never dereferenced
    call = lambda d, *p: lib.rcdm_png_encode_match(ctypes.byref(d) if d is not None else None, *p, None)
    assert call(None, src, ws, dst, sizes) == EINVAL
    for k in range(4):                                       # each null pointer
        p = [src, ws, dst, sizes]
        p[k] = None
        assert call(good(), *p) == EINVAL, k
    d = good()
    d.n, d.dst_stride = 2, hip.png_bound(good()) - 1          # a short dst_stride with n > 1
    assert call(d, src, ws, dst, sizes) == EINVAL
    assert call(good(), src, ws + 8, dst, sizes) == EINVAL    # a misaligned workspace
    assert call(good(), src, ws, dst, sizes + 4) == EINVAL    # misaligned sizes
    d = good()
    d.channels = 4
    assert call(d, src, ws, dst, sizes) == EINVAL
    d = good()
    d.filter = 5
    assert call(d, src, ws, dst, sizes) == EINVAL
    d = good()
    d.src_pitch = 3 * w - 1
    assert call(d, src, ws, dst, sizes) == EINVAL
    d = good()
    d.w = 8193
    d.src_pitch = 3 * d.w
    assert call(d, src, ws, dst, sizes) == ESHAPE
    d = good()
    d.n = 65536
    assert call(d, src, ws, dst, sizes) == ESHAPE
    # the same calls on the literal-only entry give the same codes
    d = good()
    d.channels = 4
    assert lib.rcdm_png_encode(ctypes.byref(d), src, ws, dst, sizes, None) == EINVAL
