"""GPU: what the attention kernels must reproduce EXACTLY (inputs and reasoning: tests/attn_exact.py; the same assertions
against a wrong model on the CPU: tests/test_attn_exact_host.py).  The tolerance of tests/test_hip_kernels.py::close sits an
order of magnitude above the kernels' own error; these assertions have none.

  unity       V column j holds c_j (a signed power of two) in every key row: out == c_j bit for bit, whatever Q, K and the
              mask are.  With the ones-column the numerator is exactly c_j l and c_j l fl(1 / l) is within 2^-23 of c_j; without
              it l and the numerator are two fp32 sums of the same <= 1024 non-negative terms in different orders, 1024 * 2^-23
              = 1.2e-4 apart at the most, below half an f16 ulp under a power of two (2^-12 = 2.4e-4): hence Lk <= 1024 here.
              A row sum taken from the UNROUNDED probabilities is 3e-4 too large and fails on most rows.
  selection   Q_i = t K_pi(i) over pairwise distinct +-1 keys: out[i] == V[pi(i)] bit for bit (gap >= 24 in the exponent: every
              other probability rounds to 0 in f16 even where the deferred running max of the d = 40 kernel lags by 2^6).  A
              key-index slip in a ragged tile, a V row / column permutation or an ignored mask (invisible decoys) cannot pass.
  no key      a query with no visible key yields a zero row (rcdm.h), not NaN.

Every operand sits in a guarded allocation (tests/guard.py) with four different padded row strides."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import attn_exact as X
from tests.test_hip_kernels import check_all, close, gin, gout

pytestmark = pytest.mark.gpu

B, H = X.BATCH, X.HEADS


def _rows(a):
    """[batch][L][C] float32 holding f16 values -> f16 rows [batch*L][C]."""
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, a.shape[-1]).half()


def _bits(out, C):
    return out[:, :C].contiguous().cpu().numpy()


def run_flash(q, k, v, d, valid=None, causal=False, masked=False, flags=0):
    """rcdm_flash_attn / rcdm_flash_attn_masked on q [B][Lq][C], k, v [B][Lk][C] -> out [B*Lq][C] float16 (numpy)."""
    from rcdms_amd import hip
    batch, Lq, C = q.shape
    Lk = k.shape[1]
    ldq, ldk, ldv, ldo = C + 8, C + 16, C + 24, C + 32
    qd, kd, vd = gin(_rows(q), ldq), gin(_rows(k), ldk), gin(_rows(v), ldv)
    out = gout(batch * Lq, C, ldo)
    desc = hip.AttnDesc(batch, H, Lq, Lk, d, ldq, ldk, ldv, ldo, d ** -0.5, flags)
    guarded = [out, qd, kd, vd]
    if masked:
        vm = gin(torch.from_numpy(valid), guard_rows=4) if valid is not None else None
        if vm is not None:
            guarded.append(vm)
        hip.flash_attn_masked(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), vm.data_ptr() if vm is not None else 0, causal,
                              out.data_ptr())
    else:
        hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(*guarded)
    return _bits(out, C)


def run_xattn(q, k, v, d):
    """rcdm_xattn_pack_kv + rcdm_xattn."""
    from rcdms_amd import hip
    batch, Lq, C = q.shape
    Lk = k.shape[1]
    ldq, ldk, ldv, ldo = C + 8, C + 16, C + 24, C + 32
    qd, kd, vd = gin(_rows(q), ldq), gin(_rows(k), ldk), gin(_rows(v), ldv)
    img = gout(1, hip.xattn_image_bytes(batch, H, d), dtype=torch.uint8, guard_rows=1)
    out = gout(batch * Lq, C, ldo)
    desc = hip.AttnDesc(batch, H, Lq, Lk, d, ldq, ldk, ldv, ldo, d ** -0.5)
    hip.xattn_pack_kv(kd.data_ptr(), vd.data_ptr(), batch, Lk, H, d, ldk, ldv, img.data_ptr())
    hip.xattn(desc, qd.data_ptr(), img.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, img, qd, kd, vd)
    return _bits(out, C)


def run_temporal(q, k, v, d, frames):
    """rcdm_temporal_attn on [B*pixels][frames][C] attention problems -> out in the same layout, [B*pixels*frames][C] float16."""
    from rcdms_amd import hip
    px, C = X.TEMPORAL_PIXELS, q.shape[-1]
    qkv = np.concatenate([X.temporal_rows(a, B, frames, px) for a in (q, k, v)], axis=1)
    ldqkv, ldo = 3 * C + 8, C + 24
    qkv_d = gin(torch.from_numpy(qkv).half(), ldqkv)
    out = gout(B * frames * px, C, ldo)
    desc = hip.TemporalAttnDesc(B, frames, px, H, d, ldqkv, ldo, d ** -0.5)
    hip.temporal_attn(desc, qkv_d.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    check_all(out, qkv_d)
    o = _bits(out, C)                      # rows (b, frame, pixel) -> (b, pixel, frame)
    return o.reshape(B, frames, px, C).transpose(0, 2, 1, 3).reshape(B * px * frames, C)


def _unity(entry, d, shapes, mode=None, flags=0):
    """Every (Lq, Lk) of `shapes` at both gains; all failing launches in one message."""
    failed = []
    for Lq, Lk in shapes:
        for gain in X.GAINS:
            batch = B * X.TEMPORAL_PIXELS if entry == "temporal" else B
            q, k = X.unity_qk(entry, d, Lq, Lk, mode, gain, batch=batch)
            v = X.unity_v(batch * Lk, H, d).reshape(batch, Lk, H * d)
            if entry == "xattn":
                out = run_xattn(q, k, v, d)
            elif entry == "temporal":
                out = run_temporal(q, k, v, d, Lk)
            elif entry == "masked":
                valid, causal = X.unity_mask(d, Lk, mode)
                out = run_flash(q, k, v, d, valid, causal, masked=True)
            else:
                out = run_flash(q, k, v, d, flags=flags)
            n = X.unity_mismatches(out, H, d)
            print(f"unity {entry} d={d} Lq={Lq} Lk={Lk} mask={mode} gain={gain} flags={flags}: {n} / {out.size} elements differ from c_j")
            if n:
                bad = out.view(np.uint16) != np.tile(X.unity_column(d), H).astype(np.float16).view(np.uint16)[None, :]
                r, c = (int(x) for x in np.argwhere(bad)[0])
                failed.append(f"Lq={Lq} Lk={Lk} gain={gain}: {n} / {out.size} elements, first at row {r}, column {c}: "
                              f"{float(out[r, c])!r} for {float(np.tile(X.unity_column(d), H)[c])!r}")
    assert not failed, f"{entry} d={d} mask={mode}: out != c_j in " + "; ".join(failed)


# ---- (a) partition of unity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", X.FLASH_D)
def test_unity_flash(hiplib, d):
    """Every instantiation of flash_attn_kernel; Lk = 85: a ragged second tile, Lk = 320: five tiles (d = 40: the MSUB kernel)."""
    _unity("flash", d, [(X.FLASH_LQ, lk) for lk in X.FLASH_LK])


def test_unity_flash_d40_wide_range(hiplib):
    """d = 40, Lk = 320 once more with RCDM_ATTN_WIDE_RANGE: the fma-softmax kernel where the launch above took MSUB."""
    from rcdms_amd import hip
    _unity("flash", 40, [(X.FLASH_LQ, 320)], flags=hip.ATTN_WIDE_RANGE)


@pytest.mark.parametrize("d", X.FALLBACK_D)
def test_unity_flash_no_spare_column(hiplib, d):
    """d = 32 and d = 160, the head dims with no spare column for the ones-row: one key, both sides of the 64-key tile, 16 tiles."""
    _unity("flash", d, [(lq, lk) for lk in X.FALLBACK_LK for lq in X.FALLBACK_LQ])


@pytest.mark.parametrize("mode", X.MASKED_MODES)
@pytest.mark.parametrize("d", X.MASKED_D)
def test_unity_flash_masked(hiplib, d, mode):
    _unity("masked", d, [(L, L) for L in X.MASKED_L], mode=mode)


@pytest.mark.parametrize("d", [40, 64, 160])
def test_unity_flash_masked_first_tile_hidden_scores_far_below_zero(hiplib, d):
    """Softmax does not change when every score of a row moves by the same amount.  Here every scaled score is far below zero
    (-30 and less in the exponent of 2, inside the documented range) and padding hides the whole first 64-key tile of batch
    entry 1: the running max of a query has to start at its first VISIBLE score.  Started at 0 — a max the row never had —
    every probability underflows f16 and the row comes back 0 instead of c_j."""
    L = 150
    g = np.random.default_rng([31, d])
    q = -np.abs(X.f16(16 * g.standard_normal((B, L, H * d))).astype(np.float32))
    k = np.abs(X.f16(g.standard_normal((B, L, H * d))).astype(np.float32))
    v = X.unity_v(B * L, H, d).reshape(B, L, H * d)
    valid, causal = X.unity_mask(d, L, "pad")
    assert not valid[1, :64].any() and not causal
    top = max(float((q[b][:, h * d:(h + 1) * d].astype(np.float64) @ k[b][:, h * d:(h + 1) * d].astype(np.float64).T).max())
              for b in range(B) for h in range(H)) * d ** -0.5 * X.LOG2E
    low = -float(np.abs(q).max() * np.abs(k).max()) * d ** 0.5 * X.LOG2E
    assert top < -30 and low > -2 ** 15, (top, low)
    out = run_flash(q, k, v, d, valid, causal, masked=True)
    n = X.unity_mismatches(out, H, d)
    rows0 = int((out.view(np.uint16) & 0x7FFF == 0).all(axis=1).sum())
    assert n == 0, f"d={d}: {n} / {out.size} elements differ from c_j ({rows0} whole rows are 0.0); largest scaled score 2^{top:.0f}"


@pytest.mark.parametrize("d", X.XATTN_D)
def test_unity_xattn(hiplib, d):
    """Lq = 300: several query chunks per block."""
    _unity("xattn", d, [(lq, lk) for lk in X.XATTN_LK for lq in X.XATTN_LQ])


@pytest.mark.parametrize("d", X.WIDE_D)
def test_unity_flash_wide_heads(hiplib, d):
    _unity("wide", d, [(X.WIDE_LQ, lk) for lk in X.WIDE_LK])


@pytest.mark.parametrize("d", X.TEMPORAL_D)
def test_unity_temporal(hiplib, d):
    _unity("temporal", d, [(f, f) for f in X.TEMPORAL_FRAMES])


# ---- (b) selection -----------------------------------------------------------------------------------------------------------
def _selected(name, out, v, d, pi, q, k, valid=None, causal=False):
    gap = X.selection_gap(q, k, H, d, pi, valid, causal)
    assert gap >= X.MIN_GAP, f"{name}: score gap {gap} (float64) before the launch"
    want = X.selection_expected(v, H, d, pi)
    bad = out.view(np.uint16) != want.view(np.uint16)
    if bad.any():
        r, c = (int(x) for x in np.argwhere(bad)[0])
        L = pi.shape[2]
        raise AssertionError(f"{name}: out != V[pi]: {int(bad.sum())} / {bad.size} elements in {int(bad.any(axis=1).sum())} rows, first at "
                             f"batch {r // L}, query {r % L}, column {c} (pi = {int(pi[r // L, c // d, r % L])}): {float(out[r, c])!r} "
                             f"for {float(want[r, c])!r}")


@pytest.mark.parametrize("d,Lq,Lk", X.SEL_FLASH)
def test_selection_flash(hiplib, d, Lq, Lk):
    q, k, v, pi = X.sel_case("flash", d, Lq, Lk)
    _selected(f"flash d={d} Lq={Lq} Lk={Lk}", run_flash(q, k, v, d), v, d, pi, q, k)


@pytest.mark.parametrize("d,Lq,Lk", X.SEL_XATTN)
def test_selection_xattn(hiplib, d, Lq, Lk):
    q, k, v, pi = X.sel_case("xattn", d, Lq, Lk)
    assert all(len(set((pi[b, h] // 32).tolist())) == (Lk + 31) // 32 for b in range(B) for h in range(H))   # every 32-key tile
    _selected(f"xattn d={d} Lq={Lq} Lk={Lk}", run_xattn(q, k, v, d), v, d, pi, q, k)


@pytest.mark.parametrize("d,Lq,Lk", X.SEL_WIDE)
def test_selection_flash_wide_heads(hiplib, d, Lq, Lk):
    """A key selected in a late tile leaves the first-tile window of attn_wide.hip by far: the second pass, too."""
    q, k, v, pi = X.sel_case("wide", d, Lq, Lk)
    _selected(f"wide d={d} Lq={Lq} Lk={Lk}", run_flash(q, k, v, d), v, d, pi, q, k)


@pytest.mark.parametrize("d,frames", X.SEL_TEMPORAL)
def test_selection_temporal(hiplib, d, frames):
    q, k, v, pi = X.sel_temporal_case(d, frames)
    _selected(f"temporal d={d} frames={frames}", run_temporal(q, k, v, d, frames), v, d, pi, q, k)


@pytest.mark.parametrize("d,L,pad,causal", X.SEL_MASKED)
def test_selection_flash_masked_with_invisible_decoys(hiplib, d, L, pad, causal):
    """pi(i) is visible; an exact copy of K_pi(i) with another V row sits where the mask hides it (a padded position, behind the
    query under a causal mask): a kernel that ignores the mask returns the mean of the two rows."""
    q, k, v, valid, pi, planted = X.sel_masked_case(d, L, pad, causal)
    assert planted.mean() > 0.25
    out = run_flash(q, k, v, d, valid, causal, masked=True)
    _selected(f"masked d={d} L={L} pad={pad} causal={causal}", out, v, d, pi, q, k, valid, causal)


# ---- (c) rows with no visible key ----------------------------------------------------------------------------------------
def _random_qkv(seed, L, d):
    g = np.random.default_rng(seed)
    return tuple(X.f16(g.standard_normal((B, L, H * d))).astype(np.float32) for _ in range(3))


def _oracle(q, k, v, valid, causal):
    L = q.shape[1]
    add = (1.0 - torch.from_numpy(valid).float())[:, None, :] * -10000.0
    add = add + torch.full((L, L), -10000.0).triu_(1)[None] if causal else add.expand(B, L, L)
    return O.attention_core(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), H, mask=add)


@pytest.mark.parametrize("d", [64, 160])
def test_batch_entry_with_every_key_padded_gives_zero_rows(hiplib, d):
    """key_valid all zero for batch entry 0, not causal: its rows are exactly 0.0 (not NaN); entry 1 is ordinary attention."""
    L = 97
    q, k, v = _random_qkv([21, d], L, d)
    valid = np.ones((B, L), dtype=np.uint8)
    valid[0, :] = 0
    valid[1, 30:70] = 0
    out = run_flash(q, k, v, d, valid, False, masked=True)
    assert (out[:L].view(np.uint16) & 0x7FFF == 0).all(), f"{int((out[:L].view(np.uint16) & 0x7FFF != 0).sum())} elements of the all-padded batch entry are not 0.0"
    ref = _oracle(q, k, v, valid, False)
    close(torch.from_numpy(out[L:].astype(np.float32)), ref[1].reshape(L, H * d))


@pytest.mark.parametrize("d", [64, 160])
def test_causal_queries_in_front_of_the_first_valid_key_give_zero_rows(hiplib, d):
    """Keys 0 .. 2 padded out under a causal mask: queries 0 .. 2 see nothing (zero rows), query 3 sees key 3 alone (exactly V[3]),
    the rest is ordinary attention."""
    L = 97
    q, k, v = _random_qkv([22, d], L, d)
    valid = np.ones((B, L), dtype=np.uint8)
    valid[:, :3] = 0
    valid[1, 40:60] = 0
    out = run_flash(q, k, v, d, valid, True, masked=True).reshape(B, L, H * d)
    assert (out[:, :3].view(np.uint16) & 0x7FFF == 0).all(), "queries 0 .. 2 have no visible key: zero rows"
    assert np.array_equal(out[:, 3].view(np.uint16), v[:, 3].astype(np.float16).view(np.uint16)), "query 3 sees key 3 alone: V[3]"
    ref = _oracle(q, k, v, valid, True)
    close(torch.from_numpy(out[:, 3:].astype(np.float32)), ref[:, 3:])
