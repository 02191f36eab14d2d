"""GPU: every launch-plan form of the UNet at the REAL widths, on a probe small enough to run in seconds.

The probe (mirrored("unet_probe"), oracle/make_golden.py --only probe) is UNet3DConditionModel with two levels, 320 channels
(head dim 40: row chains, rcdm_ff_fused, the conv_out tap planes, the stride-2 downsample) and 640 channels (head dim 80:
Winograd at sides 8..32, the nine-plane upsample, shortcut folds at 1280 -> 640 and 960 -> 320), one layer per block,
cross-attention everywhere: 136.3 M parameters.  Which form a site takes depends on its width, on its row count against
emit_blocks.CHAIN_MIN_ROWS (30720 on MI355X: lowered here so that a few thousand rows take the chain forms) and on the
switches of rcdms_amd/switches.py, whose "0" sides are also the fall-backs a shape takes on its own.  Every case

  * runs once eager and once as the hipGraph replay (bit-equal),
  * compares with the reference's fp32 output on the same procedural weights (tests/golden/unet_probe_<geometry>.npz),
  * asserts FROM THE PLAN'S TAGS that the intended form was taken — a silently taken fall-back would make the case vacuous.

Tolerance.  Measured on MI355X, default plan against the reference (rel-RMS / max-abs over max|ref|):
    A (2, 5, 16x16)  1.61e-3 / 2.04e-3        B (1, 3, 16x24)  1.65e-3 / 1.75e-3
    C (1, 2, 32x32)  1.83e-3 / 2.19e-3        D (2, 5, 8x16)   1.58e-3 / 1.52e-3
    E (2, 5, 32x32)  1.61e-3 / 2.03e-3        the motion_module_resolutions=(1, 2) config on B's geometry: 1.86e-3 / 2.03e-3
The bound of a geometry (TOL) is the project's rule — <= 2x what its default plan measures, so that a doubling fails — and lies
under the whole-UNet bound of test_hip_unet.py (rel-RMS 4e-3, max 6e-3 of max|ref|), the ceiling.  Every switch variant, the
shared-prefix plan and the moved thresholds meet the bound of their geometry; measured, they stay within 5 % (rel-RMS) / 12 %
(max) of the default plan's error: 1.58e-3 .. 1.70e-3 on A, 1.83e-3 .. 1.87e-3 on C.  Each prints its error beside the default's.

The program cache of a model is keyed by geometry only, so every switch / threshold setting builds a fresh model; the
state dict is generated once per module."""
import re

import pytest
import torch

from rcdms_amd import emit_blocks, synth
from rcdms_amd import switches as SW
from tests.test_hip_unet import DEV, check, rel_rms
from tests.test_oracle_golden import SEEDS, gold, mirrored, shapes_of

pytestmark = pytest.mark.gpu

# golden name -> (rel-RMS, max-abs / max|ref|): <= 2x the default plan's measurement (module docstring)
TOL = {"unet_probe_a": (3.2e-3, 4.0e-3), "unet_probe_b": (3.3e-3, 3.5e-3), "unet_probe_c": (3.6e-3, 4.3e-3),
       "unet_probe_d": (3.1e-3, 3.0e-3), "unet_probe_mm12": (3.7e-3, 4.0e-3), "unet_probe_e": (3.2e-3, 4.0e-3)}
assert all(r <= 4e-3 and m <= 6e-3 for r, m in TOL.values())
L = 13

# name: (b, f, H, W, chain threshold) — the threshold puts level 0 (320 channels) exactly at the chain kernels' row count
GEO = {"a": (2, 5, 16, 16, 2560), "b": (1, 3, 16, 24, 1152), "c": (1, 2, 32, 32, 2048), "d": (2, 5, 8, 16, 1280),
       "e": (2, 5, 32, 32, 10240)}

FORMS = {
    "rowchain": r"^rowchain ", "chain_gn": r"^rowchain .* gn=1$", "chain_pe": r"^rowchain .* pe=1 ",
    "chain_tail0": r"^rowchain .* tail=0 ", "chain_tail1": r"^rowchain .* tail=1 ", "chain_tail2": r"^rowchain .* tail=2 ",
    "chain_tail3": r"^rowchain .* tail=3 ",
    "ff_fused": r"^ff_fused ", "layernorm": r"^layernorm ", "ln_pe": r"^layernorm .* pe=1$", "lnx": r" lnx( |$)", "stat": r" stat( |$)",
    "gemm": r"^gemm ", "geglu": r"^gemm .* epi=(8|9)( |$)",
    "wino": r"^conv3x3_wino ", "wino_gn": r"^conv3x3_wino .* gn( |$)", "wino_sc": r"^conv3x3_wino .* add1x1=",
    "fold": r"^conv3x3 .* add1x1=", "nine_tap": r"^conv3x3 .* s=1 up=0 ",
    "up9": r"^upsample_gather ", "up_phase": r"^conv3x3 .* up=2 ", "up_taps": r"^conv3x3 .* up=1 ",
    "out_taps": r"^conv_gather ", "out_conv": r"^conv3x3 .*->8 ",
    "gnstat": r" gnstat( |$)", "prestat": r" prestat( |$)", "gn_stats": r"^groupnorm_stats ", "gn_per_frame": r"^groupnorm .* silu=0( |$)",
    "temporal": r"^temporal_attn ", "xattn": r"^xattn ", "flash": r"^flash_attn ",
}


def forms(tags):
    """Count of the plan's tags per form (FORMS), plus "ffz": GEMMs with K = 5 N, the composed [W_po W_ff2 | W_po] product."""
    out = {k: sum(1 for t in tags if re.search(p, t)) for k, p in FORMS.items()}
    out["ffz"] = sum(1 for t in tags for m in [re.match(r"gemm M=\d+ N=(\d+) K=(\d+) ", t)] if m and int(m[2]) == 5 * int(m[1]))
    return out


def expect(tags, **want):
    got = forms(tags)
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"plan forms (got, expected): {bad}\n" + "\n".join(tags)
    return got


def fold_widths(tags, kind="conv3x3 "):
    return [int(t.split("add1x1=")[1].split()[0]) for t in tags if t.startswith(kind) and " add1x1=" in t]


_SD = {}
ERR = {}    # (geometry, variant) -> (rel-RMS, max / max|ref|) of the cases run so far: a variant prints the default's beside its own


def fresh_model(kind="unet_probe"):
    """A NEW model object (no cached launch plan) holding the module-wide procedural state dict."""
    if kind not in _SD:
        _SD[kind] = synth.procedural_state_dict(shapes_of(mirrored(kind)), SEEDS[kind])
    m = mirrored(kind).to_empty(device="cpu")
    m.load_state_dict(_SD[kind])
    return m.to(DEV).eval()


def run_case(monkeypatch, geo, variant="default", threshold="geo", shared=False, kind="unet_probe", golden=None, **switches):
    """Build a fresh model under the given switches / chain threshold, run geometry `geo` eager + replayed, check both against
    the golden; returns (tags, program)."""
    b, f, H, W, thr = GEO[geo]
    for k, v in switches.items():
        assert hasattr(SW, k), k
        monkeypatch.setattr(SW, k, v)
    if threshold is not None:
        monkeypatch.setattr(emit_blocks.CHAIN_MIN_ROWS, "_v", thr if threshold == "geo" else threshold)
    golden = golden or f"unet_probe_{geo}"
    g = gold(golden)
    if "x" not in g:    # (outputs only: the inputs are the fixture's synthetic story, assembled as the CFG step does)
        st = synth.synthetic_story(stories=1, latent_hw=(H, W), ctx_len=L, ctx_dim=64, seed=int(g["story_seed"]))
        g = dict(g, x=torch.cat([torch.cat([st["latents"]] * 2), st["mask"], st["masked_latents"]], dim=1), ctx=st["ctx"])
    assert tuple(g["x"].shape) == (b, 9, f, H, W) and tuple(g["ctx"].shape) == (b * f, L, 64)
    m = fresh_model(kind)
    x, ctx, t = g["x"].to(DEV), g["ctx"].to(DEV), torch.tensor(g["t"])
    with torch.no_grad():
        if shared:
            assert torch.equal(g["x"][: b // 2], g["x"][b // 2:]) and not torch.equal(g["ctx"][: b * f // 2], g["ctx"][b * f // 2:])
            prog = m.program(b, f, H, W, L, shared_prefix=True)
            y = prog.forward(x, t, ctx).clone()
            y2 = prog.forward(x, t, ctx)
        else:
            y = m(x, t, ctx, return_dict=False)[0].clone()
            y2 = m(x, t, ctx)
            prog = m.program(b, f, H, W, L)
    assert prog.calls == 2 and prog.graph is not None, "the second call did not replay the captured graph of this plan"
    assert prog.shared_prefix is shared
    what = f"probe {geo} [{variant}]"
    got, ref = y.float().cpu(), g["y"]
    ERR[(geo, variant)] = (rel_rms(got, ref), ((got - ref).abs().max() / ref.abs().max()).item())
    d = ERR.get((geo, "default"))
    if d is not None and variant != "default":
        print(f"probe {geo} [default]: rel-RMS {d[0]:.3e}  max-abs/max|ref| {d[1]:.3e}   <- the default plan, for comparison")
    check(y, ref, *TOL[golden], what)
    assert torch.equal(y, y2), f"{what}: graph replay differs from the eager launch sequence"
    return prog.plan.tags, prog


# what every plan of the probe has whatever the switches: 7 spatial transformers (3 at level 0), 6 motion modules x 2 attentions
SITES = dict(flash=7, xattn=7, temporal=12)
# geometry A's default plan: 3 layers of level 0 chained (3 transformer + 3 motion chains each), level 1 on the deferred forms
A_DEFAULT = dict(SITES, rowchain=18, chain_gn=6, chain_pe=6, chain_tail0=0, chain_tail1=3, chain_tail2=6, chain_tail3=9, ff_fused=0,
                 layernorm=0, lnx=21, stat=21, ffz=7, gemm=51, wino=6, wino_gn=6, wino_sc=0, fold=5, up9=1, up_phase=0, up_taps=0,
                 out_taps=1, out_conv=0)


# ---- geometries, default switches ------------------------------------------------------------------------------------------

def test_geometry_a_chains_with_groupnorm_prologue_wino8_up9(hiplib, monkeypatch):
    """(2, 5, 16x16), threshold 2560.  Level 0 (M = 2560, hw = 256 >= 160): every transformer and motion module on the row
    chains, the per-frame GroupNorm as a statistics launch whose apply rides in the first chain (gn=1), positional rows in the
    two temporal chains (pe=1), the feed-forward + proj_out inside the tail-2 chains (no rcdm_ff_fused launch, no LayerNorm
    launch).  Level 1 (M = 640): deferred LayerNorms (3 consumers per transformer / motion module), composed proj_out (K = 5C).
    Winograd 8x8 on the mid ResNets and the up block's conv1 (a conv2 with a shortcut keeps nine taps below side 16); shortcut
    folds at 320, 1280, 960 (640 wide) and 960, 640 (320 wide); nine-plane upsample at 640; conv_out as tap planes."""
    tags, prog = run_case(monkeypatch, "a")
    got = expect(tags, **A_DEFAULT)
    assert all(t.startswith("rowchain M=2560 C=320 ") for t in tags if t.startswith("rowchain "))
    assert sum(t == "groupnorm_stats S=10 R=256 C=320" for t in tags) == 6          # the chains' GroupNorm prologues
    assert got["gn_per_frame"] == 7 and all("C=640" in t for t in tags if re.search(FORMS["gn_per_frame"], t))
    assert [t.split()[1:3] for t in tags if t.startswith("conv3x3_wino ")] == \
        [["10x8x8", "640->640"]] * 4 + [["10x8x8", "1280->640"], ["10x8x8", "960->640"]]
    assert fold_widths(tags) == [320, 1280, 960, 960, 640] and "res_sc" not in prog.plan.bufs
    assert "upsample_gather 10x8x8 C=640" in tags and "conv_gather 10x16x16 C=8" in tags
    assert "conv3x3 10x16x16 320->320 s=2 up=0 epi=1" in tags                                  # the stride-2 downsample
    assert got["gnstat"] > 0 and got["gnstat"] == got["prestat"]                          # every statistics hand-off is taken


def test_geometry_a_shared_prefix(hiplib, monkeypatch):
    """The same inputs (two identical samples, different context rows) through program(..., shared_prefix=True): conv_in, the
    first ResNet block and the first transformer up to the cross-attention query run on HALF the batch (5 images, M = 1280) and
    store to both halves (dup_rows); that transformer leaves the first two chains (16 chain launches instead of 18) and, its half
    being below the threshold, defers its norm1 / norm2 (2 more consumers)."""
    tags, prog = run_case(monkeypatch, "a", "shared", shared=True)
    expect(tags, **dict(A_DEFAULT, rowchain=16, chain_gn=5, chain_tail1=2, chain_tail3=8, lnx=23, stat=23, gemm=55))
    assert tags[4] == "conv3x3 5x16x16 64->320 s=1 up=0 epi=1"                       # conv_in behind the 4 time-embedding ops
    assert sum(t.startswith("conv3x3 5x16x16 320->320 ") for t in tags) == 2
    assert "groupnorm S=5 R=256 C=320 silu=0" in tags and "flash_attn B=5 H=8 Lq=256 Lk=256 d=40" in tags
    assert sum(t.startswith("gemm M=1280 N=960 K=320 ") and " lnx" in t for t in tags) == 1
    assert sum(t.startswith("xattn B=10 ") for t in tags) == 7                        # the cross-attention sees the whole batch


def test_geometry_a_device_threshold_every_level_small(hiplib, monkeypatch):
    """The threshold as the device sets it (3/4 of the CUs x 160 rows): the 2560 rows of level 0 are far below it, so BOTH real
    widths run the tile-parallel forms — deferred LayerNorms and the composed proj_out at 320 channels too, no chain."""
    assert int(emit_blocks.CHAIN_MIN_ROWS) > 2560, "RCDM_CHAIN_MIN_ROWS overridden"
    tags, _ = run_case(monkeypatch, "a", "device threshold", threshold=None)
    expect(tags, **dict(A_DEFAULT, rowchain=0, chain_gn=0, chain_pe=0, chain_tail1=0, chain_tail2=0, chain_tail3=0, lnx=39, stat=39,
                        ffz=13, gemm=93, layernorm=0, ff_fused=0))
    assert sum(t == "groupnorm S=10 R=256 C=320 silu=0" for t in tags) == 6
    assert sum(t.startswith("gemm M=2560 N=320 K=1600 ") for t in tags) == 6


def test_geometry_a_big_path_at_640(hiplib, monkeypatch):
    """Threshold 160: level 1 (M = 640, 640 channels) is at the chain kernels' row count but has no chain kernel — the path the
    640-channel level of a 1024x1024 image takes: stand-alone LayerNorms (3 per transformer, 3 per motion module, the temporal
    ones with the positional rows), plain GEGLU + ff.net.2 + proj_out GEMMs, no deferred form, no composed product."""
    tags, _ = run_case(monkeypatch, "a", "big640", threshold=160)
    expect(tags, **dict(A_DEFAULT, lnx=0, stat=0, ffz=0, layernorm=21, ln_pe=6, gemm=58, geglu=7))
    assert all(t.startswith("layernorm M=640 C=640 ") for t in tags if t.startswith("layernorm "))
    assert sum(t.startswith("gemm M=640 N=640 K=2560 ") for t in tags) == 7          # ff.net.2 on its own


def test_geometry_b_non_square_odd_batch_three_frames(hiplib, monkeypatch):
    """(1, 3, 16x24), threshold 1152: one sample, 3 of the 5 positional rows (chains at level 0, the per-frame row table at level
    1), 16x24 / 8x12 images through the convolutions, Winograd at 8x12, the gathers."""
    tags, _ = run_case(monkeypatch, "b")
    expect(tags, **A_DEFAULT)
    assert all(t.startswith("rowchain M=1152 C=320 ") for t in tags if t.startswith("rowchain "))
    assert sum(t == "temporal_attn S=1 F=3 P=384 H=8 d=40" for t in tags) == 6
    assert sum(t == "temporal_attn S=1 F=3 P=96 H=8 d=80" for t in tags) == 6
    assert sum(t.startswith("conv3x3_wino 3x8x12 ") for t in tags) == 6
    assert "upsample_gather 3x8x12 C=640" in tags and "conv_gather 3x16x24 C=8" in tags


def test_geometry_c_wino_conv2_carries_the_shortcut(hiplib, monkeypatch):
    """(1, 2, 32x32), threshold 2048: level 1 at 16x16 = WINO_SHORTCUT_MIN_SIDE — the three width-changing blocks of level 1 run
    conv2 as a Winograd conv with the conv_shortcut as parity GEMMs (add1x1 = 320, 1280, 960); only the 320-wide folds stay on
    nine taps.  9 Winograd launches: conv2 of 320 -> 640, both convs of the mid ResNets, both convs of the two up ResNets."""
    assert emit_blocks.WINO_SHORTCUT_MIN_SIDE == 16
    tags, prog = run_case(monkeypatch, "c")
    expect(tags, **dict(A_DEFAULT, wino=9, wino_gn=9, wino_sc=3, fold=2))
    assert fold_widths(tags, "conv3x3_wino ") == [320, 1280, 960] and fold_widths(tags) == [960, 640]
    assert all(t.startswith("conv3x3_wino 2x16x16 ") for t in tags if t.startswith("conv3x3_wino "))
    assert "conv3x3 2x16x16 320->640 s=1 up=0 epi=3 gnstat" in tags or "conv3x3 2x16x16 320->640 s=1 up=0 epi=3" in tags
    assert "res_sc" not in prog.plan.bufs


def test_geometry_d_chains_with_launched_groupnorm_no_wino(hiplib, monkeypatch):
    """(2, 5, 8x16), threshold 1280: chains with hw = 128 < 160 — the per-frame GroupNorm is LAUNCHED in full and the chains read
    normalised rows (gn=0 everywhere); level 1 at 4x8 is below WINO_MIN_SIDE: every 3x3 conv on nine taps."""
    tags, _ = run_case(monkeypatch, "d")
    expect(tags, **dict(A_DEFAULT, chain_gn=0, wino=0, wino_gn=0, gn_stats=0))
    assert sum(t == "groupnorm S=10 R=128 C=320 silu=0" for t in tags) == 6
    assert sum(t.startswith("conv3x3 10x4x8 ") and " s=1 up=0 " in t for t in tags) == 10
    assert fold_widths(tags) == [320, 1280, 960, 960, 640]


def test_geometry_e_ten_images_at_16x16(hiplib, monkeypatch):
    """(2, 5, 32x32), threshold 10240: the level shapes of a 256x256 story at the real widths — 64 chain blocks at level 0, ten
    16x16 images at level 1 (Winograd conv2 with its shortcut, per-tile GroupNorm partials across five frames).  The default
    plan of the geometry whose 640-channel upsampler is large enough for the four-phase form (next test)."""
    tags, _ = run_case(monkeypatch, "e")
    expect(tags, **dict(A_DEFAULT, wino=9, wino_gn=9, wino_sc=3, fold=2))
    assert all(t.startswith("rowchain M=10240 C=320 ") for t in tags if t.startswith("rowchain "))
    assert "upsample_gather 10x16x16 C=640" in tags


def test_switch_up9_off_phase_form_at_640(hiplib, monkeypatch):
    """UP9=False where the library takes the phase form (rcdm_conv3x3_up2_supported needs the four 2x2 phase convolutions to
    fill the chip: 2560 source pixels at 640 channels do, the 512 / 640 of geometries C / A do not)."""
    tags, _ = run_case(monkeypatch, "e", "UP9=0", UP9=False)
    expect(tags, **dict(A_DEFAULT, wino=9, wino_gn=9, wino_sc=3, fold=2, up9=0, up_phase=1, up_taps=0, gemm=50))
    assert "conv3x3 10x16x16 640->640 s=1 up=2 epi=1" in tags


# ---- switch sides on geometry A (and C for the Winograd / upsample / shortcut switches) ----------------------------------------

def test_switch_row_chain_off(hiplib, monkeypatch):
    """ROW_CHAIN=False: level 0 keeps its row count (>= threshold) but launches separately — LayerNorm launches (norm1, norm2 of
    3 transformers; the two positional norms of 3 motion modules), the feed-forward as rcdm_ff_fused (6), proj_out on its own."""
    tags, _ = run_case(monkeypatch, "a", "ROW_CHAIN=0", ROW_CHAIN=False)
    expect(tags, **dict(A_DEFAULT, rowchain=0, chain_gn=0, chain_pe=0, chain_tail1=0, chain_tail2=0, chain_tail3=0, ff_fused=6,
                        layernorm=12, ln_pe=6, gemm=87))
    assert all(t.startswith("layernorm M=2560 C=320 ") for t in tags if t.startswith("layernorm "))
    assert all(t == "ff_fused M=2560 C=320" for t in tags if t.startswith("ff_fused "))


def test_switch_ff_fuse_off(hiplib, monkeypatch):
    """FF_FUSE=False.  With the chains on the switch is never consulted (the feed-forward rides in the tail-2 chains): the plan
    is the default one, tag for tag."""
    tags, _ = run_case(monkeypatch, "a", "FF_FUSE=0", FF_FUSE=False)
    expect(tags, **A_DEFAULT)


def test_switch_ff_fuse_off_without_chains(hiplib, monkeypatch):
    """... so its "0" side is reached with ROW_CHAIN=False beside it: LayerNorm -> GEGLU -> ff.net.2 as three launches at level 0
    (6 more LayerNorms, 6 more GEGLU GEMMs, no rcdm_ff_fused)."""
    tags, _ = run_case(monkeypatch, "a", "ROW_CHAIN=0 FF_FUSE=0", ROW_CHAIN=False, FF_FUSE=False)
    expect(tags, **dict(A_DEFAULT, rowchain=0, chain_gn=0, chain_pe=0, chain_tail1=0, chain_tail2=0, chain_tail3=0, ff_fused=0,
                        layernorm=18, ln_pe=6, gemm=99, geglu=13))


def test_switch_lnx_off(hiplib, monkeypatch):
    """LNX=False: the 21 deferred LayerNorms of level 1 become stand-alone launches (what a shape takes when gemm_lnx_ok refuses),
    no statistics-producing GEMM is left; the composed proj_out stays."""
    tags, _ = run_case(monkeypatch, "a", "LNX=0", LNX=False)
    expect(tags, **dict(A_DEFAULT, lnx=0, stat=0, layernorm=21, ln_pe=6))


def test_switch_ffz_off(hiplib, monkeypatch):
    """FFZ=False: ff.net.2 and proj_out as two GEMMs at level 1 (7 sites: no K = 5C product, 7 more GEMMs)."""
    tags, _ = run_case(monkeypatch, "a", "FFZ=0", FFZ=False)
    expect(tags, **dict(A_DEFAULT, ffz=0, gemm=58))


def test_switch_gn_prestat_off(hiplib, monkeypatch):
    """GN_PRESTAT=False: no producer leaves GroupNorm statistics and no norm runs its prestat form."""
    tags, _ = run_case(monkeypatch, "a", "GN_PRESTAT=0", GN_PRESTAT=False)
    expect(tags, **dict(A_DEFAULT, gnstat=0, prestat=0))


def test_switch_gn_prestat_off_wino16(hiplib, monkeypatch):
    """... and on geometry C, where the Winograd output transforms hand per-tile partials on."""
    tags, _ = run_case(monkeypatch, "c", "GN_PRESTAT=0", GN_PRESTAT=False)
    expect(tags, **dict(A_DEFAULT, wino=9, wino_gn=9, wino_sc=3, fold=2, gnstat=0, prestat=0))


def test_switch_sc_fold_off(hiplib, monkeypatch):
    """SC_FOLD=False (what a width not divisible by 64 takes): all five conv_shortcuts as their own 1x1 GEMM, read back as conv2's
    residual — also behind a Winograd conv1 (the two 8x8 up ResNets)."""
    tags, prog = run_case(monkeypatch, "a", "SC_FOLD=0", SC_FOLD=False)
    expect(tags, **dict(A_DEFAULT, fold=0, gemm=56))
    assert "res_sc" in prog.plan.bufs
    sc = [m.groups() for t in tags for m in [re.match(r"gemm M=(\d+) N=(\d+) K=(\d+) epi=1$", t)] if m and m[2] != m[3]]
    assert sc == [("640", "640", "320"), ("640", "640", "1280"), ("640", "640", "960"), ("2560", "320", "960"), ("2560", "320", "640")]
    assert sum(t.startswith("conv3x3 10x8x8 640->640 s=1 up=0 epi=5") for t in tags) == 3   # conv2 + residual, three 640-wide blocks


def test_switch_sc_fold_off_wino16(hiplib, monkeypatch):
    """SC_FOLD=False on geometry C: the Winograd conv2 keeps its shortcut (parity GEMMs are not the fold), the 320-wide blocks
    unfold."""
    tags, prog = run_case(monkeypatch, "c", "SC_FOLD=0", SC_FOLD=False)
    expect(tags, **dict(A_DEFAULT, wino=9, wino_gn=9, wino_sc=3, fold=0, gemm=53))
    assert "res_sc" in prog.plan.bufs


@pytest.mark.parametrize("geo", ["a", "c"])
def test_switch_up9_off(hiplib, monkeypatch, geo):
    """UP9=False: no tap-plane GEMM + gather.  At these sizes (640 / 512 source rows) the library refuses the phase form
    (rcdm_conv3x3_up2_supported: it does not fill the chip), so the upsampler takes nine taps over the upsampled grid."""
    tags, _ = run_case(monkeypatch, geo, "UP9=0", UP9=False)
    w = dict(wino=9, wino_gn=9, wino_sc=3, fold=2) if geo == "c" else {}
    expect(tags, **dict(A_DEFAULT, up9=0, up_phase=0, up_taps=1, gemm=50, **w))
    assert sum(re.match(r"conv3x3 \d+x\d+x\d+ 640->640 s=1 up=1 epi=1$", t) is not None for t in tags) == 1


@pytest.mark.parametrize("geo", ["a", "c"])
def test_switch_up9_up2_off(hiplib, monkeypatch, geo):
    """UP9=False, UP2=False: nine taps over the upsampled grid, by the switch."""
    tags, _ = run_case(monkeypatch, geo, "UP9=0 UP2=0", UP9=False, UP2=False)
    w = dict(wino=9, wino_gn=9, wino_sc=3, fold=2) if geo == "c" else {}
    expect(tags, **dict(A_DEFAULT, up9=0, up_phase=0, up_taps=1, gemm=50, **w))


def test_switch_out_taps_off(hiplib, monkeypatch):
    """OUT_TAPS=False: conv_out as the nine-tap implicit GEMM (320 -> 4 channels padded to 8)."""
    tags, _ = run_case(monkeypatch, "a", "OUT_TAPS=0", OUT_TAPS=False)
    expect(tags, **dict(A_DEFAULT, out_taps=0, out_conv=1, gemm=50))
    assert tags[-1] == "conv3x3 10x16x16 320->8 s=1 up=0 epi=1"


@pytest.mark.parametrize("geo", ["a", "c"])
def test_switch_wino_off(hiplib, monkeypatch, geo):
    """Winograd off: every 3x3 conv on nine taps; on C the three 640-wide shortcuts fall back to the fold."""
    tags, _ = run_case(monkeypatch, geo, "WINO=0", WINO_MAX_SIDE=0, WINO=())
    expect(tags, **dict(A_DEFAULT, wino=0, wino_gn=0, wino_sc=0, fold=5))
    assert fold_widths(tags) == [320, 1280, 960, 960, 640]


def test_switch_everything_off(hiplib, monkeypatch):
    """All of the above together: the plainest plan the planner can emit."""
    tags, prog = run_case(monkeypatch, "a", "all off", ROW_CHAIN=False, FF_FUSE=False, LNX=False, FFZ=False, GN_PRESTAT=False,
                          SC_FOLD=False, UP9=False, UP2=False, OUT_TAPS=False, WINO_MAX_SIDE=0, WINO=())
    expect(tags, **dict(SITES, rowchain=0, ff_fused=0, lnx=0, stat=0, ffz=0, gnstat=0, prestat=0, gn_stats=0, wino=0, fold=0, up9=0,
                        up_phase=0, up_taps=1, out_taps=0, out_conv=1, layernorm=39, ln_pe=12, gemm=109, geglu=13))
    assert "res_sc" in prog.plan.bufs


def test_wino_groupnorm_eps_on_low_variance_rows(hiplib):
    """The eps of the GroupNorm whose apply rides in the Winograd input transform.  On the UNet fixtures the norms see
    unit-variance rows, where an eps of 1e-3 instead of 1e-5 moves the output by less than the f16 path's own error (tried: the
    whole-output checks above do not see it).  A GroupNorm is scale-invariant but for its eps, so one ResnetBlock3D of a
    Winograd shape (640 -> 640, an 8x8 image) is run on rows of variance 9e-4 against the reference class's output: there a wrong
    eps is a 30 % error of the normalised rows.  Measured on MI355X: rel-RMS 7.6e-4, max 7.9e-4 of max|ref|; bound <= 2x that (the
    rel-RMS one is the single-block bound of test_hip_unet.py)."""
    from rcdms_amd.plan import Geo
    from tests.test_hip_unet import build
    assert emit_blocks.wino_level(Geo(1, 1, 8, 8), 640, 640) == (True, True)
    g = gold("unet_probe_resnet_lowvar")
    m = build("resnet_640_lowvar")
    with torch.no_grad():
        y = m(g["x"].to(DEV), g["temb"].to(DEV))
    check(y, g["y"], 1.5e-3, 1.6e-3, "ResnetBlock3D 640 -> 640 at 8x8 (Winograd), input variance 9e-4")


# ---- motion modules where the reference puts them ------------------------------------------------------------------------------

def test_motion_modules_follow_the_state_dict(hiplib, monkeypatch):
    """motion_module_resolutions=(1, 2) on the two-level config: the reference (and the mirrored class) give up block i motion
    modules when 2 ** (3 - i) is listed (unet.py:199) — here none — while the down blocks keep theirs.  The plan follows the
    state dict: 4 temporal attentions (2 down-block modules), against the reference's output for that config."""
    tags, _ = run_case(monkeypatch, "b", "mm12", kind="unet_probe_mm12", golden="unet_probe_mm12")
    expect(tags, flash=7, xattn=7, temporal=4, rowchain=12, chain_pe=2, ffz=5, lnx=15, layernorm=0, wino=6, fold=5)


def test_motion_module_layout_mismatch_is_refused(hiplib):
    """A state dict whose motion modules are not where motion_module_resolutions puts them is refused by name (RcdmError), not
    with a KeyError from the packer."""
    from rcdms_amd import engine
    from rcdms_amd.hip import RcdmError
    meta = mirrored("unet_probe")
    sd = {k: torch.zeros(s) for k, s in shapes_of(mirrored("unet_probe_mm12")).items()}
    with pytest.raises(RcdmError, match=r"up_blocks\.0\.motion_modules\.0.*lacks a motion module"):
        engine.UNetProgram(meta.engine_config(), sd, 1, 3, 16, 24, L, DEV)
