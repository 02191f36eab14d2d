"""GPU: the rank-1-context plan, the numerics / headroom report and the third ("sdlike") weight family.

Rank-1 context: for an unseen frame the reference's semantic_stack has ONE key / value token
(stage2_batchtest_rcdms_model.py:117-132), so all L context rows of that image are one vector
(RCDMs_pipeline.py:447-450) and attn2 (attention.py:139-144,170-199) is independent of the query — with mask
[1,0,0,0,0] that is 8 of the 10 images of every UNet call.  The plan variant evaluates norm2 / to_q / the attention /
to_out on the full-rank images only; everything here is checked against REFERENCE-minted goldens
(oracle/make_golden.py --only rank1ctx) and against the general plan on the same inputs."""
import os

import pytest
import torch

from oracle import unet_oracle as O
from rcdms_amd import engine, hip, synth
from tests.test_hip_unet import DEV, build, check, rel_rms
from tests.test_oracle_golden import gold

pytestmark = pytest.mark.gpu


def _x_of(s):
    return torch.cat([torch.cat([s["latents"]] * 2), s["mask"], s["masked_latents"]], dim=1)


@pytest.fixture(scope="module")
def tiny(hiplib):
    return build("unet_tiny")


def test_full_rank_runs_detection(hiplib):
    ctx = torch.randn(10, 13, 64, device=DEV)
    assert engine.full_rank_runs(ctx) == ((0, 10),)
    ctx[2:] = ctx[2:, :1].expand(-1, 13, -1).clone()
    assert engine.full_rank_runs(ctx) == ((0, 2),)
    ctx[5] = torch.randn(13, 64, device=DEV)
    assert engine.full_rank_runs(ctx) == ((0, 2), (5, 6))
    ctx[:] = ctx[:, :1].expand(-1, 13, -1).clone()
    assert engine.full_rank_runs(ctx) == ()
    ctx[3, 7, 9] = float("nan")                  # NaN compares unequal: that image counts as full rank (general path)
    assert engine.full_rank_runs(ctx) == ((3, 4),)


def test_tiny_unet_rank1ctx_vs_reference(tiny):
    """Width-64 topology, 16x16 latents (every level below the chain kernels' row count: the deferred-LayerNorm form with the
    per-image row in attn1.to_out's epilogue) against the reference's output on the structured context."""
    g = gold("unet_tiny_16_rank1ctx")
    with torch.no_grad():
        y = tiny(g["x"].to(DEV), torch.tensor(int(g["t"])), g["ctx"].to(DEV), return_dict=False)[0]
        y2 = tiny(g["x"].to(DEV), torch.tensor(int(g["t"])), g["ctx"].to(DEV))     # hipGraph replay
    prog = tiny.program(2, 5, 16, 16, 13, rank1_runs=((0, 2),))
    assert prog.rank1_runs == ((0, 2),) and prog.calls >= 2, "forward() did not select the rank-1-context plan"
    assert any(t.startswith("rank1_") for t in prog._ctx_plan.tags)
    n_x = sum(t.startswith("xattn ") for t in prog.plan.tags)
    assert n_x == prog.n_sites and all(" B=2 " in t for t in prog.plan.tags if t.startswith("xattn "))
    check(y, g["y"], 4e-3, 8e-3, "unet_tiny_16_rank1ctx")
    assert torch.equal(y, y2), "graph replay differs from the eager launch sequence"


def test_rank1_plan_matches_general_plan(tiny, monkeypatch):
    """The same structured context through the GENERAL plan (fast path switched off) and through the rank-1 plan: two f16
    evaluations of the same function (the general plan's softmax over equal scores is uniform), so they agree far inside the
    whole-UNet tolerance; and the fast path really launches less."""
    g = gold("unet_tiny_16_rank1ctx")
    x, t, ctx = g["x"].to(DEV), torch.tensor(int(g["t"])), g["ctx"].to(DEV)
    with torch.no_grad():
        y_fast = tiny(x, t, ctx, return_dict=False)[0].clone()
        monkeypatch.setattr(engine.SW, "RANK1_CTX", False)
        y_gen = tiny(x, t, ctx.clone(), return_dict=False)[0].clone()    # (a new tensor object: no cached plan choice)
    p_gen, p_fast = tiny.program(2, 5, 16, 16, 13), None
    monkeypatch.setattr(engine.SW, "RANK1_CTX", True)
    p_fast = tiny.program(2, 5, 16, 16, 13, rank1_runs=((0, 2),))
    assert p_gen.rank1_runs is None and p_fast.rank1_runs == ((0, 2),)
    r = rel_rms(y_fast.cpu(), y_gen.cpu())
    print(f"rank-1 plan vs general plan: rel-RMS {r:.2e}")
    assert r < 4e-3      # (the tolerance of "same story, different plan": two f16 evaluations differ by ~2e-3, test_hip_unet.py)
    gemm_rows = lambda p: sum(int(tg.split("M=")[1].split()[0]) for tg in p.plan.tags if tg.startswith("gemm ") and " N=" in tg)
    assert gemm_rows(p_fast) < gemm_rows(p_gen)


@pytest.mark.parametrize("runs", [((0, 1), (5, 6)), (), ((3, 10),)])
def test_rank1_arbitrary_runs_vs_oracle(tiny, runs):
    """Full-rank images anywhere (fix_context_order=True interleaves them: [u0 | u1..u4 | c0 | c1..c4]), none at all, and a
    suffix: several runs, row offsets into the statistics buffer, the all-rank-1 plan — against the CPU oracle."""
    s = synth.synthetic_story(stories=1, latent_hw=(16, 16), ctx_len=13, ctx_dim=64, seed=51)
    ctx = s["ctx"]
    full = [any(i0 <= i < i1 for i0, i1 in runs) for i in range(10)]
    for i in range(10):
        if not full[i]:
            ctx[i] = ctx[i, :1].expand(13, -1).clone()
    x = _x_of(s)
    sd = synth.procedural_state_dict({k: v.shape for k, v in tiny.state_dict().items()}, 7)
    cfg = O.tiny_config(width=64, cross_dim=64, layers_per_block=2)
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, torch.tensor(321), ctx)
        y = tiny(x.to(DEV), torch.tensor(321), ctx.to(DEV), return_dict=False)[0]
    prog = tiny.program(2, 5, 16, 16, 13, rank1_runs=runs)
    assert prog.rank1_runs == runs and prog.calls >= 1
    check(y, ref, 4e-3, 8e-3, f"rank-1 runs {runs}")


def test_rank1_plan_refuses_a_dense_context(tiny):
    prog = tiny.program(2, 5, 16, 16, 13, rank1_runs=((0, 2),))
    with pytest.raises(hip.RcdmError, match="identical rows"):
        prog.set_context(torch.randn(10, 13, 64, device=DEV), force=True)


@pytest.fixture(scope="module")
def full_unet(hiplib):
    return build("unet_full")


@pytest.mark.parametrize("hw", [32, 64])
def test_full_unet_rank1ctx_vs_reference(full_unet, hw):
    """The 1276.9 M-parameter UNet on synthetic_story(structure="reference") — rows [u0, c0 | 8 rank-1 images] — against the
    reference UNet's fp32 output (oracle/make_golden.py --only rank1ctx).  32x32: every level on the deferred form; 64x64: the
    chain kernels' level keeps attn2.to_q inside its chain and reads the rank-1 images' V rows from the site's own buffer."""
    path = os.path.join(os.path.dirname(__file__), "golden", f"unet_full_{hw}_rank1ctx.npz")
    assert os.path.exists(path)
    g = gold(f"unet_full_{hw}_rank1ctx")
    s = synth.synthetic_story(stories=1, latent_hw=(hw, hw), ctx_len=85, seed=42, structure="reference")
    x = _x_of(s).to(DEV)
    with torch.no_grad():
        y = full_unet(x, torch.tensor(int(g["t"])), s["ctx"].to(DEV), return_dict=False)[0]
    prog = full_unet.program(2, 5, hw, hw, 85, rank1_runs=((0, 2),))
    assert prog.rank1_runs == ((0, 2),) and prog.calls >= 1
    check(y, g["y"], 4e-3, 6e-3, f"unet_full_{hw}_rank1ctx")


def test_denoise_loop_selects_rank1_plan(tiny):
    """DenoiseLoop.load() picks the plan per context the way it picks the shared CFG prefix per story; 4 CFG + DDIM steps on
    the structured story against the oracle loop, and the dense story still takes the general plan."""
    from rcdms_amd.sampler import DenoiseLoop
    from rcdms_amd.scheduler import DDIMScheduler
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    loop = DenoiseLoop(tiny, 1, 5, 16, 16, 13, 2.0, sched, 4)
    s = synth.synthetic_story(stories=1, latent_hw=(16, 16), ctx_len=13, ctx_dim=64, seed=61, structure="reference")
    loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
    assert loop.rank1_runs == ((0, 2),) and loop.shared
    out = loop.run().cpu()
    sd = synth.procedural_state_dict({k: v.shape for k, v in tiny.state_dict().items()}, 7)
    cfg = O.tiny_config(width=64, cross_dim=64, layers_per_block=2)
    with torch.no_grad():
        ref = O.denoise_loop(sd, cfg, s["latents"], s["mask"], s["masked_latents"], s["ctx"], 4, 2.0)
    check(out, ref, 4e-3, 8e-3, "4-step loop, rank-1 context plan")
    d = synth.synthetic_story(stories=1, latent_hw=(16, 16), ctx_len=13, ctx_dim=64, seed=61)
    loop.load(d["latents"], d["mask"], d["masked_latents"], d["ctx"])
    assert loop.rank1_runs is None


def test_gemm_lnx_requested_stat_parts(hiplib):
    """rcdm_gemm_lnx with a stat_parts other than the shape's own tile choice (rcdm_gemm_lnx_parts_ok): a row subset of a
    projection rewrites its rows' statistics inside the buffer the full-row launch filled — same slot count, same plane
    stride, the other rows untouched; the slots (tile sum, centred sum of squares) against float64."""
    from rcdms_amd.engine import Plan, emit_gemm, Rows
    torch.manual_seed(0)
    M, C, r0, n = 10240, 640, 2048, 2048
    plan = Plan(DEV)
    A = plan.rows("A", M, C, unique=True)
    out = plan.rows("out", M, C, unique=True)
    W = (torch.randn(C, C, device=DEV) * C ** -0.5).half()
    bias = torch.randn(C, device=DEV) * 0.1
    st = emit_gemm(plan, A, W, C, C, out, bias=bias, stat=True)
    assert st is not None
    sub_parts = hip.gemm_stat_parts(hip.GemmDesc(n, C, C, C, C, 0, hip.EPI_BIAS, 1, 0, 1.0, 0, 0))
    st2 = emit_gemm(plan, A.rows(r0, n), W, C, C, out.rows(r0, n), bias=bias * 2, stat_into=st, stat_row0=r0)
    assert st2 is st, "no tile with the buffer's slot count for the subset shape"
    print(f"full launch: {st.parts} slots; the subset's own choice would be {sub_parts}")
    plan.materialize()
    a = torch.randn(M, C, device=DEV).half()
    A.buf.t.view(torch.float16)[:M * C].copy_(a.reshape(-1))
    plan.run()
    torch.cuda.synchronize()
    o = out.buf.t.view(torch.float16)[:M * C].view(M, C).double()
    slots = st.buf.t.view(torch.float32)[:st.parts * st.rows * 2].view(st.parts, st.rows, 2).double()
    stat = slots.sum(dim=0)
    ref = a.float() @ W.float().t()
    exp = (ref + bias).half()
    exp[r0:r0 + n] = (ref[r0:r0 + n] + 2 * bias).half()
    assert (o - exp.double()).abs().max() <= 2e-2
    assert torch.allclose(stat[:, 0], o.sum(dim=1), rtol=2e-6, atol=1e-3)
    # a slot's second half is the centred sum of squares of its column tile (the slot rule: igemm_args.h), summed about the
    # tile's first value: 2e-6 of that sum's size, as the sums above
    bn = C if st.parts == 1 else next(w for w in (64, 128, 256) if (C + w - 1) // w == st.parts)
    for t in range(st.parts):
        v = o[:, t * bn:min(C, (t + 1) * bn)]
        mean = v.mean(dim=1)
        m2 = ((v - mean[:, None]) ** 2).sum(dim=1)
        size = m2 + 2 * v.shape[1] * (v[:, 0] - mean) ** 2
        assert ((slots[t, :, 1] - m2).abs() <= 2e-6 * size + 1e-3).all()


# ---- numerics report + the third weight family --------------------------------------------------------------------------

def test_numerics_report_tiny(tiny):
    g = gold("unet_tiny_16")
    rep = tiny.numerics_report(g["x"].to(DEV), torch.tensor(int(g["t"])), g["ctx"].to(DEV), verbose=True)
    assert rep["n_ops"] > 100 and rep["buffers"] and rep["attention"] and rep["layernorm"]
    assert 1.0 < rep["min_headroom"] < float("inf")
    assert all(r["weight_bound"] >= r["input_bound"] * 0.999 for r in rep["attention"]), "the weight-norm bound must dominate"
    assert not any(r["wide_range"] for r in rep["attention"])


def test_numerics_report_raises_on_overflow(tiny):
    g = gold("unet_tiny_16")
    x = g["x"].to(DEV).clone()
    x[:, :4] *= 3e5           # latents far outside anything the loop produces: conv_in's output leaves the f16 range
    with pytest.raises(hip.RcdmError, match="non-finite"):
        tiny.numerics_report(x, torch.tensor(int(g["t"])), g["ctx"].to(DEV), verbose=False)


def test_full_unet_sdlike_weights_vs_reference(hiplib):
    """The THIRD weight family at full width, 32x32 latents: synth style "sdlike" — two output channels of
    every ResnetBlock3D conv1 / conv2 at 50-100x gain feeding the GroupNorms (activations of ~270 on the residual stream), the
    spatial self-attentions' to_q / to_k at 3x gain each (scaled-score bound of this input ~240: logits in the hundreds, 11 of
    the 16 sites leave the matrix-pipe softmax argument by the weight-norm bound) — against the reference UNet's fp32 output with
    the same weights (oracle/make_golden.py --only sdlike), at the PRODUCT tolerance INTEGRATION.md states for real checkpoints
    (rel-RMS <= 7e-3, max <= 1e-2 of max|ref|; measured 2.5e-3 / 3.2e-3), with the report a user would read first.
    Measured beside it and NOT asserted: the outlier channels alone cost nothing (1.3e-3); a q / k gain of 5 (score
    bound ~650) gives 1.6e-2 with the outliers and 2.5e-1 without — a random network with one-hot attention is discontinuous
    (an argmax flip moves an output by O(1)), which no arithmetic of finite precision follows; the d = 40 / 80 / 160 kernels
    themselves hold the ordinary tolerance at such scores (test_flash_attn_large_logits_all_head_dims)."""
    g = gold("unet_full_32_sdlike")
    m = build("unet_full", seed=int(g["seed"]), style="sdlike")
    s = synth.synthetic_story(stories=1, latent_hw=(32, 32), ctx_len=85, seed=int(g["story_seed"]))
    x = _x_of(s).to(DEV)
    t = torch.tensor(int(g["t"]))
    rep = m.numerics_report(x, t, s["ctx"].to(DEV), verbose=True)
    print(f"reference's largest residual-stream activation {float(g['max_final']):.1f}; HIP path min headroom x{rep['min_headroom']:.1f}")
    assert rep["min_headroom"] > 4.0
    assert max(r["max_abs"] for r in rep["buffers"]) >= 100.0, "the family is supposed to produce outlier activations"
    assert max(r["input_bound"] for r in rep["attention"]) >= 100.0, "... and attention logits in the hundreds"
    assert rep["wide_sites"] >= 1, "... and to push some sites past the matrix-pipe softmax argument's documented range"
    with torch.no_grad():
        y = m(x, t, s["ctx"].to(DEV), return_dict=False)[0]
    check(y, g["y"], 7e-3, 1e-2, "unet_full_32_sdlike")


@pytest.mark.parametrize("d,L", [(40, 1024), (80, 256), (160, 64)])
def test_flash_attn_large_logits_all_head_dims(hiplib, d, L):
    """Self-attention with |scale log2(e) q.k| in the several hundreds (a nearly one-hot softmax) on every head width of the
    UNet, with and without RCDM_ATTN_WIDE_RANGE: the ordinary kernel tolerance against the fp32 oracle on the same f16 inputs
    (the wide-range flag only changes the d = 40 kernel; the others always take their softmax argument in fp32)."""
    from tests.test_hip_kernels import close, h16
    heads, gain = 8, 12.0
    C = heads * d
    gq = torch.Generator().manual_seed(5 + d)
    q = h16(torch.randn(2, L, C, generator=gq) * gain ** 0.5)
    k = h16(torch.randn(2, L, C, generator=gq) * gain ** 0.5)
    v = h16(torch.randn(2, L, C, generator=gq))
    ref = O.attention_core(q, k, v, heads)
    qd, kd, vd = (t.reshape(-1, C).half().to(DEV) for t in (q, k, v))
    smax = (torch.einsum("blhd,bmhd->bhlm", q.view(2, L, heads, d), k.view(2, L, heads, d)).abs().max() * d ** -0.5 * 1.4427).item()
    for flags in (hip.ATTN_WIDE_RANGE, 0):
        out = torch.full((2 * L, C), float("nan"), dtype=torch.float16, device=DEV)
        desc = hip.AttnDesc(2, heads, L, L, d, C, C, C, C, d ** -0.5, flags)
        hip.flash_attn(desc, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        got = out.float().cpu().reshape(2, L, C)
        assert torch.isfinite(got).all()
        print(f"d = {d}, flags {flags}: max |scaled score| {smax:.0f}, max abs err {(got - ref).abs().max().item():.3e}")
        if flags or d != 40:
            close(got, ref, rel=2e-3, abs_frac=4e-3)
