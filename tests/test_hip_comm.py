"""The thin RCCL layer of the C-ABI (rcdm_comm_*, rcdm_bcast, rcdm_allgather) and the CFG-split latency mode of the
denoising loop (two GPUs per story, one classifier-free-guidance half each; reference arithmetic
RCDMs_pipeline.py:482-497).  A GPU box here has ONE device, so the collectives run on a one-rank communicator (a one-rank
all-gather is a device copy through RCCL) and the two halves of the split loop run on the same device in lockstep; the
two-process wiring (pairing, id exchange) is covered on CPU in test_dist_gloo.py."""
import pytest
import torch

from rcdms_amd import synth
from tests.test_hip_unet import DEV, build, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comm1(hiplib):
    from rcdms_amd import hip
    c = hip.Comm(hip.Comm.unique_id(), 1, 0)
    yield c
    c.close()


def test_one_rank_bcast_and_allgather(comm1):
    x = torch.arange(4096, dtype=torch.float32, device=DEV)
    y = torch.zeros(2, 4096, dtype=torch.float32, device=DEV)
    comm1.bcast(x.data_ptr(), x.numel() * 4, root=0)
    comm1.allgather(x.data_ptr(), y.data_ptr() + 4096 * 4, 4096 * 4)       # "my slot" may be anywhere in recv
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.arange(4096, dtype=torch.float32))
    assert torch.equal(y[1], x) and not y[0].any()


def test_allgather_inside_a_captured_graph(comm1):
    from rcdms_amd import hip
    x = torch.ones(1 << 16, dtype=torch.float16, device=DEV)
    y = torch.zeros_like(x)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        comm1.allgather(x.data_ptr(), y.data_ptr(), x.numel() * 2)        # once outside capture (lazy init)
        st.synchronize()
        y.zero_()
        g = hip.Graph()
        g.begin()
        try:
            comm1.allgather(x.data_ptr(), y.data_ptr(), x.numel() * 2)
        finally:
            g.end()
        st.synchronize()
        assert not y.any()                                                  # capture did not execute
        for k in (2.0, 3.0):
            x.fill_(k)
            g.launch()
            st.synchronize()
            assert torch.equal(y, x)


def test_bad_arguments(hiplib):
    from rcdms_amd import hip
    with pytest.raises(ValueError):
        hip.Comm(b"short", 1, 0)
    with pytest.raises(hip.RcdmError, match="RCDM_EINVAL"):
        hip.Comm(bytes(128), 1, 1)                                          # rank outside [0, nranks)


def test_cfg_split_loop_equals_unsplit_loop(comm1):
    """Half 0 and half 1 of the split loop, each with batch S, in lockstep on one device — every exchange a one-rank
    RCCL all-gather into the right slot of BOTH ranks' gathered buffers — against the ordinary loop with batch 2S.
    Not bitwise (tile shapes follow M), so within the tolerance of 'a story of a batch vs the story alone'."""
    from rcdms_amd.dist import CfgSplit
    from rcdms_amd.sampler import DenoiseLoop
    from rcdms_amd.scheduler import DDIMScheduler
    m, m_other = build("unet_tiny"), build("unet_tiny")   # two "ranks": programs (buffers, context) are cached per module
    S, steps = 2, 3
    s = synth.synthetic_story(stories=S, latent_hw=(16, 16), ctx_len=13, ctx_dim=64, cfg=True, seed=21)
    s["masked_latents"][S:] += 0.05                                        # make the halves' inputs really differ
    mk = lambda: DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    ref_loop = DenoiseLoop(m, S, 5, 16, 16, 13, 2.0, mk(), steps)
    ref_loop.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
    ref = ref_loop.run().clone()

    sent = []
    halves = [DenoiseLoop(mod, S, 5, 16, 16, 13, 2.0, mk(), steps,
                          cfg_split=CfgSplit(h, lambda a, b, n, h=h: sent.append((h, a, b, n))))
              for h, mod in ((0, m), (1, m_other))]
    for lp in halves:
        lp.load(s["latents"], s["mask"], s["masked_latents"], s["ctx"])
        assert lp.prog.b == S and lp.shared is False
    st = halves[0].prog.stream
    with torch.cuda.stream(st):
        for _ in range(steps):
            for lp in halves:
                for op in lp._pre:
                    op()
                lp.prog.run_body(skip_time=True)
            for lp in halves:                                               # what rcdm_allgather does across the pair
                lp._post[0]()
            assert [h for h, *_ in sent] == [0, 1]
            (_, a0, _, n0), (_, a1, _, n1) = sent
            assert n0 == n1 == halves[0].prog.eps_out.M * halves[0].prog.eps_out.ld * 2
            for lp in halves:
                comm1.allgather(a0, lp.eps_full.data_ptr(), n0)
                comm1.allgather(a1, lp.eps_full.data_ptr() + n0, n0)
            sent.clear()
            for lp in halves:
                for op in lp._post[1:]:
                    op()
        st.synchronize()
    assert torch.equal(halves[0].lat, halves[1].lat)                        # both ranks hold the same story state
    check(halves[0].lat, ref.cpu(), 3.5e-3, 5e-3, "CFG-split loop vs batch-2S loop")


def test_cfg_split_needs_guidance(hiplib):
    from rcdms_amd.dist import CfgSplit
    from rcdms_amd.sampler import DenoiseLoop
    from rcdms_amd.scheduler import DDIMScheduler
    m = build("unet_tiny")
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False)
    with pytest.raises(ValueError, match="guidance"):
        DenoiseLoop(m, 1, 5, 16, 16, 13, 1.0, sched, 2, cfg_split=CfgSplit(0, lambda *a: None))


def test_bench_two_ranks_share_one_gpu(hiplib):
    """The N > 1 code path of bench.py end to end on a one-GPU box (`--share-gpu`: both ranks on device 0, gloo instead of
    RCCL): per-rank build barrier, the full-width UNet built on every rank, broadcast_module of rank 0's 1286 tensors (GPU
    tensors, f16 wire), one story per rank with its own seed, the barrier / max-over-ranks timing and the gathered device
    list.  The line is marked INVALID — it only proves that the path the driver's 8-GPU run takes executes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-gpu", "--steps", "1", "--warmup", "0",
                        "--ddim-steps", "2", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and len(out["per_rank_ms"]) == 2 and len(out["devices"]) == 2
    assert out["data"].startswith("INVALID (--share-gpu") and out["gathered_stories"] == 2
    assert out["config"]["parallelism"] == "story-replicas x2" and out["scaling"] == "weak"
    # value = the frames of BOTH ranks over the slower rank's time
    assert abs(out["value"] - 5 * 1 * 1 * 2 / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]


def test_bench_eight_ranks_share_one_gpu(hiplib):
    """Rehearsal of the driver's `--gpus 8` run on the one device a builder's box has (VERDICT r5 #5a): EIGHT ranks of
    bench.py's real multi-rank path on device 0 (gloo in place of RCCL, a width-64 UNet so that eight launch plans fit) —
    build by the node's first rank + stamp check on the seven others, broadcast_module of rank 0's weights, the shared
    unconditional context rows broadcast from rank 0 (rcdms_amd.dist.broadcast_context, what north_star words as the RCCL
    context broadcast), one story per rank, barrier / max-over-ranks timing, and the final gather with an UNEVEN story count
    (--ragged: the odd ranks contribute none, so gather_stories' size exchange + padding runs on device tensors)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--share-gpu", "--width", "64", "--latent", "16",
                        "--ctx-len", "13", "--steps", "2", "--warmup", "1", "--ddim-steps", "3", "--ragged", "--no-cpu-baseline",
                        "--watchdog", "600"], capture_output=True, text=True, timeout=1200, env=env, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 8 and len(out["per_rank_ms"]) == 8 and len(out["devices"]) == 8
    assert out["gathered_stories"] == 4, "ranks 0, 2, 4, 6 hand one story each to the gather"
    assert out["data"].startswith("INVALID (")
    assert out["config"]["parallelism"] == "story-replicas x8" and out["scaling"] == "weak"
    assert abs(out["value"] - 5 * 1 * 2 * 8 / (2 * out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]


def test_bench_plain_run_dumps_outputs(hiplib, tmp_path):
    """A plain one-GPU bench.py run (no --full) times the headline only and, with --dump-outputs, writes the finished latents of
    its last timed pass; inputs and weights are seeded, so runs with different --steps / --warmup dump the same latents."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for steps, warmup in ((1, 0), (2, 1)):
        d = str(tmp_path / f"s{steps}")
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--width", "64", "--latent", "16",
                            "--ctx-len", "13", "--ddim-steps", "3", "--steps", str(steps), "--warmup", str(warmup),
                            "--dump-outputs", d], capture_output=True, text=True, timeout=900, env=env, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
        assert "cpu_baseline" not in out and "extra_configs" not in out
        assert sorted(os.listdir(d)) == ["latents.npy"]
        lat = np.load(os.path.join(d, "latents.npy"))
        assert lat.dtype == np.float32 and lat.shape == (1, 4, 5, 16, 16) and np.isfinite(lat).all()
        dumps.append(lat)
    np.testing.assert_allclose(dumps[0], dumps[1], rtol=1e-3, atol=1e-4)
