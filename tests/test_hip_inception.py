"""GPU: rcdms_amd/inception.py against the CPU restatement tests/inception_oracle.py, full width, synthetic weights.

The rule for every comparison: let e_model be the relative RMS error of the oracle's f16 MODEL (folded weights rounded to f16,
every layer output rounded to f16: the arithmetic the kernels are allowed) against the oracle's fp32 evaluation on the same
input, computed here from the oracle alone.  The kernels must be within 2 e_model of the fp32 oracle; the factor 2 covers a
different summation order inside a k-step and in the pools.  Blocks are compared at that rule on a block's output, the whole
network on the 2048 features.

Measured on an MI355X, 2 frames of 48 x 64, seed 0 weights (printed by the whole-network test):
    fid          e_model 5.18e-04, kernels against the fp32 oracle 5.37e-04, against the f16 model 2.14e-04
    torchvision  e_model 5.13e-04, kernels against the fp32 oracle 5.18e-04, against the f16 model 1.95e-04
and the blocks at 1.00 x their e_model (2.1e-04 ... 4.5e-04)."""
import pytest
import torch

from tests import inception_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt())


@pytest.fixture(scope="module")
def sd():
    return O.synthetic_state_dict(0, num_classes=9)


@pytest.fixture(scope="module")
def frames():
    g = torch.Generator().manual_seed(1)
    return torch.randint(0, 256, (2, 48, 64, 3), generator=g, dtype=torch.uint8)


@pytest.fixture(scope="module")
def nets(hiplib, sd):
    from rcdms_amd.inception import InceptionV3Features
    return {v: InceptionV3Features(sd, variant=v, device=DEV) for v in ("fid", "torchvision")}


BLOCK_CASES = [("Mixed_5b", 7, 5, "fid"), ("Mixed_6a", 9, 7, "fid"), ("Mixed_6b", 5, 6, "fid"), ("Mixed_7a", 9, 7, "fid"),
               ("Mixed_7b", 3, 4, "fid"), ("Mixed_7b", 3, 4, "torchvision"), ("Mixed_7c", 3, 4, "fid"),
               ("Mixed_5b", 7, 5, "torchvision"), ("Mixed_6b", 5, 6, "torchvision")]


@pytest.mark.parametrize("block,h,w,variant", BLOCK_CASES, ids=[f"{b}-{v}" for b, _, _, v in BLOCK_CASES])
def test_block_against_oracle(hiplib, sd, block, h, w, variant):
    from rcdms_amd import inception as I
    net = I.InceptionV3Features(sd, variant=variant, device=DEV, blocks=(block,))
    g = torch.Generator().manual_seed(h * 16 + w)
    x = torch.randn(2, h, w, I.BLOCK_IN[block], generator=g).abs().half()           # post-ReLU-like rows, n = 2
    got = net.run_block(block, x.to(DEV)).float().cpu().permute(0, 3, 1, 2)
    xin = x.float().permute(0, 3, 1, 2)
    ref = O.Net(sd, variant).block(block, xin)
    model = O.Net(sd, variant, f16=True).block(block, xin)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    e_model, e_kernel = rel_rms(model, ref), rel_rms(got, ref)
    print(f"{block} {variant} at {h}x{w}: e_model {e_model:.3e}, kernels {e_kernel:.3e}")
    assert e_kernel <= 2 * e_model, (e_kernel, e_model)
    # every concat window separately, so a branch in the wrong window cannot hide in the block's RMS
    widths = {"Mixed_5b": (64, 64, 96, 32), "Mixed_6a": (384, 96, 288), "Mixed_6b": (192, 192, 192, 192),
              "Mixed_7a": (320, 192, 768), "Mixed_7b": (320, 768, 768, 192), "Mixed_7c": (320, 768, 768, 192)}[block]
    o = 0
    for c in widths:
        e_m, e_k = rel_rms(model[:, o:o + c], ref[:, o:o + c]), rel_rms(got[:, o:o + c], ref[:, o:o + c])
        # a pass-through max pool is exact in both (e_m = 0)
        assert e_k <= 2 * e_m, (block, o, c, e_k, e_m)
        o += c
    assert o == ref.shape[1]


@pytest.mark.parametrize("variant", ["fid", "torchvision"])
def test_whole_network_within_twice_the_f16_model(nets, sd, frames, variant):
    net = nets[variant]
    feats, logits = net(frames.to(DEV), return_logits=True)
    assert tuple(feats.shape) == (2, 2048) and feats.dtype == torch.float32 and feats.is_cuda
    assert tuple(logits.shape) == (2, 9)
    f = feats.cpu()
    assert torch.isfinite(f).all(), "non-finite features"
    ref = O.features(sd, frames, variant)
    model = O.features(sd, frames, variant, f16=True)
    e_model, e_kernel = rel_rms(model, ref), rel_rms(f, ref)
    print(f"whole network {variant}: e_model {e_model:.3e}, kernels against the fp32 oracle {e_kernel:.3e}, "
          f"kernels against the f16 model {rel_rms(f, model):.3e}")
    assert e_kernel <= 2 * e_model, (e_kernel, e_model)
    # logits: the oracle's fc on the kernels' own features, f16 weights as rcdm_small_linear holds them, at that kernel's
    # tolerance in tests/test_hip_kernels.py (rel 1e-3 + 1e-3 of the largest)
    want = f.double() @ sd["fc.weight"].half().double().T + sd["fc.bias"].double()
    lg = logits.cpu().double()
    assert torch.isfinite(lg).all()
    tol = 1e-3 * want.abs().max() + 1e-3 * want.abs()
    assert bool(((lg - want).abs() <= tol).all()), float((lg - want).abs().max())


def test_plumbing_stats_banks_chunks_and_plan_reuse(nets, sd, frames):
    from rcdms_amd.frechet import FeatureStats
    from rcdms_amd.inception import InceptionV3Features
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd import hip
    net = nets["fid"]
    dev = frames.to(DEV)
    built = net.plans_built
    rows = net(dev)
    again = net(dev)
    assert net.plans_built <= built + 1 and torch.equal(rows, again)
    built = net.plans_built
    net(dev)
    assert net.plans_built == built, "a second call at the same (N, H, W) built a plan"
    other = torch.randint(0, 256, (2, 31, 17, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)).to(DEV)
    assert tuple(net(other).shape) == (2, 2048) and net.plans_built == built, "another frame size at the same N built a plan"
    assert torch.equal(net(dev), rows), "the shared plan carried something over from the other frame size"
    st, bank = FeatureStats(2048, DEV), FeatureBank(2048, DEV)
    st.update(rows)
    bank.append(rows)
    assert st.n == 2 and bank.n == 2
    # N = 7 in chunks of 3 (3 + 3 + 1) against one chunk of 7
    g = torch.Generator().manual_seed(4)
    seven = torch.randint(0, 256, (7, 24, 40, 3), generator=g, dtype=torch.uint8).to(DEV)
    one = InceptionV3Features(sd, device=DEV, batch=7)(seven)
    small = InceptionV3Features(sd, device=DEV, batch=3)
    three = small(seven)
    assert small.plans_built == 2                                                  # n = 3 and n = 1
    assert torch.equal(one.view(torch.int32), three.view(torch.int32))
    # logits of 9 frames: rcdm_small_linear once with 8 rows (8 * 2048 * 4 bytes: the whole 64 KB of LDS it may use) and once
    # with 1, each row equal to the oracle's fc on that row's features at that kernel's tolerance
    nine = torch.randint(0, 256, (9, 24, 40, 3), generator=g, dtype=torch.uint8).to(DEV)
    f9, l9 = net(nine, return_logits=True)
    assert tuple(l9.shape) == (9, 9) and torch.equal(f9, net(nine))
    want = f9.cpu().double() @ sd["fc.weight"].half().double().T + sd["fc.bias"].double()
    assert torch.isfinite(l9).all()
    assert bool(((l9.cpu().double() - want).abs() <= 1e-3 * want.abs().max() + 1e-3 * want.abs()).all())
    # leading axes flatten; a strip's cell is read by its pitch
    strip = torch.randint(0, 256, (2, 24, 120, 3), generator=g, dtype=torch.uint8).to(DEV)
    cell = strip[:, :, 40:80]
    assert torch.equal(net(cell), net(cell.contiguous()))
    assert tuple(net(seven[:6].view(2, 3, 24, 40, 3)).shape) == (6, 2048)
    with pytest.raises(hip.RcdmError, match="no CPU path"):
        net(frames)
    with pytest.raises(ValueError, match="uint8"):
        net(dev.float())


class _CountingLib:
    """librcdm_hip.so with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


from tests.test_story_gpu import DEV as _DEV, S, chain  # noqa: E402,F401  (chain: the module-scoped fixture)
from tests.test_story_metrics_gpu import call  # noqa: E402

NEW_ENTRIES = ("rcdm_conv2d", "rcdm_pool2d", "rcdm_global_avgpool", "rcdm_image_bilinear_rows")


def counted(fn):
    """fn() with every call into the library counted by symbol -> (result, {symbol: calls})."""
    from rcdms_amd import hip
    lib = hip.load()
    proxy = _CountingLib(lib)
    hip._lib = proxy
    try:
        out = fn()
    finally:
        hip._lib = lib
    return out, proxy.calls


def minus(a, b):
    return {k: a.get(k, 0) - b.get(k, 0) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}


def plus(a, b):
    return {k: a.get(k, 0) + b.get(k, 0) for k in set(a) | set(b)}


class _Forwards:
    """The vision tower with its forwards counted by batch size."""

    def __init__(self, inner):
        self.inner, self.batches = inner, []

    def __call__(self, *args, **kw):
        out = self.inner(*args, **kw)
        self.batches.append(out.image_embeds.shape[0])
        return out

    def __getattr__(self, name):
        return getattr(self.inner, name)


def test_story_runner_inception_feature_source(chain, nets):
    from rcdms_amd.frechet import FeatureStats
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.story import StoryRunner
    b, net = chain, nets["fid"]
    old = b.runner
    assert old.inception is None
    # the extractor goes in through the constructor; everything else is the chain's own runner
    b.runner = StoryRunner(old.prior_pipe, old.stage2_pipe, old.image_encoder, clip_processor=old.clip_processor,
                           frame_transform=old.frame_transform, inception=net)
    try:
        assert b.runner.inception is net
        gen, ref = FeatureStats(2048, DEV), FeatureStats(2048, DEV)
        bgen, bref = FeatureBank(2048, DEV), FeatureBank(2048, DEV)
        rec = _Forwards(b.runner.image_encoder)
        b.runner.image_encoder = rec
        res = call(b, (), feature_source="inception", feature_stats=(gen, ref), feature_banks=(bgen, bref))
        assert 5 * S not in rec.batches[1:], "a CLIP forward over the generated frames ran without clip_i being asked for"
    finally:
        b.runner = old
    assert gen.n == 5 * S and ref.n == 5 * S and bgen.n == 5 * S and bref.n == 5 * S
    assert res.clip_i is None
    # the rows are the extractor's on the same frames
    want_gen = net(res.videos.reshape(5 * S, *res.videos.shape[2:]))
    want_ref = net(b.frames.to(DEV).reshape(5 * S, *b.frames.shape[2:]))
    assert torch.equal(bgen.rows(), want_gen) and torch.equal(bref.rows(), want_ref)
    g2, r2 = FeatureStats(2048, DEV), FeatureStats(2048, DEV)
    g2.update(want_gen)
    r2.update(want_ref)
    assert torch.equal(gen.mean(), g2.mean()) and torch.equal(ref.mean(), r2.mean())


def test_clip_feature_source_launches_what_the_parts_launch(chain):
    """feature_source="clip" must launch what the call launched before the argument existed.  The reference is built outside
    story_metrics: the library calls, symbol by symbol, of a call with clip_i alone, plus those of FeatureStats.update /
    FeatureBank.append made directly on rows of the shape the runner hands over.  The call with feature_stats (and
    feature_banks) on top of clip_i must make exactly that many of every symbol — clip_i already pays for the one vision
    forward, so a second forward, a second update or any new entry point shows as a surplus — and the vision tower must
    have run on 5 S rows exactly twice (targets, generated frames)."""
    from rcdms_amd.frechet import FeatureStats
    from rcdms_amd.kid import FeatureBank
    b = chain
    call(b, ("clip_i",))                                                   # steady state: plans, the black / white embeddings
    base, c_base = counted(lambda: call(b, ("clip_i",)))
    rows = base.target_embeds.reshape(5 * S, -1)
    _, c_update = counted(lambda: (FeatureStats(b.E, DEV).update(rows), FeatureStats(b.E, DEV).update(rows)))
    _, c_append = counted(lambda: (FeatureBank(b.E, DEV).append(rows), FeatureBank(b.E, DEV).append(rows)))
    assert sum(c_update.values()) >= 2, c_update
    for kw in ({}, {"feature_source": "clip"}):
        s1, s2 = FeatureStats(b.E, DEV), FeatureStats(b.E, DEV)
        rec = _Forwards(b.runner.image_encoder)
        b.runner.image_encoder = rec
        try:
            out, c = counted(lambda: call(b, ("clip_i",), feature_stats=(s1, s2), **kw))
        finally:
            b.runner.image_encoder = rec.inner
        surplus = minus(c, plus(c_base, c_update))
        print(f"feature_stats {kw}: {sum(c.values())} library calls = {sum(c_base.values())} (clip_i alone) + "
              f"{sum(c_update.values())} (two updates); surplus {surplus}")
        assert not surplus, surplus
        assert not any(n in c for n in NEW_ENTRIES)
        assert rec.batches.count(5 * S) == 2, rec.batches
        assert s1.n == 5 * S and s2.n == 5 * S
        assert torch.equal(out.videos, base.videos) and torch.equal(out.clip_i, base.clip_i)
        k1, k2 = FeatureBank(b.E, DEV), FeatureBank(b.E, DEV)
        t1, t2 = FeatureStats(b.E, DEV), FeatureStats(b.E, DEV)
        _, c = counted(lambda: call(b, ("clip_i",), feature_stats=(t1, t2), feature_banks=(k1, k2), **kw))
        surplus = minus(c, plus(plus(c_base, c_update), c_append))
        assert not surplus, surplus
        assert k1.n == 5 * S and torch.equal(k2.rows(), rows.float())
