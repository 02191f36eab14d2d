"""GPU: StoryRunner(..., lpips=net, metrics=("lpips",)) on the tiny chain of tests/test_story_gpu.py: res.lpips is the network
applied to the generated uint8 frames and the resized targets "ssim" / "psnr" use (the same bits), "lpips" without a network is
refused before anything runs, and a call without "lpips" launches nothing from csrc/lpips.hip."""
import pytest
import torch

from tests import lpips_oracle as O
from tests.test_story_gpu import DEV, H, S, W, chain  # noqa: F401  (chain: the module-scoped fixture)
from tests.test_story_metrics_gpu import call, targets

pytestmark = pytest.mark.gpu


class _Counter:
    """Counts the calls of the two entry points of csrc/lpips.hip that go through rcdms_amd.hip."""

    def __init__(self, monkeypatch):
        from rcdms_amd import hip
        self.calls = 0
        for name in ("lpips_head", "lpips_input_rows"):
            inner = getattr(hip, name)
            monkeypatch.setattr(hip, name, self._wrap(inner))

    def _wrap(self, inner):
        def fn(*args, **kw):
            self.calls += 1
            return inner(*args, **kw)
        return fn


@pytest.mark.parametrize("net_name", ["alex", "vgg"])
def test_story_lpips_equals_the_network_on_the_frames_and_targets(chain, monkeypatch, net_name):
    from rcdms_amd.lpips import LpipsNet
    b = chain
    net = LpipsNet(O.synthetic_state_dict(net_name, 2), net_name, device=DEV, batch=4)
    monkeypatch.setattr(b.runner, "lpips", net)
    counter = _Counter(monkeypatch)
    res = call(b, ("lpips", "psnr"))
    assert counter.calls > 0
    assert tuple(res.lpips.shape) == (S, 5) and res.lpips.dtype == torch.float64 and res.lpips.is_cuda and res.ssim is None
    want = net(res.videos, targets(b))
    assert torch.equal(res.lpips.view(torch.int64), want.view(torch.int64))
    flat = net(res.videos.reshape(S * 5, H, W, 3), targets(b).reshape(S * 5, H, W, 3))          # one leading axis, other chunks
    assert torch.equal(flat.view(S, 5).view(torch.int64), want.view(torch.int64))
    assert bool(torch.isfinite(res.lpips).all()) and bool((res.lpips > 0).all())
    print(f"story lpips ({net_name}): {float(res.lpips.min()):.4f}..{float(res.lpips.max()):.4f}")
    # without "lpips" nothing of lpips.hip is launched and the other figures are what they were
    before = counter.calls
    off = call(b, ("ssim", "psnr"))
    assert counter.calls == before and off.lpips is None
    assert torch.equal(off.videos, res.videos) and torch.equal(off.psnr.view(torch.int64), res.psnr.view(torch.int64))


def test_lpips_without_a_network_is_refused(chain, monkeypatch):
    assert chain.runner.lpips is None
    with pytest.raises(ValueError, match="LpipsNet"):
        call(chain, ("lpips",))
    monkeypatch.setattr(chain.runner, "lpips", object())                         # never reached: the output type is checked first
    with pytest.raises(ValueError, match="uint8"):
        call(chain, ("lpips",), output_type="tensor")
