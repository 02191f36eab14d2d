"""Per-frame quality figures of generated frames against their targets, on the HIP path: SSIM, PSNR, MAE.

The stage-2 driver imports skimage's structural_similarity (stage2_batchtest_rcdms_model.py:23), writes every generated frame
into a `metric_...` directory (:162, :384) and pairs it with its resized target in the comparison grid (:389-401), but never
computes the figure.  Here both rows of that grid are uint8 on the device already (output_type="uint8", Resampler.to_uint8), and
`frame_metrics` compares them where they lie: one rcdm_frame_metrics call (two launches) for n pairs, no download.

  SSIM   scikit-image's structural_similarity(a, b, channel_axis=-1, data_range=255): K1 = 0.01, K2 = 0.03, the mean over the
         window positions inside the image, then over the three channels.  window="uniform": skimage's default 7 x 7 box;
         "gaussian": gaussian_weights=True, sigma=1.5 (11 taps).  sample_covariance: skimage's use_sample_covariance.
         Identical frames give exactly 1.0, and the same inputs always give the same bits (include/rcdm.h, "Frame metrics").
  MSE    mean of (a - b)^2 over all 3 H W bytes, from exact integer sums; PSNR = 10 log10(255^2 / MSE), inf for identical
         frames; MAE the mean of |a - b|.
scikit-image is not a dependency and the definition is restated (tests/ssim_oracle.py), not pinned against skimage itself.

No CPU path: a host tensor raises."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip

WINDOWS = {"uniform": hip.SSIM_UNIFORM7, "gaussian": hip.SSIM_GAUSS11}
WINDOW_SIDE = {"uniform": 7, "gaussian": 11}
SIGMA = 1.5


def gaussian_window():
    """skimage's Gaussian window for sigma 1.5 (truncate 3.5 -> radius 5): 11 float64 taps that sum to 1."""
    i = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


@dataclass
class FrameMetricsResult:
    ssim: torch.Tensor            # (n,) float64: the mean of the three channels, skimage's return value
    ssim_channels: torch.Tensor   # (n, 3) float64
    mse: torch.Tensor             # (n,) float64
    psnr: torch.Tensor            # (n,) float64, inf where the frames are identical
    mae: torch.Tensor             # (n,) float64
    sse: torch.Tensor             # (n, 3) int64: sum of squared differences per channel
    sad: torch.Tensor             # (n, 3) int64: sum of absolute differences per channel


def _window(window):
    if window not in WINDOWS:
        raise ValueError(f"window {window!r}: one of {sorted(WINDOWS)}")
    return window


def _frames(name, t):
    """-> the (n, H, W, 3) device uint8 view the kernel reads: dense pixels, any row pitch, one stride between images."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"`{name}` is a device uint8 tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise ValueError(f"`{name}` is uint8, got {t.dtype}: metrics on float frames are not provided (frames_to_uint8 first)")
    if t.dim() < 3 or t.shape[-1] != 3 or 0 in t.shape:
        raise ValueError(f"`{name}` is (..., H, W, 3), got {tuple(t.shape)}")
    return t


def _view(t):
    H, W = t.shape[-3], t.shape[-2]
    if t.stride(-1) != 1 or (W > 1 and t.stride(-2) != 3) or (H > 1 and t.stride(-3) < 3 * W):
        t = t.contiguous()
    try:
        return t.view(-1, H, W, 3)               # leading axes with one common stride: the cells of one grid row, a batch
    except RuntimeError:
        return t.contiguous().view(-1, H, W, 3)  # e.g. rows x columns of a grid at once: no single image stride


class FrameMetrics:
    """n pairs of H x W frames on one device: the workspace (large enough for either window) and the Gaussian table, kept for
    every call of this shape."""

    def __init__(self, n, H, W, device):
        self.n, self.H, self.W, self.device = int(n), int(H), int(W), torch.device(device)
        if self.device.type != "cuda":
            raise hip.RcdmError("frame_metrics runs on the HIP path only: there is no CPU path here")
        need = 0
        for w in WINDOWS.values():
            need = max(need, hip.frame_metrics_workspace_bytes(self._desc(3 * self.W, 0, 3 * self.W, 0, w, True)))
        if need == 0:
            raise hip.RcdmError(f"rcdm_frame_metrics takes 1..65535 pairs with sides 7..8192, got {self.n} of {self.H}x{self.W}")
        self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.window = torch.from_numpy(gaussian_window()).to(self.device)

    def _desc(self, a_pitch, a_stride, b_pitch, b_stride, window, sample_covariance):
        return hip.MetricsDesc(a_pitch, a_stride, b_pitch, b_stride, self.n, self.H, self.W, 3, window, int(bool(sample_covariance)))

    def launch(self, a, b, ssim, sse, sad, window="uniform", sample_covariance=True):
        """The two launches alone, on the current stream (graph-capturable).  a, b: (n, H, W, 3) uint8 views as `_view` makes
        them; ssim float64 (n, 3), sse / sad int64 (n, 3), dense, on this device."""
        for t in (a, b):
            if tuple(t.shape) != (self.n, self.H, self.W, 3) or t.device != self.device:
                raise ValueError(f"this instance takes ({self.n}, {self.H}, {self.W}, 3) on {self.device}, got {tuple(t.shape)} on {t.device}")
        pitch = lambda t: t.stride(1) if self.H > 1 else 3 * self.W
        stride = lambda t: t.stride(0) if self.n > 1 else 0
        d = self._desc(pitch(a), stride(a), pitch(b), stride(b), WINDOWS[_window(window)], sample_covariance)
        if hip.frame_metrics_workspace_bytes(d) == 0:
            raise hip.RcdmError(f"rcdm_frame_metrics: {self.H}x{self.W} frames are smaller than the {WINDOW_SIDE[window]}-wide "
                                f"{window} window")
        hip.frame_metrics(d, a.data_ptr(), b.data_ptr(), self.window.data_ptr(), ssim.data_ptr(), sse.data_ptr(), sad.data_ptr(),
                          self.workspace.data_ptr(), self.workspace.numel())

    def __call__(self, a, b, window="uniform", sample_covariance=True):
        ssim = torch.empty(self.n, 3, dtype=torch.float64, device=self.device)
        sse = torch.empty(self.n, 3, dtype=torch.int64, device=self.device)
        sad = torch.empty(self.n, 3, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self.launch(a, b, ssim, sse, sad, window, sample_covariance)
        count = float(3 * self.H * self.W)
        mse = sse.sum(dim=1).to(torch.float64) / count
        return FrameMetricsResult(ssim=ssim.mean(dim=1), ssim_channels=ssim, mse=mse, psnr=10.0 * torch.log10(255.0 ** 2 / mse),
                                  mae=sad.sum(dim=1).to(torch.float64) / count, sse=sse, sad=sad)


_INSTANCES = {}


def frame_metrics_for(n, H, W, device):
    device = torch.device(device)
    key = (int(n), int(H), int(W), device)
    m = _INSTANCES.get(key)
    if m is None:
        m = _INSTANCES[key] = FrameMetrics(n, H, W, device)
    return m


def frame_metrics(a, b, window="uniform", sample_covariance=True):
    """a, b: device uint8 tensors (..., H, W, 3) of one shape, RGB (or any three channels in one order); leading axes are
    flattened to n pairs.  Any row pitch with dense pixels is read where it lies — a cell sliced out of a grid image, the
    cells of one grid row — without a copy; a and b may differ in pitch.  -> FrameMetricsResult of device tensors."""
    a, b = _frames("a", a), _frames("b", b)
    if a.shape != b.shape:
        raise ValueError(f"`a` {tuple(a.shape)} and `b` {tuple(b.shape)} differ in shape")
    _window(window)
    if not a.is_cuda or not b.is_cuda:
        raise hip.RcdmError("frame_metrics runs on the HIP path only: a and b must be device tensors (there is no CPU path here)")
    if a.device != b.device:
        raise ValueError(f"`a` is on {a.device}, `b` on {b.device}")
    va, vb = _view(a), _view(b)
    return frame_metrics_for(va.shape[0], va.shape[1], va.shape[2], va.device)(va, vb, window, sample_covariance)


def ssim(a, b, window="uniform", sample_covariance=True):
    """(n,) float64: skimage's structural_similarity(a[i], b[i], channel_axis=-1, data_range=255)."""
    return frame_metrics(a, b, window, sample_covariance).ssim


def psnr(a, b):
    """(n,) float64: 10 log10(255^2 / MSE), inf for identical frames."""
    return frame_metrics(a, b).psnr
