"""Fidelity and diversity of generated frames on the HIP path: the k-nearest-neighbour manifold figures.

One distance (rcdms_amd.frechet, rcdms_amd.kid) cannot say whether a model lost fidelity or lost diversity.  The standard split is
improved precision and recall (Kynkaanniemi et al., 2019) and density and coverage (Naeem et al., 2020), all four from the
k-th-nearest-neighbour balls of the real rows X and the generated rows Y:

  radius      rX2[i] = the k-th smallest squared distance of X_i to the OTHER rows of X (by position: a repeated row is its twin's
              neighbour at distance 0); rY2 the same over Y.
  precision   the share of generated rows inside some real ball          recall    the share of real rows inside some generated ball
  density     real balls holding a generated row, per generated row and k
  coverage    the share of real rows whose nearest generated row lies inside their own ball
  balls       closed (<=) everywhere, on squared distances in float64; csrc/prdc_core.h has every rule.  The prdc package
              compares strictly: the two differ on exact ties only.

  knn_radii2        (n, d) rows -> (n,) float64 squared radii: the distance matrix is formed tile by tile on the float64 matrix
                    pipe and never reaches memory (csrc/prdc.hip).
  manifold_metrics  banks or tensors -> PrdcResult: two radius sweeps (one if the bank has its radii cached, see
                    FeatureBank.radii2), one count sweep, one read-back of four int64.

nearest_k defaults to 5, the choice of the density / coverage paper; the precision / recall paper uses 3.  The figures do not
care where the features come from.  Parity: restated from the papers (tests/prdc_oracle.py, exact integer cases and goldens),
unpinned against prdc / torch-fidelity / torchmetrics: none is a dependency.

No CPU path: a host tensor raises."""
from dataclasses import dataclass

import torch

from . import hip
from .kid import FeatureBank

MAX_DIM, MAX_K, MAX_N = hip.FRECHET_MAX_DIM, hip.PRDC_MAX_K, hip.PRDC_MAX_N


@dataclass
class PrdcResult:
    precision: float
    recall: float
    density: float
    coverage: float
    counts: tuple                  # the four int64 numerators, in that order
    n_real: int
    n_fake: int
    nearest_k: int
    fake_count: torch.Tensor       # (n_fake,) int32: real balls that hold generated row j
    real_hit: torch.Tensor         # (n_real,) int32: 1 where real row i lies in some generated ball
    real_min2: torch.Tensor        # (n_real,) float64: squared distance of real row i to its nearest generated row
    radii2_real: torch.Tensor      # (n_real,) float64
    radii2_fake: torch.Tensor      # (n_fake,) float64


def _k(k):
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"nearest_k is an integer in 1..{MAX_K}, got {k!r}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"nearest_k is 1..{MAX_K}, got {k}")
    return k


def _check(t, name, k):
    """Everything about one set that needs no device: a wrong type, dtype, shape or size is an error on any machine."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"`{name}` is a FeatureBank or a device tensor, got {type(t).__name__}")
    if t.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"`{name}` is float32 or float16, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"`{name}` is (n, d), got {tuple(t.shape)}")
    if t.shape[1] > MAX_DIM:
        raise ValueError(f"d is 1..{MAX_DIM}, got {t.shape[1]}")
    if t.shape[0] < k + 1:
        raise ValueError(f"`{name}` needs at least nearest_k + 1 = {k + 1} rows, got {t.shape[0]}")
    if t.shape[0] > MAX_N:
        raise ValueError(f"`{name}` holds at most {MAX_N} rows, got {t.shape[0]}")
    return t


def _rows(t, name, k):
    """The checks of kid._rows plus this module's sizes -> rows a kernel can read."""
    t = _check(t, name, k)
    if not t.is_cuda:
        raise hip.RcdmError(f"the manifold figures run on the HIP path only: `{name}` must be a device tensor")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _code(t):
    return hip.FSTATS_F16 if t.dtype == torch.float16 else hip.FSTATS_F32


def _radii2(x, k, col_chunks=0):
    """x from _rows -> (n,) float64 on its device.  No read-back."""
    n, d = x.shape
    desc = hip.KnnDesc(x.stride(0), n, d, k, _code(x), int(col_chunks), 0)
    need = hip.knn_radii2_workspace_bytes(desc)
    if need == 0:
        raise hip.RcdmError(f"rcdm_knn_radii2 refused {n} rows of {d} features at k = {k}, col_chunks = {col_chunks}")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    r2 = torch.empty(n, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        hip.knn_radii2(desc, x.data_ptr(), r2.data_ptr(), ws.data_ptr(), ws.numel())
    return r2


def _counts(x, y, rx2, ry2, col_chunks=0):
    """x, y from _rows, their radii -> (the four int64 numerators, fake_count, real_hit, real_min2) on the device.  No read-back."""
    nx, ny, d = x.shape[0], y.shape[0], x.shape[1]
    dev = x.device
    desc = hip.PrdcDesc(x.stride(0), y.stride(0), nx, ny, d, _code(x), int(col_chunks), 0)
    need = hip.prdc_counts_workspace_bytes(desc)
    if need == 0:
        raise hip.RcdmError(f"rcdm_prdc_counts refused {nx} x {ny} rows of {d} features, col_chunks = {col_chunks}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.int64, device=dev)
    fake_count = torch.empty(ny, dtype=torch.int32, device=dev)
    real_hit = torch.empty(nx, dtype=torch.int32, device=dev)
    real_min2 = torch.empty(nx, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.prdc_counts(desc, x.data_ptr(), y.data_ptr(), rx2.data_ptr(), ry2.data_ptr(), out.data_ptr(), fake_count.data_ptr(),
                        real_hit.data_ptr(), real_min2.data_ptr(), ws.data_ptr(), ws.numel())
    return out, fake_count, real_hit, real_min2


def knn_radii2(x, k, col_chunks=0):
    """x: (n, d) device tensor, float32 or float16, rows may be strided; k: 1..16, n >= k + 1.  -> (n,) float64 device tensor, the
    squared distance of every row to its k-th nearest OTHER row.  col_chunks: 0 lets the library split the columns over the
    device; the result does not depend on it."""
    k = _k(k)
    return _radii2(_rows(x, "x", k), k, col_chunks)


def _set(v, name, k):
    """-> the rows of a bank or the tensor itself, checked as far as no device is needed."""
    if isinstance(v, FeatureBank):
        if len(v) < 1:
            raise ValueError(f"`{name}` holds no rows yet")
        return _check(v.rows(), name, k)
    return _check(v, name, k)


def manifold_metrics(real, fake, nearest_k=5, col_chunks=0):
    """real, fake: FeatureBanks or (n, d) device tensors of one dtype and width (`real is fake` is allowed) -> PrdcResult.
    The four figures are host floats — four int64 numerators read back once and divided in float64 —, the per-sample vectors
    and the radii stay on the device.  nearest_k: 5 (density / coverage) by default; 3 is the precision / recall paper's."""
    k = _k(nearest_k)
    x = _set(real, "real", k)
    y = x if fake is real else _set(fake, "fake", k)
    if x.dtype != y.dtype or x.shape[1] != y.shape[1]:
        raise ValueError(f"real and fake are rows of one dtype and width, got {x.dtype} {tuple(x.shape)} and {y.dtype} {tuple(y.shape)}")
    x = _rows(x, "real", k)
    y = x if fake is real else _rows(y, "fake", k)
    if x.device != y.device:
        raise ValueError(f"`real` is on {x.device}, `fake` on {y.device}")
    rx2 = real.radii2(k) if isinstance(real, FeatureBank) else _radii2(x, k, col_chunks)          # a bank's come from its cache
    ry2 = rx2 if fake is real else fake.radii2(k) if isinstance(fake, FeatureBank) else _radii2(y, k, col_chunks)
    out, fake_count, real_hit, real_min2 = _counts(x, y, rx2, ry2, col_chunks)
    nx, ny = x.shape[0], y.shape[0]
    counts = tuple(int(v) for v in out.tolist())                                 # the one read-back
    return PrdcResult(precision=counts[0] / float(ny), recall=counts[1] / float(nx), density=counts[2] / float(k * ny),
                      coverage=counts[3] / float(nx), counts=counts, n_real=nx, n_fake=ny, nearest_k=k, fake_count=fake_count,
                      real_hit=real_hit, real_min2=real_min2, radii2_real=rx2, radii2_fake=ry2)
