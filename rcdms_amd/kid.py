"""Set-level quality of generated frames on the HIP path, for few samples: the kernel distance (KID).

The Fréchet distance of rcdms_amd.frechet is strongly biased when a set is a few hundred frames against d = 1280 features.  Its
standard companion there is the Kernel Inception Distance (Binkowski et al., "Demystifying MMD GANs", 2018): the unbiased
squared maximum mean discrepancy under the polynomial kernel k(x, y) = (gamma <x, y> + c)^p, averaged over random subsets of
the features and reported as a mean and a spread.  It needs no covariance and no factorisation — but it needs the rows:

  FeatureBank       keeps feature rows on the device (FeatureStats keeps only moments); StoryRunner(..., feature_banks=...) fills two.
                    radii2(k) caches the k-nearest-neighbour radii of rcdms_amd.prdc.
  draw_subsets      this project's rule for the random subsets (numpy's RandomState, see there).
  polynomial_mmd    Sxx, Syy, Sxy and mmd^2 of every subset: one launch of the tile kernel (float64 matrix pipe, rows gathered
                    through the index lists) and one of the reduce (csrc/kid.hip; csrc/kid_core.h has the definition).
  kernel_distance   banks or tensors -> KernelDistanceResult(mean, std, values, ...): one upload of the indices, one read-back of
                    `subsets` doubles, mean and standard deviation on the host in a fixed order.

The figure does not care where the features come from; from the CLIP vision tower built in here it is a CLIP-KID, not an
Inception KID.  Parity: restated from the definition (tests/kid_oracle.py, 60-digit goldens), unpinned against torch-fidelity /
torchmetrics / clean-fid: none is a dependency.

No CPU path: a host tensor raises."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from .frechet import FeatureStats, _device

MAX_DIM = hip.FRECHET_MAX_DIM
MAX_M, MAX_SUBSETS, MAX_DEGREE = hip.KID_MAX_M, hip.KID_MAX_SUBSETS, hip.KID_MAX_DEGREE


@dataclass
class KernelDistanceResult:
    mean: float            # the mean of the subsets' mmd^2: the figure reported as KID
    std: float             # their population standard deviation (ddof = 0)
    values: tuple          # mmd^2 of every subset, in order
    subsets: int
    subset_size: int


class FeatureBank:
    """Feature rows of one width kept on one device, appended as they come."""

    def __init__(self, d, device, dtype=torch.float32):
        self.d, self.device = int(d), _device(device)
        if not 1 <= self.d <= MAX_DIM:
            raise ValueError(f"d is 1..{MAX_DIM}, got {d}")
        if dtype not in (torch.float32, torch.float16):
            raise ValueError(f"a bank holds float32 or float16 rows, got {dtype}")
        self.dtype = dtype
        self.n = 0
        self._buf = None           # (capacity, d), the first n rows live
        self._radii2 = {}          # k -> (n,) float64 squared k-nearest-neighbour radii of the rows held (radii2)

    def append(self, feats):
        """feats: (..., d) float32 or float16 on this device, rows of any pitch.  float16 rows into a float32 bank are widened
        exactly; float32 rows into a float16 bank are refused."""
        if not isinstance(feats, torch.Tensor):
            raise TypeError(f"`feats` is a device tensor, got {type(feats).__name__}")
        if not feats.is_cuda:
            raise hip.RcdmError("feature banks live on the HIP path only: `feats` must be a device tensor")
        if feats.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"`feats` is float32 or float16, got {feats.dtype}")
        if feats.dtype == torch.float32 and self.dtype == torch.float16:
            raise ValueError("float32 rows do not go into a float16 bank: they would be rounded")
        if feats.dim() < 1 or feats.shape[-1] != self.d or feats.numel() == 0:
            raise ValueError(f"`feats` is (..., {self.d}) with at least one row, got {tuple(feats.shape)}")
        if self.device.index is None:
            self.device = feats.device
        if feats.device != self.device:
            raise ValueError(f"`feats` is on {feats.device}, the bank on {self.device}")
        x = feats.reshape(-1, self.d)
        need = self.n + x.shape[0]
        if self._buf is None or need > self._buf.shape[0]:
            cap = max(need, 2 * (0 if self._buf is None else self._buf.shape[0]), 64)      # geometric growth
            buf = torch.empty(cap, self.d, dtype=self.dtype, device=self.device)
            if self.n:
                buf[:self.n] = self._buf[:self.n]
            self._buf = buf
        self._buf[self.n:need] = x               # copy_ widens float16 exactly
        self.n = need
        self._radii2.clear()
        return self

    def __len__(self):
        return self.n

    def rows(self):
        """(n, d), a view of the rows held."""
        if self._buf is None:
            return torch.empty(0, self.d, dtype=self.dtype, device=self.device if self.device.index is not None else "cpu")
        return self._buf[:self.n]

    def clear(self):
        self.n = 0
        self._radii2.clear()
        return self

    def radii2(self, k):
        """(n,) float64 device tensor: the squared distance of every row to its k-th nearest other row (rcdms_amd.prdc), kept per
        k until the next append or clear — a reference set is swept once, as FeatureStats keeps its factor."""
        from . import prdc
        k = prdc._k(k)
        if k not in self._radii2:
            self._radii2[k] = prdc._radii2(prdc._rows(self.rows(), "bank", k), k)
        return self._radii2[k]

    def stats(self):
        """A FeatureStats of the same rows (for frechet_distance)."""
        if self.n < 1:
            raise ValueError("no rows yet")
        return FeatureStats(self.d, self.device).update(self.rows())

    def save(self, path):
        """.npz with `features`."""
        np.savez(path, features=self.rows().cpu().numpy())

    @classmethod
    def load(cls, path, device):
        with np.load(path) as z:
            f = z["features"]
        if f.ndim != 2 or f.dtype not in (np.float32, np.float16):
            raise ValueError(f"`features` is (n, d) float32 or float16, got {f.dtype} {f.shape}")
        self = cls(f.shape[1], device, torch.float16 if f.dtype == np.float16 else torch.float32)
        if f.shape[0]:
            self.append(torch.from_numpy(f).to(self.device))
        return self


def draw_subsets(na, nb, subsets, m, seed):
    """The index lists of `subsets` random subsets of m rows out of na and out of nb -> two int32 arrays (subsets, m).
    This project's rule (no KID implementation's draws are reproduced): rng = numpy.random.RandomState(seed); per subset, first
    rng.choice(na, m, replace=False), then rng.choice(nb, m, replace=False)."""
    na, nb, subsets, m = int(na), int(nb), int(subsets), int(m)
    if m < 2:
        raise ValueError(f"a subset has at least 2 rows, got {m}")
    if m > na or m > nb:
        raise ValueError(f"a subset of {m} rows cannot be drawn without replacement from sets of {na} and {nb}")
    if subsets < 1:
        raise ValueError(f"at least one subset, got {subsets}")
    rng = np.random.RandomState(seed)
    ia, ib = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(subsets):
        ia[s] = rng.choice(na, m, replace=False)
        ib[s] = rng.choice(nb, m, replace=False)
    return ia, ib


def _rows(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"`{name}` is a device tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise hip.RcdmError(f"the kernel distance runs on the HIP path only: `{name}` must be a device tensor")
    if t.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"`{name}` is float32 or float16, got {t.dtype}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"`{name}` is (n, d), got {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _list(idx, name, n, device):
    """A caller's index list -> int32 (subsets, m) on the device, every entry checked against n: on the host for a host array,
    with one device-side min / max (one read-back) for a device tensor."""
    on_device = isinstance(idx, torch.Tensor) and idx.is_cuda
    t = idx if on_device else torch.as_tensor(np.asarray(idx))
    if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"`{name}` holds integers, got {t.dtype}")
    t = t if t.dim() == 2 else t.reshape(1, -1)
    if t.shape[1] < 2:
        raise ValueError(f"`{name}`: a subset has at least 2 rows")
    lo, hi = torch.stack(torch.aminmax(t)).tolist()             # before the cast to int32: nothing wraps into range
    if lo < 0 or hi >= n:
        raise ValueError(f"`{name}` indexes rows {lo}..{hi} of a set of {n}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def polynomial_mmd(x, y, ia=None, ib=None, degree=3, gamma=None, coef0=1.0):
    """x (nx, d), y (ny, d): device tensors of one dtype, float32 or float16; rows may be strided.  ia, ib: (subsets, m) index
    lists into their rows (arrays or tensors; checked), or both None: one subset of rows 0 .. m - 1 with m = min(nx, ny).
    gamma: default 1 / d.  -> (subsets, 4) float64 device tensor: Sxx, Syy, Sxy, mmd^2 per subset.  No read-back (but the one of
    the min / max of index lists given as device tensors)."""
    x, y = _rows(x, "x"), _rows(y, "y")
    if (ia is None) != (ib is None):
        raise ValueError("give both index lists or neither")
    if ia is not None:
        ia, ib = _list(ia, "ia", x.shape[0], x.device), _list(ib, "ib", y.shape[0], x.device)
    return _mmd(x, y, ia, ib, degree, gamma, coef0)


def _mmd(x, y, ia, ib, degree, gamma, coef0):
    """x, y from _rows; ia, ib: int32 (subsets, m) on the device with every entry in range, or None."""
    if x.dtype != y.dtype or x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y are rows of one dtype and width, got {x.dtype} {tuple(x.shape)} and {y.dtype} {tuple(y.shape)}")
    if x.device != y.device:
        raise ValueError(f"`x` is on {x.device}, `y` on {y.device}")
    degree = int(degree)
    if not 1 <= degree <= MAX_DEGREE:
        raise ValueError(f"degree is 1..{MAX_DEGREE}, got {degree}")
    nx, ny, d = x.shape[0], y.shape[0], x.shape[1]
    if d > MAX_DIM:
        raise ValueError(f"d is 1..{MAX_DIM}, got {d}")
    dev = x.device
    if ia is None:
        subsets, m = 1, min(nx, ny)
    else:
        if ia.shape != ib.shape:
            raise ValueError(f"the index lists differ in shape: {tuple(ia.shape)} and {tuple(ib.shape)}")
        subsets, m = ia.shape
    if not 2 <= m <= MAX_M:
        raise ValueError(f"a subset has 2..{MAX_M} rows, got {m}")
    if not 1 <= subsets <= MAX_SUBSETS:
        raise ValueError(f"1..{MAX_SUBSETS} subsets, got {subsets}")
    gamma = 1.0 / d if gamma is None else float(gamma)
    desc = hip.MmdDesc(x.stride(0) if nx > 1 else d, y.stride(0) if ny > 1 else d, nx, ny, d, subsets, m, degree,
                       hip.FSTATS_F16 if x.dtype == torch.float16 else hip.FSTATS_F32, gamma, float(coef0), 0)
    need = hip.poly_mmd_workspace_bytes(desc)
    if need == 0:
        raise hip.RcdmError(f"rcdm_poly_mmd refused {subsets} subsets of {m} rows of {d} features")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(subsets, 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.poly_mmd(desc, x.data_ptr(), y.data_ptr(), hip.ptr(ia), hip.ptr(ib), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def _set(v, name):
    if isinstance(v, FeatureBank):
        if len(v) < 1:
            raise ValueError(f"`{name}` holds no rows yet")
        return v.rows()
    return v


def kernel_distance(a, b, subsets=100, subset_size=None, degree=3, gamma=None, coef0=1.0, seed=0, indices=None):
    """a, b: FeatureBanks or (n, d) device tensors (`a is b` is allowed) -> KernelDistanceResult (host floats; the arithmetic ran
    on the device).  subset_size: rows per subset, default min(1000, len(a), len(b)).  The subsets are draw_subsets(len(a),
    len(b), subsets, subset_size, seed), or `indices` = (ia, ib), two (subsets, m) lists of the caller's (then `subsets`,
    `subset_size` and `seed` are not used)."""
    xa, xb = _set(a, "a"), _set(b, "b")
    for v, name in ((xa, "a"), (xb, "b")):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"`{name}` is a FeatureBank or a device tensor, got {type(v).__name__}")
        if v.dim() != 2:
            raise ValueError(f"`{name}` is (n, d), got {tuple(v.shape)}")
    na, nb = xa.shape[0], xb.shape[0]
    if indices is None:
        m = min(1000, na, nb) if subset_size is None else int(subset_size)
        if m < 2:
            raise ValueError(f"a subset has at least 2 rows, got {m} (sets of {na} and {nb} rows)")
        if m > na or m > nb:
            raise ValueError(f"subset_size {m} is above the rows there are ({na} and {nb})")
        if not 1 <= int(subsets) <= MAX_SUBSETS:
            raise ValueError(f"1..{MAX_SUBSETS} subsets, got {subsets}")
        xa, xb = _rows(xa, "a"), _rows(xb, "b")
        both = torch.from_numpy(np.stack(draw_subsets(na, nb, subsets, m, seed))).to(xa.device)      # the one upload
        out = _mmd(xa, xb, both[0], both[1], degree, gamma, coef0)               # drawn here: in range by construction
    else:
        if len(indices) != 2:
            raise ValueError("`indices` is a pair (ia, ib) of (subsets, m) index lists")
        out = polynomial_mmd(xa, xb, indices[0], indices[1], degree, gamma, coef0)
    values = tuple(out[:, 3].tolist())                                           # the one read-back
    n = len(values)
    total = 0.0
    for v in values:
        total = total + v
    mean = total / n
    sq = 0.0
    for v in values:
        sq = sq + (v - mean) * (v - mean)
    return KernelDistanceResult(mean=mean, std=math.sqrt(sq / n), values=values, subsets=n,
                                subset_size=m if indices is None else int(np.shape(indices[0])[-1]))
