"""Set-level quality of generated frames on the HIP path: running float64 feature statistics and the Fréchet distance.

Story-visualisation work reports a Fréchet distance (FID) first; the reference drivers leave it to an outside script that
downloads features, runs numpy.cov and takes scipy.linalg.sqrtm of a d x d product.  Here the features stay on the device:

  FeatureStats      n, sum (x - k) and sum (x - k)(x - k)^T in float64 about a float32 shift k, updated by rcdm_feature_stats_update
                    (the outer product on the float64 matrix pipe, fixed order, no atomics); mean() and cov() from them.
  frechet_distance  |mu_a - mu_b|^2 + tr Sa + tr Sb - 2 tr (Sa Sb)^(1/2), the last term as the sum of the singular values of
                    Fb^T Fa with S = F F^T.  Factors and singular values come from one-sided Jacobi on the device
                    (csrc/frechet_core.h); no square root of a matrix is taken, and a rank-deficient covariance (n < d) costs
                    no accuracy.  A statistics object keeps its factor until its next update: a reference set is factored once.
                    factor="cholesky" (opt-in) takes both factors from a diagonally pivoted Cholesky factorisation instead
                    (rcdm_cholesky_pivoted_f64: O(d) launches, the trailing updates on the float64 matrix pipe, no sweeps) and
                    rotates only the rank_b x rank_a block of Fb^T Fa: any F with S = F F^T serves the formula.

The distance does not care where the features come from: pytorch-fid's `mu` / `sigma` .npz files load with FeatureStats.load.
The extractor built in here is the CLIP vision tower (StoryRunner(..., feature_stats=...)), so that figure is a CLIP-FD, not
an Inception FID.  Parity: restated from the definition (tests/frechet_oracle.py, 60-digit goldens); not pinned against
pytorch-fid, which is not a dependency.

No CPU path: a host tensor raises."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip

MAX_DIM = hip.FRECHET_MAX_DIM
MAX_SWEEPS = 30


@dataclass
class FrechetResult:
    distance: float        # may be a rounding error below zero for near-identical sets: never clamped
    mean_term: float       # |mu_a - mu_b|^2
    trace_a: float
    trace_b: float
    sqrt_trace: float      # tr (Sa Sb)^(1/2)
    rank_a: int            # numerical ranks of the two covariances (rule 3)
    rank_b: int
    sweeps: tuple          # Jacobi sweeps of (factor a, factor b, singular values); 0 for a factor that was cached or is a Cholesky factor
    block: tuple = None    # (vectors, length) of the buffer the singular-value run rotated; None when there was no such run


def _device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.RcdmError("feature statistics run on the HIP path only: there is no CPU path here")
    if device.index is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _jacobi(w, rows, length, dim, count):
    """Sweeps over w (rows x length, dense) until one rotates nothing.  -> (descriptor, its workspace, sweeps)."""
    desc = hip.JacobiDesc(length, rows, length, dim, 0)
    need = hip.jacobi_workspace_bytes(desc)
    if need == 0:
        raise hip.RcdmError(f"rcdm_jacobi_sweep takes an even number of 2..{MAX_DIM} vectors of 1..{MAX_DIM}, got {rows} of {length}")
    ws = torch.empty(need, dtype=torch.uint8, device=w.device)
    for sweep in range(1, MAX_SWEEPS + 1):
        hip.jacobi_sweep(desc, w.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel())
        if int(count.item()) == 0:        # the one readback of the sweep
            return desc, ws, sweep
    raise hip.RcdmError(f"one-sided Jacobi did not converge in {MAX_SWEEPS} sweeps ({rows} vectors of {length})")


class FeatureStats:
    """Running statistics of d-dimensional feature rows on one device."""

    def __init__(self, d, device, shift=None):
        self.d, self.device = int(d), _device(device)
        if not 1 <= self.d <= MAX_DIM:
            raise ValueError(f"d is 1..{MAX_DIM}, got {d}")
        self.n = 0
        self.shift = None if shift is None else torch.as_tensor(shift, dtype=torch.float32).to(self.device).reshape(self.d).contiguous()
        self.sum = self.outer = None     # (d,) and (d, d) float64, allocated with the first rows
        self._moments = None       # (mean, cov or None, trace or None) of the current sums
        self._given = False        # from_moments: the moments are the data, there are no sums yet
        self._factor = None        # (F (d x rows), rank) from one-sided Jacobi
        self._factor_chol = None   # (F (d x rows), rank) from the pivoted Cholesky factorisation: never handed out for the other

    # ---- accumulation ----
    def update(self, feats):
        """feats: (..., d) float32 or float16 on this device; rows may be strided (dense features, any pitch)."""
        if not isinstance(feats, torch.Tensor):
            raise TypeError(f"`feats` is a device tensor, got {type(feats).__name__}")
        if not feats.is_cuda:
            raise hip.RcdmError("feature statistics run on the HIP path only: `feats` must be a device tensor")
        if feats.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"`feats` is float32 or float16, got {feats.dtype}")
        if feats.dim() < 1 or feats.shape[-1] != self.d or feats.numel() == 0:
            raise ValueError(f"`feats` is (..., {self.d}) with at least one row, got {tuple(feats.shape)}")
        if self.device.index is None:
            self.device = feats.device             # "cuda": the device of the first rows
        if feats.device != self.device:
            raise ValueError(f"`feats` is on {feats.device}, the statistics on {self.device}")
        self._sums()
        self._alloc()
        x = feats if feats.dim() == 2 else feats.reshape(-1, self.d)
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < self.d):
            x = x.contiguous()
        n = x.shape[0]
        ld = x.stride(0) if n > 1 else self.d
        if self.shift is None:
            self.shift = x.to(torch.float64).mean(dim=0).to(torch.float32)
        desc = hip.FStatsDesc(ld, n, self.d, hip.FSTATS_F16 if x.dtype == torch.float16 else hip.FSTATS_F32, 0)
        with torch.cuda.device(self.device):
            hip.feature_stats_update(desc, x.data_ptr(), self.shift.data_ptr(), self.sum.data_ptr(), self.outer.data_ptr())
        self.n += n
        self._moments = self._factor = self._factor_chol = None
        return self

    def merge(self, other):
        """Add the rows `other` has seen (statistics of a shard from another process, moved to this device), re-centred to
        this object's shift."""
        if other.d != self.d:
            raise ValueError(f"d differs: {self.d} and {other.d}")
        self._sums()
        other._sums()
        if other.n == 0:
            return self
        self._alloc()
        if self.shift is None:
            self.shift = other.shift.to(self.device).clone()
        osum, oouter = other.sum.to(self.device), other.outer.to(self.device)
        delta = other.shift.to(self.device, torch.float64) - self.shift.to(torch.float64)
        cross = torch.outer(delta, osum)
        self.outer += oouter + cross + cross.T + other.n * torch.outer(delta, delta)
        self.sum += osum + other.n * delta
        self.n += other.n
        self._moments = self._factor = self._factor_chol = None
        return self

    def _alloc(self):
        if self.sum is None:
            self.sum = torch.zeros(self.d, dtype=torch.float64, device=self.device)
            self.outer = torch.zeros(self.d, self.d, dtype=torch.float64, device=self.device)

    def _sums(self):
        """Moments that were given (from_moments, load) become sums about the float32-rounded mean, so that rows can be added."""
        if not self._given:
            return
        mean, cov, _ = self._moments
        if self.n < 2 or cov is None:
            raise ValueError("these statistics were built from moments without a row count n >= 2: rows cannot be added to them")
        self.shift = mean.to(torch.float32)
        self.sum = self.n * (mean - self.shift.to(torch.float64))
        self.outer = (self.n - 1) * cov + torch.outer(self.sum, self.sum) / self.n
        self._given = False

    # ---- moments ----
    def _finalize(self):
        if self._moments is None:
            if self.n < 1:
                raise ValueError("no rows yet")
            mean = torch.empty(self.d, dtype=torch.float64, device=self.device)
            cov = trace = None
            if self.n >= 2:
                cov = torch.empty(self.d, self.d, dtype=torch.float64, device=self.device)
                trace = torch.empty(1, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                hip.feature_stats_finalize(self.d, self.n, self.shift.data_ptr(), self.sum.data_ptr(), self.outer.data_ptr(),
                                           mean.data_ptr(), hip.ptr(cov), hip.ptr(trace))
            self._moments = (mean, cov, trace)
        return self._moments

    def mean(self):
        return self._finalize()[0]

    def cov(self):
        """(d, d) float64, the sample covariance (n - 1 in the denominator, as numpy.cov), symmetric bit for bit."""
        if not self._given and self.n < 2:
            raise ValueError(f"a covariance needs n >= 2 rows, got {self.n}")
        return self._finalize()[1]

    def trace(self):
        self.cov()
        mean, cov, trace = self._moments
        if trace is None:
            trace = torch.empty(1, dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                hip.frechet_trace(self.d, cov.data_ptr(), trace.data_ptr())
            self._moments = (mean, cov, trace)
        return trace

    @classmethod
    def from_moments(cls, mu, sigma, n=None, device=None):
        """Statistics that ARE the given mean (d,) and covariance (d, d): arrays or tensors, e.g. of Inception features computed
        elsewhere.  n: the rows behind them, where known (needed only to add more rows)."""
        mu, sigma = torch.as_tensor(mu), torch.as_tensor(sigma)
        device = device if device is not None else mu.device
        self = cls(mu.shape[-1], device)
        if mu.dim() != 1 or tuple(sigma.shape) != (self.d, self.d):
            raise ValueError(f"mu is (d,), sigma (d, d), got {tuple(mu.shape)} and {tuple(sigma.shape)}")
        self._moments = (mu.to(self.device, torch.float64).contiguous(), sigma.to(self.device, torch.float64).contiguous(), None)
        self._given = True
        self.n = 0 if n is None else int(n)
        return self

    def save(self, path):
        """.npz with `mu`, `sigma` (pytorch-fid's keys) and `n`."""
        np.savez(path, mu=self.mean().cpu().numpy(), sigma=self.cov().cpu().numpy(), n=np.int64(self.n))

    @classmethod
    def load(cls, path, device):
        with np.load(path) as z:
            n = int(z["n"]) if "n" in z.files else None
            return cls.from_moments(z["mu"], z["sigma"], n, device=device)

    # ---- the factor ----
    def factor(self, method="jacobi"):
        """-> (F (d, rows) float64 with cov = F F^T, numerical rank, sweeps run: 0 when F was cached).
        method "jacobi": columns lambda_j^(1/2) v_j from one-sided Jacobi on cov.  "cholesky": columns of P L from the diagonally
        pivoted Cholesky factorisation, the leading `rank` columns non-zero; no sweeps.  Each method keeps its own cache."""
        if method not in ("jacobi", "cholesky"):
            raise ValueError(f'`method` is "jacobi" or "cholesky", got {method!r}')
        if method == "cholesky":
            return self._cholesky()
        if self._factor is not None:
            return (*self._factor, 0)
        cov = self.cov()
        d = self.d
        rows = d + (d & 1)
        w = torch.zeros(rows, d, dtype=torch.float64, device=self.device)
        w[:d] = cov
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        f = torch.empty(d, rows, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            desc, ws, sweeps = _jacobi(w, rows, d, d, count)
            hip.frechet_factor(desc, w.data_ptr(), f.data_ptr(), rows, count.data_ptr(), ws.data_ptr(), ws.numel())
        self._factor = (f, int(count.item()))
        return (*self._factor, sweeps)

    def _cholesky(self):
        if self._factor_chol is None:
            cov = self.cov()
            d = self.d
            rows = d + (d & 1)
            desc = hip.CholeskyDesc(d, rows, d, 0)
            ws = torch.empty(hip.cholesky_workspace_bytes(desc), dtype=torch.uint8, device=self.device)
            f = torch.zeros(d, rows, dtype=torch.float64, device=self.device)      # the entry writes d columns: the pad one stays 0
            rank = torch.zeros(1, dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                hip.cholesky_pivoted_f64(desc, cov.data_ptr(), f.data_ptr(), rank.data_ptr(), ws.data_ptr(), ws.numel())
            self._factor_chol = (f, int(rank.item()))                              # the one readback
        return (*self._factor_chol, 0)


def frechet_distance(a, b, factor="jacobi"):
    """a, b: FeatureStats of one dimension on one device -> FrechetResult (host floats; the arithmetic ran on the device).
    factor: how S = F F^T is formed, "jacobi" (the default) or "cholesky" (FeatureStats.factor)."""
    if factor not in ("jacobi", "cholesky"):
        raise ValueError(f'`factor` is "jacobi" or "cholesky", got {factor!r}')
    if a.d != b.d:
        raise ValueError(f"d differs: {a.d} and {b.d}")
    if a.device != b.device:
        raise ValueError(f"`a` is on {a.device}, `b` on {b.device}")
    d, dev = a.d, a.device
    rows = d + (d & 1)
    if factor == "cholesky":
        return _distance_cholesky(a, b)
    fa, rank_a, sweeps_a = a.factor()
    fb, rank_b, sweeps_b = (fa, rank_a, 0) if b is a else b.factor()
    m = torch.empty(rows, rows, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.gemm_tn_f64(rows, rows, d, fb.data_ptr(), rows, fa.data_ptr(), rows, m.data_ptr(), rows)
        desc, ws, sweeps_m = _jacobi(m, rows, rows, d, count)
        hip.jacobi_norm_sum(desc, m.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel())
        hip.frechet_mean_term(d, a.mean().data_ptr(), b.mean().data_ptr(), out[2:].data_ptr())
    sqrt_trace, _, mean_term, _ = out.tolist()
    trace_a, trace_b = float(a.trace().item()), float(b.trace().item())
    return FrechetResult(distance=((mean_term + trace_a) + trace_b) - 2.0 * sqrt_trace, mean_term=mean_term, trace_a=trace_a,
                         trace_b=trace_b, sqrt_trace=sqrt_trace, rank_a=rank_a, rank_b=rank_b, sweeps=(sweeps_a, sweeps_b, sweeps_m),
                         block=(rows, rows))


def _distance_cholesky(a, b):
    """The non-zero columns of a Cholesky factor are its leading `rank` ones, so Fb^T Fa is the rank_b x rank_a block (rank_b rounded
    up to even: the next column of Fb is zero) and the sweeps run over that alone, with dim = d for rules 2 and 3."""
    d, dev = a.d, a.device
    rows = d + (d & 1)
    fa, rank_a, _ = a.factor("cholesky")
    fb, rank_b = (fa, rank_a) if b is a else b.factor("cholesky")[:2]
    rows_b = rank_b + (rank_b & 1)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    sweeps_m, block = 0, None
    with torch.cuda.device(dev):
        if rank_a and rank_b:
            m = torch.empty(rows_b, rank_a, dtype=torch.float64, device=dev)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            hip.gemm_tn_f64(rows_b, rank_a, d, fb.data_ptr(), rows, fa.data_ptr(), rows, m.data_ptr(), rank_a)
            desc, ws, sweeps_m = _jacobi(m, rows_b, rank_a, d, count)
            hip.jacobi_norm_sum(desc, m.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel())
            block = (desc.rows, desc.len)
        hip.frechet_mean_term(d, a.mean().data_ptr(), b.mean().data_ptr(), out[2:].data_ptr())
    sqrt_trace, _, mean_term, _ = out.tolist()
    trace_a, trace_b = float(a.trace().item()), float(b.trace().item())
    return FrechetResult(distance=((mean_term + trace_a) + trace_b) - 2.0 * sqrt_trace, mean_term=mean_term, trace_a=trace_a,
                         trace_b=trace_b, sqrt_trace=sqrt_trace, rank_a=rank_a, rank_b=rank_b, sweeps=(0, 0, sweeps_m), block=block)
