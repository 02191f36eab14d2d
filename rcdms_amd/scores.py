"""Figures from classifier logits on the HIP path: Char-F1 / Frm-Acc and the Inception Score.

Story-visualisation papers (StoryGAN, DUCO, StoryDALL-E, ARLDM, and RCDMs' own table) print FID, Char-F1 and Frm-Acc: a
fine-tuned Inception-v3 character classifier looks at every generated frame, and its multi-label predictions are scored
against the frame's character labels.  The usual route downloads the logits and calls scikit-learn.  Here the logits stay on
the device (InceptionV3Features(...)(frames, return_logits=True) produces them; num_classes is the classifier's 7 or 9):

  LabelCounts       the integer sufficient statistics of every multi-label figure — n, per-class tp / fp / fn and the histogram
                    H[t][e] of rows by (true positives, false positives + false negatives) — added to by one call per batch
                    (rcdm_label_counts: two launches, no read-back, no atomics).  Integer sums are exact and order-free, so
                    states merge by addition and batches may arrive in any order.  result() is the one read-back; every
                    averaging rule (label_scores) is then a division on the host in float64: frame accuracy (the subset
                    accuracy, Frm-Acc), F1 micro / macro / weighted / samples (Char-F1 is one of them, which one differs
                    between papers), Hamming loss and the per-class figures, as scikit-learn defines them.
  inception_score   exp of the mean KL(p_row || p_mean) over `splits` consecutive stretches of the rows (Salimans et al. 2016),
                    from stored logits: (N, C) device tensor or a FeatureBank of width C.  Three launches, float64 throughout,
                    fixed summation orders (csrc/scores_core.h), one read-back of `splits` doubles.

Prediction rule: logit > threshold, strictly, in float32; default threshold 0.0.  Deviation: the lineage's
round(sigmoid(x)) in float32 gives 0 for 0 < x <~ 6e-8 (sigmoid rounds to 0.5, which rounds to even), where this rule gives 1.

Parity: restated from the definitions, unpinned against torch-fidelity / torchmetrics (neither is a dependency); the label
figures are held against scikit-learn (tests/test_scores_host.py).  No classifier weights ship with the project.

No CPU path: a host tensor raises."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from .frechet import _device
from .kid import FeatureBank

MAX_LABEL_CLASSES = hip.SCORES_MAX_LABEL_CLASSES
MIN_CLASSES, MAX_CLASSES, MAX_SPLITS = hip.SCORES_MIN_CLASSES, hip.SCORES_MAX_CLASSES, hip.SCORES_MAX_SPLITS


def label_state_len(num_classes):
    """Length of the int64 state of `num_classes` classes: n, 3 per class, (C + 1)^2 histogram bins."""
    c = int(num_classes)
    if not 1 <= c <= MAX_LABEL_CLASSES:
        raise ValueError(f"num_classes is 1..{MAX_LABEL_CLASSES}, got {num_classes}")
    return 1 + 3 * c + (c + 1) * (c + 1)


@dataclass
class LabelScores:
    n: int
    num_classes: int
    frame_accuracy: float      # rows with every class right / n: sklearn's accuracy_score on multi-label rows, the papers' Frm-Acc
    f1_micro: float
    f1_macro: float
    f1_weighted: float         # by support
    f1_samples: float          # the mean over rows of 2 t / (2 t + e)
    hamming: float             # (fp + fn) / (n C)
    precision: np.ndarray      # per class, float64
    recall: np.ndarray
    f1: np.ndarray
    support: np.ndarray        # per class: tp + fn, int64
    tp: np.ndarray             # the raw integers
    fp: np.ndarray
    fn: np.ndarray
    hist: np.ndarray           # (C + 1, C + 1): rows by (true positives, false positives + false negatives)


def _div(num, den, zero_division):
    return float(zero_division) if den == 0 else num / den


def label_scores(state, num_classes, zero_division=0):
    """The figures of an int64 state (host array) -> LabelScores.  Python-int numerators and denominators, one float64 division
    each, sums of quotients with math.fsum: every figure is within one rounding of its exact value per operation."""
    c = int(num_classes)
    if zero_division not in (0, 1):
        raise ValueError(f"zero_division is 0 or 1, got {zero_division!r}")
    s = np.asarray(state)
    if s.dtype != np.int64 or s.shape != (label_state_len(c),):
        raise ValueError(f"a state of {c} classes is int64[{label_state_len(c)}], got {s.dtype} {s.shape}")
    v = [int(x) for x in s]
    n = v[0]
    if n < 1:
        raise ValueError("no rows yet")
    tp, fp, fn = (v[1 + k:1 + 3 * c:3] for k in range(3))
    hist = [v[1 + 3 * c + t * (c + 1):1 + 3 * c + (t + 1) * (c + 1)] for t in range(c + 1)]
    z = zero_division
    prec = [_div(tp[k], tp[k] + fp[k], z) for k in range(c)]
    rec = [_div(tp[k], tp[k] + fn[k], z) for k in range(c)]
    f1 = [_div(2 * tp[k], 2 * tp[k] + fp[k] + fn[k], z) for k in range(c)]
    support = [tp[k] + fn[k] for k in range(c)]
    stp, sfp, sfn, ssup = sum(tp), sum(fp), sum(fn), sum(support)
    samples = math.fsum(hist[t][e] * _div(2 * t, 2 * t + e, z) for t in range(c + 1) for e in range(c + 1) if hist[t][e])
    return LabelScores(
        n=n, num_classes=c,
        frame_accuracy=sum(hist[t][0] for t in range(c + 1)) / n,
        f1_micro=_div(2 * stp, 2 * stp + sfp + sfn, z),
        f1_macro=math.fsum(f1) / c,
        f1_weighted=float(z) if ssup == 0 else math.fsum(support[k] * f1[k] for k in range(c)) / ssup,
        f1_samples=samples / n,
        hamming=(sfp + sfn) / (n * c),
        precision=np.array(prec, np.float64), recall=np.array(rec, np.float64), f1=np.array(f1, np.float64),
        support=np.array(support, np.int64), tp=np.array(tp, np.int64), fp=np.array(fp, np.int64), fn=np.array(fn, np.int64),
        hist=np.array(hist, np.int64).reshape(c + 1, c + 1))


class LabelCounts:
    """The running integer state of the multi-label figures of `num_classes` classes on one device."""

    def __init__(self, num_classes, device, thresholds=None):
        self.num_classes, self.device = int(num_classes), _device(device)
        self.len = label_state_len(self.num_classes)
        if thresholds is None:
            self.thresholds = None
        else:
            t = np.asarray(thresholds, np.float32).reshape(-1)
            if t.shape != (self.num_classes,) or np.isnan(t).any():
                raise ValueError(f"`thresholds` is {self.num_classes} numbers, got {np.shape(thresholds)}")
            self.thresholds = t
        self._state = None         # int64[len] on the device, allocated with the first rows
        self._thr = None           # the thresholds on the device

    def _alloc(self, device):
        if self.device.index is None:
            self.device = device
        if self._state is None:
            self._state = torch.zeros(self.len, dtype=torch.int64, device=self.device)
        if self._thr is None and self.thresholds is not None:
            self._thr = torch.from_numpy(self.thresholds).to(self.device)

    def update(self, logits, labels):
        """logits: (..., C) float32 or float16 on this device; labels: (..., C) uint8 or bool of the same leading shape (non-zero
        is 1).  Rows of either may be strided.  Adds the rows into the state; no read-back."""
        c = self.num_classes
        for t, name in ((logits, "logits"), (labels, "labels")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"`{name}` is a device tensor, got {type(t).__name__}")
            if not t.is_cuda:
                raise hip.RcdmError(f"label counts run on the HIP path only: `{name}` must be a device tensor")
        if logits.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"`logits` is float32 or float16, got {logits.dtype}")
        if labels.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"`labels` is uint8 or bool, got {labels.dtype}")
        if logits.dim() < 1 or logits.shape[-1] != c or logits.numel() == 0:
            raise ValueError(f"`logits` is (..., {c}) with at least one row, got {tuple(logits.shape)}")
        if labels.shape != logits.shape:
            raise ValueError(f"`labels` has the shape of `logits`, got {tuple(labels.shape)} against {tuple(logits.shape)}")
        if labels.device != logits.device or (self.device.index is not None and logits.device != self.device):
            raise ValueError(f"`logits` is on {logits.device}, `labels` on {labels.device}, the counts on {self.device}")
        self._alloc(logits.device)
        x = logits if logits.dim() == 2 else logits.reshape(-1, c)
        y = labels if labels.dim() == 2 else labels.reshape(-1, c)
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        x, y = (t if t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= c) else t.contiguous() for t in (x, y))
        n = x.shape[0]
        desc = hip.LabelDesc(x.stride(0) if n > 1 else c, y.stride(0) if n > 1 else c, n, c,
                             hip.FSTATS_F16 if x.dtype == torch.float16 else hip.FSTATS_F32, 0)
        need = hip.label_counts_workspace_bytes(desc)
        if need == 0:
            raise hip.RcdmError(f"rcdm_label_counts refused {n} rows of {c} classes")
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            hip.label_counts(desc, x.data_ptr(), y.data_ptr(), hip.ptr(self._thr), self._state.data_ptr(), ws.data_ptr(), need)
        return self

    def merge(self, other):
        """Adds another state of the same classes and thresholds (integer addition: exact)."""
        if not isinstance(other, LabelCounts) or other.num_classes != self.num_classes:
            raise ValueError("merge takes a LabelCounts of the same number of classes")
        a, b = self.thresholds, other.thresholds
        if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
            raise ValueError("the two states were counted under different thresholds")
        if other._state is not None:
            self._alloc(other._state.device)
            self._state += other._state.to(self.device)
        return self

    def state(self):
        """int64[1 + 3 C + (C + 1)^2] on the device (None before the first rows): [n | tp, fp, fn per class | H[t][e]]."""
        return self._state

    def clear(self):
        if self._state is not None:
            self._state.zero_()
        return self

    def save(self, path):
        """.npz with `label_state` (and `thresholds` when there are any)."""
        s = np.zeros(self.len, np.int64) if self._state is None else self._state.cpu().numpy()
        extra = {} if self.thresholds is None else {"thresholds": self.thresholds}
        np.savez(path, label_state=s, **extra)

    @classmethod
    def load(cls, path, device):
        with np.load(path) as z:
            s = z["label_state"]
            thr = z["thresholds"] if "thresholds" in z.files else None
        c = next((k for k in range(1, MAX_LABEL_CLASSES + 1) if label_state_len(k) == s.size), 0)
        if s.ndim != 1 or s.dtype != np.int64 or c == 0 or (s < 0).any():
            raise ValueError(f"`label_state` is int64[1 + 3 C + (C + 1)^2] of counts, got {s.dtype} {s.shape}")
        self = cls(c, device, thr)
        if self.device.index is not None:
            self._alloc(self.device)
            self._state.copy_(torch.from_numpy(s))
        else:
            raise hip.RcdmError("no device to load the state onto")
        return self

    def result(self, zero_division=0):
        """-> LabelScores.  The one read-back."""
        if zero_division not in (0, 1):
            raise ValueError(f"zero_division is 0 or 1, got {zero_division!r}")
        if self._state is None:
            raise ValueError("no rows yet")
        return label_scores(self._state.cpu().numpy(), self.num_classes, zero_division)


@dataclass
class IscResult:
    mean: float            # the mean of the splits' scores: the figure reported as the Inception Score
    std: float             # their population standard deviation (ddof = 0)
    scores: tuple          # exp(kl) of every split, in order
    kl: tuple              # mean over the split's rows of KL(p_row || p_mean), as the device formed it


def shuffled_order(n, seed):
    """This project's rule for shuffle_seed: numpy.random.RandomState(seed).permutation(n) (no other implementation's draws are
    reproduced), as int32."""
    return np.random.RandomState(seed).permutation(int(n)).astype(np.int32)


def inception_score(logits, splits=10, shuffle_seed=None, order=None, chunks_per_block=0):
    """logits: (N, C) float32 / float16 device tensor (rows may be strided) or a FeatureBank of width C = 2 .. 4096.  Split k is
    positions [k N // splits, (k + 1) N // splits) of the row order: the given one, `order` (N row indices, uploaded once), or
    shuffled_order(N, shuffle_seed).  chunks_per_block: a launch-geometry knob that changes no bit.  -> IscResult (host floats;
    the arithmetic up to KL ran on the device)."""
    x = logits
    if isinstance(x, FeatureBank):
        if len(x) < 1:
            raise ValueError("`logits` holds no rows yet")
        x = x.rows()
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"`logits` is a FeatureBank or a device tensor, got {type(x).__name__}")
    if x.dim() != 2:
        raise ValueError(f"`logits` is (N, C), got {tuple(x.shape)}")
    n, c = x.shape
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"`logits` is float32 or float16, got {x.dtype}")
    if not MIN_CLASSES <= c <= MAX_CLASSES:
        raise ValueError(f"C is {MIN_CLASSES}..{MAX_CLASSES}, got {c}")
    splits = int(splits)
    if not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"1..{MAX_SPLITS} splits, got {splits}")
    if n < splits:
        raise ValueError(f"{splits} splits need at least as many rows, got {n}")
    if n > hip.SCORES_MAX_N:
        raise ValueError(f"at most {hip.SCORES_MAX_N} rows, got {n}")
    if not 0 <= int(chunks_per_block) <= hip.SCORES_MAX_CHUNKS_PER_BLOCK:
        raise ValueError(f"chunks_per_block is 0..{hip.SCORES_MAX_CHUNKS_PER_BLOCK}, got {chunks_per_block}")
    if order is not None and shuffle_seed is not None:
        raise ValueError("give `order` or `shuffle_seed`, not both")
    if shuffle_seed is not None:
        order = shuffled_order(n, shuffle_seed)
    if order is not None:
        o = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order)
        if o.dtype.kind not in "iu" or o.shape != (n,):
            raise ValueError(f"`order` is {n} row indices, got {o.dtype} {o.shape}")
        if o.min() < 0 or o.max() >= n:
            raise ValueError(f"`order` indexes rows {int(o.min())}..{int(o.max())} of {n}")
        order = np.ascontiguousarray(o, np.int32)
    if not x.is_cuda:
        raise hip.RcdmError("the Inception Score runs on the HIP path only: `logits` must be a device tensor")
    if x.stride(1) != 1 or (n > 1 and x.stride(0) < c):
        x = x.contiguous()
    desc = hip.IscDesc(x.stride(0) if n > 1 else c, n, c, splits, hip.FSTATS_F16 if x.dtype == torch.float16 else hip.FSTATS_F32,
                       int(chunks_per_block), 0)
    need = hip.inception_score_workspace_bytes(desc)
    if need == 0:
        raise hip.RcdmError(f"rcdm_inception_score refused {n} rows of {c} classes in {splits} splits")
    dev = x.device
    idx = None if order is None else torch.from_numpy(order).to(dev)                 # the one upload
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(splits, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.inception_score(desc, x.data_ptr(), hip.ptr(idx), out.data_ptr(), 0, ws.data_ptr(), need)
    kl = tuple(out.tolist())                                                         # the one read-back
    scores = tuple(math.exp(v) for v in kl)
    total = 0.0
    for v in scores:
        total = total + v
    mean = total / splits
    sq = 0.0
    for v in scores:
        sq = sq + (v - mean) * (v - mean)
    return IscResult(mean=mean, std=math.sqrt(sq / splits), scores=scores, kl=kl)
