"""Inception-v3 pool features on the HIP path: uint8 frames -> the 2048-wide features FID / KID are defined on.

The network is torchvision.models.inception_v3 (variant "torchvision") or pytorch-fid's FID Inception (variant "fid": the
average pools of the A and C blocks and of Mixed_7b leave the padding out of their divisor, the pool of Mixed_7c is a max
pool), evaluated with the kernels of csrc/conv2d.hip:
  rcdm_image_bilinear_rows   frames -> 299 x 299 f16 rows in [-1, 1] (torch's bilinear, no antialias; 3 channels padded to 8)
  rcdm_conv2d                every conv, its inference BatchNorm (eps 1e-3) folded in on the host in fp32 —
                             W' = W g / sqrt(var + eps) rounded once to f16, b' = beta - mean g / sqrt(var + eps) in fp32 —
                             with the bias + ReLU epilogue; a branch writes its column window of the block's concat buffer
  rcdm_pool2d                the max and average pools (a pass-through pool writes its window of the concat buffer too)
  rcdm_global_avgpool        8 x 8 x 2048 -> (N, 2048) fp32;  rcdm_small_linear: the optional fc -> logits
The weights are the caller's: a state dict with torchvision's keys.  There is no concat copy and no CPU path; a launch plan
(buffers + descriptors, one stream, program order) is built once per chunk size N (the network runs at 299 x 299 whatever the frames' H x W: only the bilinear descriptor,
made per call, sees them — so every (N, H, W) finds its plan, and two frame sizes share one) and kept in a small LRU, and a large N runs in
chunks of `batch` frames.  Restated from the published architecture and tested against tests/inception_oracle.py.

Classifier input (preprocess="pillow"): the character classifiers of the StoryGAN -> DUCO -> StoryDALL-E -> ARLDM lineage are
torchvision Inception-v3 networks fed `Resize((299, 299))` on a PIL image — Pillow's antialiased 8-bit bilinear — then `ToTensor`
and `Normalize(mean, std)`.  That is rcdm_image_resample in RCDM_IMAGE_F16_ROWS mode (image.Resampler.to_rows: Pillow's bytes
bit for bit, then (u8 / 255 - mean) / std rounded to f16) writing the plan's input rows; the ImageNet constants are the default.
torchvision's `transform_input=True` is a per-channel affine map x' = x std / 0.5 + (mean - 0.5) / 0.5 of the normalised pixel:
it folds into the constants, and with the ImageNet mean / std the folded ones are mean = std = (0.5, 0.5, 0.5) exactly.  No
classifier weights ship with the project; the preprocessing is reproduced from the published transforms."""
from collections import OrderedDict

import torch

from . import hip
from .metrics import _frames, _view

EPS = 1e-3
SIDE = 299
VARIANTS = ("fid", "torchvision")
PREPROCESS = ("fid", "pillow")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TRANSFORM_INPUT_MEAN = TRANSFORM_INPUT_STD = (0.5, 0.5, 0.5)      # ImageNet constants with transform_input=True folded in


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _layers():
    """name -> (c_in, c_out, (kh, kw), (sh, sw), (ph, pw)) of every conv on the feature path."""
    L = OrderedDict()

    def add(name, cin, cout, k, s=1, p=0):
        L[name] = (cin, cout, _pair(k), _pair(s), _pair(p))
    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80, 1)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for b, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        add(f"{b}.branch1x1", cin, 64, 1)
        add(f"{b}.branch5x5_1", cin, 48, 1)
        add(f"{b}.branch5x5_2", 48, 64, 5, 1, 2)
        add(f"{b}.branch3x3dbl_1", cin, 64, 1)
        add(f"{b}.branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(f"{b}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(f"{b}.branch_pool", cin, pf, 1)
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for b, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(f"{b}.branch1x1", 768, 192, 1)
        add(f"{b}.branch7x7_1", 768, c7, 1)
        add(f"{b}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(f"{b}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(f"{b}.branch7x7dbl_1", 768, c7, 1)
        add(f"{b}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(f"{b}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(f"{b}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(f"{b}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(f"{b}.branch_pool", 768, 192, 1)
    add("Mixed_7a.branch3x3_1", 768, 192, 1)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for b, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(f"{b}.branch1x1", cin, 320, 1)
        add(f"{b}.branch3x3_1", cin, 384, 1)
        add(f"{b}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{b}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{b}.branch3x3dbl_1", cin, 448, 1)
        add(f"{b}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(f"{b}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(f"{b}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(f"{b}.branch_pool", cin, 192, 1)
    return L


LAYERS = _layers()
BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
          "Mixed_7c")
BLOCK_IN = {"Mixed_5b": 192, "Mixed_5c": 256, "Mixed_5d": 288, "Mixed_6a": 288, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
            "Mixed_6e": 768, "Mixed_7a": 768, "Mixed_7b": 1280, "Mixed_7c": 2048}


def expected_keys(blocks=None, fc=True):
    """Every state-dict key the extractor reads -> its shape (num_classes left open: fc.weight is (num_classes, 2048))."""
    out = OrderedDict()
    for name, (cin, cout, (kh, kw), _, _) in LAYERS.items():
        if blocks is not None and name.split(".")[0] not in blocks:
            continue
        out[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.bn.{k}"] = (cout,)
    if fc:
        out["fc.weight"] = (None, 2048)
        out["fc.bias"] = (None,)
    return out


def check_state_dict(sd, blocks=None, fc=True):
    """ValueError for a missing or mis-shaped key; keys the feature path does not read (AuxLogits.*, *.num_batches_tracked)
    are accepted and ignored.  -> num_classes (None without fc)."""
    want = expected_keys(blocks, fc)
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError(f"state dict lacks {len(missing)} keys of the Inception-v3 feature path, first: {missing[:4]}")
    num_classes = None
    if fc:
        fw = tuple(sd["fc.weight"].shape)
        if len(fw) != 2 or fw[1] != 2048 or fw[0] < 1:
            raise ValueError(f"fc.weight is (num_classes, 2048), got {fw}")
        num_classes = fw[0]
    for k, shape in want.items():
        shape = tuple(num_classes if v is None else v for v in shape)
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{k} is {shape}, got {tuple(sd[k].shape)}")
    return num_classes


def fold_conv(sd, name):
    """-> (f16 [c_out][kh * kw * c_in_padded] in rcdm_conv2d's order, fp32 bias [c_out]); c_in padded to a multiple of 8."""
    w = sd[f"{name}.conv.weight"].detach().to("cpu", torch.float32)
    g = sd[f"{name}.bn.weight"].detach().to("cpu", torch.float32)
    var = sd[f"{name}.bn.running_var"].detach().to("cpu", torch.float32)
    mean = sd[f"{name}.bn.running_mean"].detach().to("cpu", torch.float32)
    beta = sd[f"{name}.bn.bias"].detach().to("cpu", torch.float32)
    s = g / torch.sqrt(var + EPS)
    w = (w * s[:, None, None, None]).permute(0, 2, 3, 1)            # (c_out, kh, kw, c_in)
    cin = w.shape[-1]
    pad = (-cin) % 8
    if pad:
        w = torch.nn.functional.pad(w, (0, pad))
    return w.reshape(w.shape[0], -1).to(torch.float16).contiguous(), (beta - mean * s).contiguous()


class _Act:
    """An activation: n * h * w rows of c channels at column `off` of the row buffer t."""

    def __init__(self, t, off, c, h, w):
        self.t, self.off, self.c, self.h, self.w = t, off, c, h, w

    @property
    def ptr(self):
        return self.t.data_ptr() + 2 * self.off

    @property
    def ld(self):
        return self.t.shape[1]

    def window(self, off, c):
        return _Act(self.t, self.off + off, c, self.h, self.w)

    def rows(self):
        return self.t[:, self.off:self.off + self.c]


def _out_side(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class _Plan:
    """The launches of one forward at a fixed (n, input side): buffers, descriptors, pointers, in program order."""

    def __init__(self, net, n):
        self.net, self.n = net, n
        self.ops, self.bufs = [], []

    def buf(self, h, w, c):
        t = torch.empty(self.n * h * w, c, dtype=torch.float16, device=self.net.device)
        self.bufs.append(t)
        return _Act(t, 0, c, h, w)

    def conv(self, name, a, out=None):
        cin, cout, (kh, kw), (sh, sw), (ph, pw) = LAYERS[name]
        W, b = self.net.weights[name]
        cin = W.shape[1] // (kh * kw)                  # the padded width of the stem's first conv
        assert a.c == cin, (name, a.c, cin)
        ho, wo = _out_side(a.h, kh, sh, ph), _out_side(a.w, kw, sw, pw)
        if out is None:
            out = self.buf(ho, wo, cout)
        assert (out.h, out.w, out.c) == (ho, wo, cout), (name, out.h, out.w, out.c, ho, wo, cout)
        d = hip.Conv2dDesc(self.n, a.h, a.w, cin, cout, kh, kw, sh, sw, ph, pw, a.ld, out.ld, hip.EPI_BIAS | hip.EPI_RELU)
        self.ops.append((hip.conv2d, (d, a.ptr, W.data_ptr(), b.data_ptr(), out.ptr)))
        return out

    def pool(self, a, k, s, p, mode, out=None):
        ho, wo = _out_side(a.h, k, s, p), _out_side(a.w, k, s, p)
        if out is None:
            out = self.buf(ho, wo, a.c)
        assert (out.h, out.w, out.c) == (ho, wo, a.c)
        d = hip.Pool2dDesc(self.n, a.h, a.w, a.c, k, k, s, s, p, p, a.ld, out.ld, mode)
        self.ops.append((hip.pool2d, (d, a.ptr, out.ptr)))
        return out

    def run(self):
        for fn, args in self.ops:
            fn(*args)

    # ---- the blocks: every branch ends in its column window of `cat` ----
    def block_a(self, p, x):
        pf = LAYERS[f"{p}.branch_pool"][1]
        cat = self.buf(x.h, x.w, 224 + pf)
        self.conv(f"{p}.branch1x1", x, cat.window(0, 64))
        self.conv(f"{p}.branch5x5_2", self.conv(f"{p}.branch5x5_1", x), cat.window(64, 64))
        t = self.conv(f"{p}.branch3x3dbl_2", self.conv(f"{p}.branch3x3dbl_1", x))
        self.conv(f"{p}.branch3x3dbl_3", t, cat.window(128, 96))
        self.conv(f"{p}.branch_pool", self.pool(x, 3, 1, 1, self.net.avg_mode(p)), cat.window(224, pf))
        return cat

    def block_b(self, p, x):
        ho, wo = _out_side(x.h, 3, 2, 0), _out_side(x.w, 3, 2, 0)
        cat = self.buf(ho, wo, 384 + 96 + x.c)
        self.conv(f"{p}.branch3x3", x, cat.window(0, 384))
        t = self.conv(f"{p}.branch3x3dbl_2", self.conv(f"{p}.branch3x3dbl_1", x))
        self.conv(f"{p}.branch3x3dbl_3", t, cat.window(384, 96))
        self.pool(x, 3, 2, 0, hip.POOL_MAX, cat.window(480, x.c))
        return cat

    def block_c(self, p, x):
        cat = self.buf(x.h, x.w, 768)
        self.conv(f"{p}.branch1x1", x, cat.window(0, 192))
        t = self.conv(f"{p}.branch7x7_2", self.conv(f"{p}.branch7x7_1", x))
        self.conv(f"{p}.branch7x7_3", t, cat.window(192, 192))
        t = self.conv(f"{p}.branch7x7dbl_1", x)
        for i in (2, 3, 4):
            t = self.conv(f"{p}.branch7x7dbl_{i}", t)
        self.conv(f"{p}.branch7x7dbl_5", t, cat.window(384, 192))
        self.conv(f"{p}.branch_pool", self.pool(x, 3, 1, 1, self.net.avg_mode(p)), cat.window(576, 192))
        return cat

    def block_d(self, p, x):
        ho, wo = _out_side(x.h, 3, 2, 0), _out_side(x.w, 3, 2, 0)
        cat = self.buf(ho, wo, 320 + 192 + x.c)
        self.conv(f"{p}.branch3x3_2", self.conv(f"{p}.branch3x3_1", x), cat.window(0, 320))
        t = self.conv(f"{p}.branch7x7x3_1", x)
        for i in (2, 3):
            t = self.conv(f"{p}.branch7x7x3_{i}", t)
        self.conv(f"{p}.branch7x7x3_4", t, cat.window(320, 192))
        self.pool(x, 3, 2, 0, hip.POOL_MAX, cat.window(512, x.c))
        return cat

    def block_e(self, p, x):
        cat = self.buf(x.h, x.w, 2048)
        self.conv(f"{p}.branch1x1", x, cat.window(0, 320))
        t = self.conv(f"{p}.branch3x3_1", x)
        self.conv(f"{p}.branch3x3_2a", t, cat.window(320, 384))
        self.conv(f"{p}.branch3x3_2b", t, cat.window(704, 384))
        t = self.conv(f"{p}.branch3x3dbl_2", self.conv(f"{p}.branch3x3dbl_1", x))
        self.conv(f"{p}.branch3x3dbl_3a", t, cat.window(1088, 384))
        self.conv(f"{p}.branch3x3dbl_3b", t, cat.window(1472, 384))
        self.conv(f"{p}.branch_pool", self.pool(x, 3, 1, 1, self.net.avg_mode(p)), cat.window(1856, 192))
        return cat

    def block(self, p, x):
        tag = p.split("_")[1]
        fn = {"5": self.block_a, "6a": self.block_b, "6": self.block_c, "7a": self.block_d, "7": self.block_e}
        return fn[tag if tag in fn else tag[0]](p, x)


class InceptionV3Features:
    """state_dict: torchvision's Inception3 keys (`<Block>.<branch>.conv.weight`, `.bn.{weight,bias,running_mean,running_var}`,
    `fc.weight`, `fc.bias`; AuxLogits.* and num_batches_tracked ignored); num_classes is fc.weight's row count.
    variant: "fid" (pytorch-fid's FID Inception) or "torchvision".  batch: frames per chunk of a large call.
    blocks: only for tests — build just these Mixed_* blocks (run_block), no stem, no fc.
    preprocess: "fid" (torch's bilinear without antialias to 299 x 299, 2 x - 1: the FID input) or "pillow" (Pillow's 8-bit
    bilinear to 299 x 299, then (u8 / 255 - mean) / std: a torchvision classifier's input; mean, std default to ImageNet's)."""

    def __init__(self, state_dict, variant="fid", device="cuda", batch=50, plans=4, blocks=None, *, preprocess="fid", mean=None,
                 std=None):
        if variant not in VARIANTS:
            raise ValueError(f"variant {variant!r}: one of {VARIANTS}")
        if preprocess not in PREPROCESS:
            raise ValueError(f"preprocess {preprocess!r}: one of {PREPROCESS}")
        if preprocess == "fid" and (mean is not None or std is not None):
            raise ValueError("mean and std belong to preprocess='pillow': the FID input is 2 x - 1")
        self.preprocess = preprocess
        self.mean = tuple(float(v) for v in (IMAGENET_MEAN if mean is None else mean))
        self.std = tuple(float(v) for v in (IMAGENET_STD if std is None else std))
        if len(self.mean) != 3 or len(self.std) != 3 or not all(v > 0.0 for v in self.std) or any(v != v for v in self.mean):
            raise ValueError(f"mean and std are three numbers each, std above 0, got {mean} and {std}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip.RcdmError("InceptionV3Features runs on the HIP path only: there is no CPU path here")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if int(batch) < 1 or int(plans) < 1:
            raise ValueError("batch and plans are at least 1")
        self.variant, self.batch, self.max_plans = variant, int(batch), int(plans)
        self.num_classes = check_state_dict(state_dict, blocks, fc=blocks is None)
        hip.load()
        self.weights = {}
        for name in LAYERS:
            if blocks is not None and name.split(".")[0] not in blocks:
                continue
            W, b = fold_conv(state_dict, name)
            self.weights[name] = (W.to(self.device), b.to(self.device))
        if blocks is None:
            self.fc_w = state_dict["fc.weight"].detach().to("cpu", torch.float32).to(torch.float16).contiguous().to(self.device)
            self.fc_b = state_dict["fc.bias"].detach().to("cpu", torch.float32).contiguous().to(self.device)
        self._plans = OrderedDict()
        self.plans_built = 0

    def avg_mode(self, block):
        """The pool in front of `branch_pool` of an A, C or E block."""
        if self.variant == "torchvision":
            return hip.POOL_AVG_INCLUDE_PAD
        return hip.POOL_MAX if block == "Mixed_7c" else hip.POOL_AVG_EXCLUDE_PAD

    # ---- plans ----
    def _plan(self, key, build):
        plan = self._plans.get(key)
        if plan is None:
            plan = build()
            self.plans_built += 1
            self._plans[key] = plan
            while len(self._plans) > self.max_plans:
                self._plans.popitem(last=False)
        else:
            self._plans.move_to_end(key)
        return plan

    def _build_net(self, n):
        p = _Plan(self, n)
        p.x0 = p.buf(SIDE, SIDE, 8)
        x = p.conv("Conv2d_1a_3x3", p.x0)
        x = p.conv("Conv2d_2a_3x3", x)
        x = p.conv("Conv2d_2b_3x3", x)
        x = p.pool(x, 3, 2, 0, hip.POOL_MAX)
        x = p.conv("Conv2d_3b_1x1", x)
        x = p.conv("Conv2d_4a_3x3", x)
        x = p.pool(x, 3, 2, 0, hip.POOL_MAX)
        for b in BLOCKS:
            x = p.block(b, x)
        assert (x.h, x.w, x.c) == (8, 8, 2048)
        p.last = x
        return p

    def _input_rows(self, frames, dst_ptr):
        """frames (n, H, W, 3) uint8 view -> n * 299 * 299 f16 rows of 8 channels at dst_ptr: one launch."""
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        if self.preprocess == "pillow":
            from . import image
            image.resampler(H, W, SIDE, SIDE, "bilinear", None, self.device).to_rows(frames, self.mean, self.std, dst_ptr, 8, 8)
            return
        pitch = frames.stride(1) if H > 1 else 3 * W
        stride = frames.stride(0) if n > 1 else 0
        d = hip.BilinearDesc(pitch, stride, n, 3, H, W, SIDE, SIDE, 0, 8, 8, (2.0, 2.0, 2.0), (-1.0, -1.0, -1.0))
        hip.image_bilinear_rows(d, frames.data_ptr(), dst_ptr)

    def _checked(self, frames):
        frames = _frames("frames", frames)
        if not frames.is_cuda:
            raise hip.RcdmError("InceptionV3Features runs on the HIP path only: frames must be a device tensor (there is no CPU path here)")
        if frames.device != self.device:
            raise ValueError(f"frames are on {frames.device}, the extractor on {self.device}")
        return _view(frames)

    @torch.no_grad()
    def preprocessed_rows(self, frames):
        """The network's input for these frames, as `preprocess` makes it: f16 (N, 299, 299, 8), channels 3 .. 7 zero.  A buffer
        of its own (no plan is built or touched); for tests and for comparing against a classifier's own transforms."""
        v = self._checked(frames)
        rows = torch.empty(v.shape[0] * SIDE * SIDE, 8, dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            for i in range(0, v.shape[0], self.batch):
                self._input_rows(v[i:i + self.batch], rows[i * SIDE * SIDE:].data_ptr())
        return rows.view(v.shape[0], SIDE, SIDE, 8)

    def _forward_chunk(self, frames, feats, logits):
        """frames (n, H, W, 3) uint8 view (any pitch, one stride), n <= batch; feats fp32 (n, 2048), logits fp32 (n, classes) or None."""
        n = frames.shape[0]
        plan = self._plan(("net", n), lambda: self._build_net(n))
        self._input_rows(frames, plan.x0.ptr)
        plan.run()
        last = plan.last
        hip.global_avgpool(n, last.h * last.w, last.c, last.ptr, last.ld, feats.data_ptr(), feats.stride(0))
        if logits is not None:
            for r in range(0, n, 8):          # rcdm_small_linear takes at most 8 rows
                m = min(8, n - r)
                hip.small_linear(feats[r:].data_ptr(), m, 2048, self.fc_w.data_ptr(), self.fc_b.data_ptr(), self.num_classes, 0, 0,
                                 logits[r:].data_ptr())

    @torch.no_grad()
    def __call__(self, frames, return_logits=False):
        """frames: device uint8 (..., H, W, 3) of one size, RGB; slices and strips are read by their pitch, without a copy.
        -> fp32 (N, 2048) on the device, N the product of the leading axes; with return_logits (features, (N, num_classes))."""
        frames = _frames("frames", frames)
        if not frames.is_cuda:
            raise hip.RcdmError("InceptionV3Features runs on the HIP path only: frames must be a device tensor (there is no CPU path here)")
        if frames.device != self.device:
            raise ValueError(f"frames are on {frames.device}, the extractor on {self.device}")
        if not hasattr(self, "fc_w"):
            raise ValueError("this extractor holds single blocks only (blocks=...): use run_block")
        v = _view(frames)
        N = v.shape[0]
        feats = torch.empty(N, 2048, dtype=torch.float32, device=self.device)
        logits = torch.empty(N, self.num_classes, dtype=torch.float32, device=self.device) if return_logits else None
        with torch.cuda.device(self.device):
            for i in range(0, N, self.batch):
                j = min(N, i + self.batch)
                self._forward_chunk(v[i:j], feats[i:j], None if logits is None else logits[i:j])
        return (feats, logits) if return_logits else feats

    @torch.no_grad()
    def run_block(self, block, x):
        """One Mixed_* block on f16 device rows: x (n, h, w, c_in) -> (n, h_out, w_out, c_out) f16, a view of the plan's concat
        buffer (valid until the next call of this shape).  What the block tests drive."""
        if block not in BLOCKS:
            raise ValueError(f"block {block!r}: one of {BLOCKS}")
        if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 4 or x.shape[-1] != BLOCK_IN[block]:
            raise ValueError(f"{block} takes device f16 (n, h, w, {BLOCK_IN[block]}), got {x.dtype} {tuple(x.shape)}")
        n, h, w, c = x.shape

        def build():
            p = _Plan(self, n)
            p.x0 = p.buf(h, w, c)
            p.last = p.block(block, p.x0)
            return p
        with torch.cuda.device(self.device):
            plan = self._plan((block, n, h, w), build)
            plan.x0.t.copy_(x.reshape(n * h * w, c))
            plan.run()
        o = plan.last
        return o.t.view(n, o.h, o.w, o.c)
