"""Inception-v3 pool features restated on the CPU with torch.nn.functional: what rcdms_amd/inception.py is tested against.

  network      torchvision.models.inception_v3 (transform_input=False, eval) through avgpool (2048) and fc, and pytorch-fid's FID
               variant of it (the average pools of the A and C blocks and of Mixed_7b exclude the padding from their divisor, the
               pool of Mixed_7c is a max pool).  Written from the published architecture; torchvision is compared against only
               where it imports (tests/test_inception_host.py), so the status is "restated, unpinned".
  features()   the network in fp32 or float64 on the unfolded state dict: conv, BatchNorm (eps 1e-3, running statistics), ReLU.
  f16 model    features(..., f16=True): the BatchNorm folded into the conv in fp32 (W' = W g / sqrt(var + eps),
               b' = beta - mean g / sqrt(var + eps)), W' rounded once to f16, every layer input and output rounded to f16,
               products and sums in fp32, the global mean in the kernel's order.  The arithmetic the kernels are allowed.
  resize()     torch's bilinear (align_corners=False, no antialias) written out on x / 255, then * scale + shift.
  ordered_mean the kernel's global average: one fp32 accumulator, rows in ascending order, one division.
  synthetic_state_dict  seeded full-width weights: He-scaled convs times GAIN, gamma and variance in [0.5, 1.5], beta and mean
               in [-0.1, 0.1].  GAIN = 1.0 keeps the activations O(1) to the last block: on two random 48 x 64 frames the RMS of
               every block's output stays between 0.2 and 6 in both variants (checked on the CPU by
               tests/test_inception_host.py::test_synthetic_activations_stay_order_one)."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-3
GAIN = 1.0
BLOCKS = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "maxpool1", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "maxpool2",
          "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
          "Mixed_7b", "Mixed_7c")
BLOCK_CHANNELS = {"Conv2d_1a_3x3": 32, "Conv2d_2a_3x3": 32, "Conv2d_2b_3x3": 64, "maxpool1": 64, "Conv2d_3b_1x1": 80,
                  "Conv2d_4a_3x3": 192, "maxpool2": 192, "Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768,
                  "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768, "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048,
                  "Mixed_7c": 2048}
BLOCK_SIDES = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "maxpool1": 73, "Conv2d_3b_1x1": 73,
               "Conv2d_4a_3x3": 71, "maxpool2": 35, "Mixed_5b": 35, "Mixed_5c": 35, "Mixed_5d": 35, "Mixed_6a": 17,
               "Mixed_6b": 17, "Mixed_6c": 17, "Mixed_6d": 17, "Mixed_6e": 17, "Mixed_7a": 8, "Mixed_7b": 8, "Mixed_7c": 8}


def conv_shapes():
    """name -> (c_out, c_in, kh, kw) of every BasicConv2d on the feature path, in forward order."""
    s = {}
    s["Conv2d_1a_3x3"] = (32, 3, 3, 3)
    s["Conv2d_2a_3x3"] = (32, 32, 3, 3)
    s["Conv2d_2b_3x3"] = (64, 32, 3, 3)
    s["Conv2d_3b_1x1"] = (80, 64, 1, 1)
    s["Conv2d_4a_3x3"] = (192, 80, 3, 3)
    for b, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        s[f"{b}.branch1x1"] = (64, cin, 1, 1)
        s[f"{b}.branch5x5_1"] = (48, cin, 1, 1)
        s[f"{b}.branch5x5_2"] = (64, 48, 5, 5)
        s[f"{b}.branch3x3dbl_1"] = (64, cin, 1, 1)
        s[f"{b}.branch3x3dbl_2"] = (96, 64, 3, 3)
        s[f"{b}.branch3x3dbl_3"] = (96, 96, 3, 3)
        s[f"{b}.branch_pool"] = (pf, cin, 1, 1)
    s["Mixed_6a.branch3x3"] = (384, 288, 3, 3)
    s["Mixed_6a.branch3x3dbl_1"] = (64, 288, 1, 1)
    s["Mixed_6a.branch3x3dbl_2"] = (96, 64, 3, 3)
    s["Mixed_6a.branch3x3dbl_3"] = (96, 96, 3, 3)
    for b, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        s[f"{b}.branch1x1"] = (192, 768, 1, 1)
        s[f"{b}.branch7x7_1"] = (c7, 768, 1, 1)
        s[f"{b}.branch7x7_2"] = (c7, c7, 1, 7)
        s[f"{b}.branch7x7_3"] = (192, c7, 7, 1)
        s[f"{b}.branch7x7dbl_1"] = (c7, 768, 1, 1)
        s[f"{b}.branch7x7dbl_2"] = (c7, c7, 7, 1)
        s[f"{b}.branch7x7dbl_3"] = (c7, c7, 1, 7)
        s[f"{b}.branch7x7dbl_4"] = (c7, c7, 7, 1)
        s[f"{b}.branch7x7dbl_5"] = (192, c7, 1, 7)
        s[f"{b}.branch_pool"] = (192, 768, 1, 1)
    s["Mixed_7a.branch3x3_1"] = (192, 768, 1, 1)
    s["Mixed_7a.branch3x3_2"] = (320, 192, 3, 3)
    s["Mixed_7a.branch7x7x3_1"] = (192, 768, 1, 1)
    s["Mixed_7a.branch7x7x3_2"] = (192, 192, 1, 7)
    s["Mixed_7a.branch7x7x3_3"] = (192, 192, 7, 1)
    s["Mixed_7a.branch7x7x3_4"] = (192, 192, 3, 3)
    for b, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        s[f"{b}.branch1x1"] = (320, cin, 1, 1)
        s[f"{b}.branch3x3_1"] = (384, cin, 1, 1)
        s[f"{b}.branch3x3_2a"] = (384, 384, 1, 3)
        s[f"{b}.branch3x3_2b"] = (384, 384, 3, 1)
        s[f"{b}.branch3x3dbl_1"] = (448, cin, 1, 1)
        s[f"{b}.branch3x3dbl_2"] = (384, 448, 3, 3)
        s[f"{b}.branch3x3dbl_3a"] = (384, 384, 1, 3)
        s[f"{b}.branch3x3dbl_3b"] = (384, 384, 3, 1)
        s[f"{b}.branch_pool"] = (192, cin, 1, 1)
    return s


def state_dict_shapes(num_classes=1000):
    """Every key the extractor reads -> shape (torchvision's names)."""
    out = {}
    for name, (co, ci, kh, kw) in conv_shapes().items():
        out[f"{name}.conv.weight"] = (co, ci, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.bn.{k}"] = (co,)
    out["fc.weight"] = (num_classes, 2048)
    out["fc.bias"] = (num_classes,)
    return out


def synthetic_state_dict(seed=0, num_classes=1000, only=None):
    """Seeded full-width weights (module docstring).  only: a block prefix ("Mixed_5b") to build just that block's keys."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (co, ci, kh, kw) in conv_shapes().items():
        # every layer draws, kept or not, so a block's weights do not depend on `only`
        w = torch.randn(co, ci, kh, kw, generator=g) * (GAIN * math.sqrt(2.0 / (ci * kh * kw)))
        gamma = 0.5 + torch.rand(co, generator=g)
        var = 0.5 + torch.rand(co, generator=g)
        beta = (torch.rand(co, generator=g) - 0.5) * 0.2
        mean = (torch.rand(co, generator=g) - 0.5) * 0.2
        if only is not None and not name.startswith(only + "."):
            continue
        sd[f"{name}.conv.weight"] = w
        sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"] = gamma, beta
        sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"] = mean, var
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    if only is None:
        sd["fc.weight"] = torch.randn(num_classes, 2048, generator=g) / math.sqrt(2048.0)
        sd["fc.bias"] = (torch.rand(num_classes, generator=g) - 0.5) * 0.2
    return sd


def fold_bn(sd, name):
    """(W' fp32 (c_out, c_in, kh, kw), b' fp32): the inference BatchNorm folded into the conv, in fp32."""
    w = sd[f"{name}.conv.weight"].float()
    s = sd[f"{name}.bn.weight"].float() / torch.sqrt(sd[f"{name}.bn.running_var"].float() + EPS)
    return w * s[:, None, None, None], sd[f"{name}.bn.bias"].float() - sd[f"{name}.bn.running_mean"].float() * s


def rt16(t):
    return t.to(torch.float16).to(t.dtype)


class Net:
    """One evaluation mode of the network: dtype fp32 / float64 with the unfolded BatchNorm, or the f16 model."""

    def __init__(self, sd, variant="fid", dtype=torch.float32, f16=False):
        assert variant in ("fid", "torchvision")
        self.sd, self.variant, self.f16 = sd, variant, f16
        self.dtype = torch.float32 if f16 else dtype

    def q(self, x):
        return rt16(x) if self.f16 else x

    def conv(self, name, x, stride=1, padding=0):
        sd = self.sd
        if self.f16:
            w, b = fold_bn(sd, name)
            y = F.conv2d(x, rt16(w), b, stride=stride, padding=padding)
            return rt16(F.relu(y))
        dt = self.dtype
        y = F.conv2d(x, sd[f"{name}.conv.weight"].to(dt), None, stride=stride, padding=padding)
        m, v = sd[f"{name}.bn.running_mean"].to(dt), sd[f"{name}.bn.running_var"].to(dt)
        g, b = sd[f"{name}.bn.weight"].to(dt), sd[f"{name}.bn.bias"].to(dt)
        y = (y - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS) * g[None, :, None, None] + b[None, :, None, None]
        return F.relu(y)

    def avg(self, x, fid_excludes):
        include = not (self.variant == "fid" and fid_excludes)
        return self.q(F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=include))

    def block_a(self, p, x):
        b1 = self.conv(f"{p}.branch1x1", x)
        b5 = self.conv(f"{p}.branch5x5_2", self.conv(f"{p}.branch5x5_1", x), padding=2)
        b3 = self.conv(f"{p}.branch3x3dbl_1", x)
        b3 = self.conv(f"{p}.branch3x3dbl_3", self.conv(f"{p}.branch3x3dbl_2", b3, padding=1), padding=1)
        bp = self.conv(f"{p}.branch_pool", self.avg(x, True))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, p, x):
        b3 = self.conv(f"{p}.branch3x3", x, stride=2)
        bd = self.conv(f"{p}.branch3x3dbl_2", self.conv(f"{p}.branch3x3dbl_1", x), padding=1)
        bd = self.conv(f"{p}.branch3x3dbl_3", bd, stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, stride=2)], 1)

    def block_c(self, p, x):
        b1 = self.conv(f"{p}.branch1x1", x)
        b7 = self.conv(f"{p}.branch7x7_1", x)
        b7 = self.conv(f"{p}.branch7x7_2", b7, padding=(0, 3))
        b7 = self.conv(f"{p}.branch7x7_3", b7, padding=(3, 0))
        bd = self.conv(f"{p}.branch7x7dbl_1", x)
        bd = self.conv(f"{p}.branch7x7dbl_2", bd, padding=(3, 0))
        bd = self.conv(f"{p}.branch7x7dbl_3", bd, padding=(0, 3))
        bd = self.conv(f"{p}.branch7x7dbl_4", bd, padding=(3, 0))
        bd = self.conv(f"{p}.branch7x7dbl_5", bd, padding=(0, 3))
        bp = self.conv(f"{p}.branch_pool", self.avg(x, True))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, p, x):
        b3 = self.conv(f"{p}.branch3x3_2", self.conv(f"{p}.branch3x3_1", x), stride=2)
        b7 = self.conv(f"{p}.branch7x7x3_1", x)
        b7 = self.conv(f"{p}.branch7x7x3_2", b7, padding=(0, 3))
        b7 = self.conv(f"{p}.branch7x7x3_3", b7, padding=(3, 0))
        b7 = self.conv(f"{p}.branch7x7x3_4", b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)

    def block_e(self, p, x, pool):
        """pool: "avg" (torchvision), "avg_exclude" (FID Mixed_7b) or "max" (FID Mixed_7c)."""
        b1 = self.conv(f"{p}.branch1x1", x)
        b3 = self.conv(f"{p}.branch3x3_1", x)
        b3 = torch.cat([self.conv(f"{p}.branch3x3_2a", b3, padding=(0, 1)), self.conv(f"{p}.branch3x3_2b", b3, padding=(1, 0))], 1)
        bd = self.conv(f"{p}.branch3x3dbl_2", self.conv(f"{p}.branch3x3dbl_1", x), padding=1)
        bd = torch.cat([self.conv(f"{p}.branch3x3dbl_3a", bd, padding=(0, 1)), self.conv(f"{p}.branch3x3dbl_3b", bd, padding=(1, 0))], 1)
        if pool == "max":
            pl = F.max_pool2d(x, 3, stride=1, padding=1)
        else:
            pl = self.q(F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=pool == "avg"))
        return torch.cat([b1, b3, bd, self.conv(f"{p}.branch_pool", pl)], 1)

    def e_pool(self, p):
        if self.variant == "torchvision":
            return "avg"
        return "avg_exclude" if p == "Mixed_7b" else "max"

    def block(self, p, x):
        """Any Mixed_* block by its name."""
        kind = {"5": self.block_a, "6a": self.block_b, "6": self.block_c, "7a": self.block_d}
        tag = p.split("_")[1]
        if tag in ("7b", "7c"):
            return self.block_e(p, x, self.e_pool(p))
        return kind[tag if tag in kind else tag[0]](p, x)

    def trunk(self, x, taps=None):
        """x (N, 3, 299, 299) -> (N, 2048, 8, 8); taps: a dict that receives every block's output."""
        x = self.q(x.to(self.dtype))

        def tap(name, y):
            if taps is not None:
                taps[name] = y
            return y
        x = tap("Conv2d_1a_3x3", self.conv("Conv2d_1a_3x3", x, stride=2))
        x = tap("Conv2d_2a_3x3", self.conv("Conv2d_2a_3x3", x))
        x = tap("Conv2d_2b_3x3", self.conv("Conv2d_2b_3x3", x, padding=1))
        x = tap("maxpool1", F.max_pool2d(x, 3, stride=2))
        x = tap("Conv2d_3b_1x1", self.conv("Conv2d_3b_1x1", x))
        x = tap("Conv2d_4a_3x3", self.conv("Conv2d_4a_3x3", x))
        x = tap("maxpool2", F.max_pool2d(x, 3, stride=2))
        for p in BLOCKS[7:]:
            x = tap(p, self.block(p, x))
        return x

    def features(self, x, taps=None):
        """x (N, 3, 299, 299) in [-1, 1] -> (N, 2048)."""
        y = self.trunk(x, taps)
        if self.f16:
            n, c, h, w = y.shape
            return ordered_mean(y.permute(0, 2, 3, 1).reshape(n, h * w, c))
        return y.mean(dim=(2, 3))

    def logits(self, feats):
        dt = feats.dtype
        return feats @ self.sd["fc.weight"].to(dt).T + self.sd["fc.bias"].to(dt)


def ordered_mean(rows):
    """rows (N, R, C) (f16 values in any float dtype) -> fp32 (N, C): one fp32 accumulator per channel, the R rows added in
    ascending order, one fp32 division: rcdm_global_avgpool's order."""
    rows = rows.float()
    s = torch.zeros(rows.shape[0], rows.shape[2], dtype=torch.float32)
    for r in range(rows.shape[1]):
        s = s + rows[:, r]
    return s / torch.tensor(float(rows.shape[1]), dtype=torch.float32)


def _axis(out, inp):
    scale = torch.tensor(float(inp), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    o = torch.arange(out, dtype=torch.float32)
    # one fused multiply-add, as torch's CPU build evaluates it: the product of a 24-bit and an 11-bit number is exact in float64
    s = (scale.double() * (o + 0.5).double() - 0.5).float()
    s = torch.clamp(s, min=0.0)
    i0 = torch.clamp(s.to(torch.int64), max=inp - 1)
    i1 = torch.clamp(i0 + 1, max=inp - 1)
    l1 = s - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def resize(frames_u8, size=(299, 299), scale=2.0, shift=-1.0):
    """frames (N, H, W, 3) uint8 -> fp32 (N, 3, oh, ow): bilinear of x / 255 written out (source coordinate
    max(fma(in / out, o + 0.5, -0.5), 0), upper neighbour clamped to in - 1, horizontal lerp inside the vertical one, all fp32),
    then * scale + shift."""
    x = frames_u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    oh, ow = size
    y0, y1, wy0, wy1 = _axis(oh, x.shape[2])
    x0, x1, wx0, wx1 = _axis(ow, x.shape[3])
    top, bot = x[:, :, y0], x[:, :, y1]
    top = wx0 * top[..., x0] + wx1 * top[..., x1]
    bot = wx0 * bot[..., x0] + wx1 * bot[..., x1]
    v = wy0[:, None] * top + wy1[:, None] * bot
    return v * scale + shift


def features(sd, frames_u8, variant="fid", dtype=torch.float32, f16=False, taps=None):
    """uint8 frames (N, H, W, 3) -> (N, 2048): resize to 299 x 299 in [-1, 1], then the network."""
    net = Net(sd, variant, dtype, f16)
    return net.features(resize(frames_u8), taps)
