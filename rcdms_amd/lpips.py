"""LPIPS on the HIP path: uint8 frame pairs -> the learned perceptual distance of Zhang et al. (The Unreasonable Effectiveness of
Deep Features as a Perceptual Metric, 2018), version 0.1, over a VGG-16 or an AlexNet tower.

  rcdm_lpips_input_rows   frames -> the tower's f16 input rows with the scaling layer applied, f16(fma(u8 / 255, 2 / scale,
                          (-1 - shift) / scale)) = (2 u8 / 255 - 1 - shift) / scale: 3 channels padded to 8 for VGG; for AlexNet
                          the space-to-depth rows of its 11 x 11 stride-4 stem (48 channels, a 3 x 3 stride-1 conv over them)
  rcdm_conv2d             every conv with the bias + ReLU epilogue (the taps are post-ReLU);  rcdm_pool2d: the max pools
  rcdm_lpips_head         per tap: channel-normalise both feature maps, lin-weighted squared difference, spatial mean -> float64

The 2 P frames of a chunk run through the tower as one batch, the a-frames first, so the head reads both halves of one buffer.
Nothing is resized (the lpips package does not resize either).  A launch plan (buffers, descriptors, one stream, program order)
per (net, pairs, H, W) is kept in a small LRU, and many pairs run in chunks of `batch`; a chunked run gives the bits of an
unchunked one.  The weights are the caller's, fp32 rounded once to f16 (biases and lin stay fp32); none ship with the project.

State-dict keys (the lpips package's, or torchvision's for the backbone):
  convs   net.slice<k>.<i>.{weight,bias} or features.<i>.{weight,bias}, i the torchvision `features` index
          (VGG-16: 0 2 | 5 7 | 10 12 14 | 17 19 21 | 24 26 28, taps after 2, 7, 14, 21, 28;  AlexNet: 0 | 3 | 6 | 8 | 10, every one a tap)
  heads   lin<k>.model.1.weight or lins.<k>.model.1.weight, k = 0 .. 4, shape (1, C, 1, 1), non-negative
  scaling_layer.shift / scaling_layer.scale: optional, default to v0.1's constants.
Restated from the paper and the package's published forward, unpinned: the package is not a dependency and no run against it
backs the key names.  No CPU path: a host tensor raises."""
from collections import OrderedDict

import numpy as np
import torch

from . import hip
from .inception import _Act, _out_side
from .metrics import _frames, _view

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
NETS = ("vgg", "alex")
MIN_SIDE = {"vgg": 16, "alex": 31}

# (features index, c_in, c_out, kernel, stride, pad, slice)
CONVS = {
    "vgg": ((0, 3, 64, 3, 1, 1, 1), (2, 64, 64, 3, 1, 1, 1), (5, 64, 128, 3, 1, 1, 2), (7, 128, 128, 3, 1, 1, 2),
            (10, 128, 256, 3, 1, 1, 3), (12, 256, 256, 3, 1, 1, 3), (14, 256, 256, 3, 1, 1, 3), (17, 256, 512, 3, 1, 1, 4),
            (19, 512, 512, 3, 1, 1, 4), (21, 512, 512, 3, 1, 1, 4), (24, 512, 512, 3, 1, 1, 5), (26, 512, 512, 3, 1, 1, 5),
            (28, 512, 512, 3, 1, 1, 5)),
    "alex": ((0, 3, 64, 11, 4, 2, 1), (3, 64, 192, 5, 1, 2, 2), (6, 192, 384, 3, 1, 1, 3), (8, 384, 256, 3, 1, 1, 4),
             (10, 256, 256, 3, 1, 1, 5)),
}
TAPS = {"vgg": (2, 7, 14, 21, 28), "alex": (0, 3, 6, 8, 10)}               # a tap follows these convs
POOL_BEFORE = {"vgg": {5: (2, 2), 10: (2, 2), 17: (2, 2), 24: (2, 2)}, "alex": {3: (3, 2), 6: (3, 2)}}   # index -> (window, stride)
TAP_CHANNELS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}


def _net(net):
    if net not in NETS:
        raise ValueError(f"net {net!r}: one of {NETS}")
    return net


def _find(sd, names):
    for k in names:
        if k in sd:
            return k
    raise ValueError(f"state dict lacks {names[0]} (also looked for {', '.join(names[1:])})")


def check_state_dict(sd, net):
    """ValueError for a missing, mis-shaped or (lin) negative key; -> {"conv<i>": (weight key, bias key), "lin<k>": key,
    "shift": key | None, "scale": key | None}.  Needs no device."""
    _net(net)
    keys = {}
    for i, cin, cout, k, _, _, sl in CONVS[net]:
        pair = []
        for part, shape in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            key = _find(sd, (f"net.slice{sl}.{i}.{part}", f"features.{i}.{part}"))
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"{key} is {shape}, got {tuple(sd[key].shape)}")
            pair.append(key)
        keys[f"conv{i}"] = tuple(pair)
    for t, c in enumerate(TAP_CHANNELS[net]):
        key = _find(sd, (f"lin{t}.model.1.weight", f"lins.{t}.model.1.weight"))
        if tuple(sd[key].shape) != (1, c, 1, 1):
            raise ValueError(f"{key} is {(1, c, 1, 1)}, got {tuple(sd[key].shape)}")
        w = sd[key].detach().to("cpu", torch.float32)
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError(f"{key} holds a negative or non-finite weight: LPIPS's lin layers are non-negative")
        keys[f"lin{t}"] = key
    for part in ("shift", "scale"):
        key = f"scaling_layer.{part}"
        keys[part] = key if key in sd else None
        if key in sd:
            v = sd[key].detach().to("cpu", torch.float64).reshape(-1)
            if v.numel() != 3 or not bool(torch.isfinite(v).all()) or (part == "scale" and not bool((v > 0).all())):
                raise ValueError(f"{key} holds three finite numbers (scale above 0), got {tuple(sd[key].shape)}")
    return keys


def check_sides(net, H, W):
    m = MIN_SIDE[_net(net)]
    if H < m or W < m:
        raise ValueError(f"LPIPS over {net} takes frames of at least {m} x {m} (the last tap would be empty), got {H} x {W}")


def input_constants(shift=SHIFT, scale=SCALE):
    """-> (mul, add), three fp32 values each: 2 / scale and (-1 - shift) / scale formed in float64 and rounded once."""
    shift, scale = [float(v) for v in shift], [float(v) for v in scale]
    return (tuple(float(np.float32(2.0 / s)) for s in scale), tuple(float(np.float32((-1.0 - h) / s)) for h, s in zip(shift, scale)))


def conv_rows(w):
    """torch weight (c_out, c_in, kh, kw) fp32 -> f16 [c_out][kh * kw * c_in_padded] in rcdm_conv2d's order (c_in padded to 8)."""
    w = w.detach().to("cpu", torch.float32).permute(0, 2, 3, 1)
    pad = (-w.shape[-1]) % 8
    if pad:
        w = torch.nn.functional.pad(w, (0, pad))
    return w.reshape(w.shape[0], -1).to(torch.float16).contiguous()


def alex_stem_rows(w):
    """AlexNet's (64, 3, 11, 11) stem weight -> f16 [64][3 * 3 * 48] for the 3 x 3 conv over the space-to-depth rows:
    W'[o][(KY 3 + KX) 48 + (dy 4 + dx) 3 + ch] = W[o][ch][4 KY + dy][4 KX + dx], zeros where 4 K + d = 11."""
    w = w.detach().to("cpu", torch.float32)
    cout = w.shape[0]
    w12 = torch.zeros(cout, 3, 12, 12, dtype=torch.float32)
    w12[:, :, :11, :11] = w
    w12 = w12.view(cout, 3, 3, 4, 3, 4)                        # (o, ch, KY, dy, KX, dx)
    return w12.permute(0, 2, 4, 3, 5, 1).reshape(cout, 3 * 3 * 48).to(torch.float16).contiguous()   # (o, KY, KX, dy, dx, ch)


class _Plan:
    """The launches of one chunk at a fixed (pairs, H, W): buffers, descriptors, pointers, in program order."""

    def __init__(self, net, pairs, H, W):
        self.net, self.pairs, self.n = net, pairs, 2 * pairs
        self.ops, self.bufs, self.taps, self.heads = [], [], [], []
        dev = net.device
        self.s2d = 4 if net.net == "alex" else 1
        mul, add = net.constants
        self.in_desc = lambda pitch, stride: hip.LpipsInputDesc(pitch, stride, pairs, H, W, self.s2d, self.x0.ld, mul, add)
        h0, w0, c0 = hip.lpips_input_sides(hip.LpipsInputDesc(3 * W, 0, pairs, H, W, self.s2d, 48 if self.s2d == 4 else 8, mul, add))
        self.x0 = x = self.buf(h0, w0, c0)
        for i, _, cout, k, s, p, _ in CONVS[net.net]:
            if i in POOL_BEFORE[net.net]:
                pk, ps = POOL_BEFORE[net.net][i]
                x = self.pool(x, pk, ps)
            if net.net == "alex" and i == 0:
                k, s, p = 3, 1, 0                              # the stem over its space-to-depth rows
            x = self.conv(i, x, cout, k, s, p)
            if i in TAPS[net.net]:
                self.taps.append(x)
        for t, x in enumerate(self.taps):
            d = hip.LpipsHeadDesc(x.ld, x.ld, pairs, x.h, x.w, x.c, 0, 0)
            nbytes = hip.lpips_head_workspace_bytes(d)
            if nbytes == 0:
                raise hip.RcdmError(f"rcdm_lpips_head refuses tap {t}: {pairs} pairs of {x.h}x{x.w}x{x.c}")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.heads.append((d, x.ptr, x.ptr + 2 * pairs * x.h * x.w * x.ld, net.lins[t].data_ptr(), ws))

    def buf(self, h, w, c):
        t = torch.empty(self.n * h * w, c, dtype=torch.float16, device=self.net.device)
        self.bufs.append(t)
        return _Act(t, 0, c, h, w)

    def conv(self, i, a, cout, k, s, p):
        W, b = self.net.weights[i]
        cin = W.shape[1] // (k * k)
        assert a.c == cin, (i, a.c, cin)
        out = self.buf(_out_side(a.h, k, s, p), _out_side(a.w, k, s, p), cout)
        d = hip.Conv2dDesc(self.n, a.h, a.w, cin, cout, k, k, s, s, p, p, a.ld, out.ld, hip.EPI_BIAS | hip.EPI_RELU)
        self.ops.append((hip.conv2d, (d, a.ptr, W.data_ptr(), b.data_ptr(), out.ptr)))
        return out

    def pool(self, a, k, s):
        out = self.buf(_out_side(a.h, k, s, 0), _out_side(a.w, k, s, 0), a.c)
        d = hip.Pool2dDesc(self.n, a.h, a.w, a.c, k, k, s, s, 0, 0, a.ld, out.ld, hip.POOL_MAX)
        self.ops.append((hip.pool2d, (d, a.ptr, out.ptr)))
        return out

    def run(self, a, b, out):
        """a, b: (pairs, H, W, 3) uint8 views; out: float64 (5, >= pairs) rows whose first `pairs` entries are written."""
        x0 = self.x0
        for half, f in enumerate((a, b)):
            pitch = f.stride(1) if f.shape[1] > 1 else 3 * f.shape[2]
            stride = f.stride(0) if f.shape[0] > 1 else 0
            hip.lpips_input_rows(self.in_desc(pitch, stride), f.data_ptr(), x0.ptr + 2 * half * self.pairs * x0.h * x0.w * x0.ld)
        for fn, args in self.ops:
            fn(*args)
        for t, (d, pa, pb, lin, ws) in enumerate(self.heads):
            hip.lpips_head(d, pa, pb, lin, out[t].data_ptr(), ws.data_ptr(), ws.numel())


class LpipsNet:
    """state_dict: the lpips package's keys (module docstring); net: "vgg" or "alex"; batch: pairs per chunk of a large call;
    plans: launch plans kept.  net(a, b) -> float64 distances with the leading shape of a."""

    def __init__(self, state_dict, net="vgg", device="cuda", batch=8, plans=4):
        self.net = _net(net)
        keys = check_state_dict(state_dict, net)
        if int(batch) < 1 or int(plans) < 1:
            raise ValueError("batch and plans are at least 1")
        self.batch, self.max_plans = int(batch), int(plans)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip.RcdmError("LpipsNet runs on the HIP path only: there is no CPU path here")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        hip.load()
        cpu = lambda k: state_dict[k].detach().to("cpu", torch.float64).reshape(-1).tolist()
        self.constants = input_constants(SHIFT if keys["shift"] is None else cpu(keys["shift"]),
                                         SCALE if keys["scale"] is None else cpu(keys["scale"]))
        self.weights = {}
        for i, *_ in CONVS[net]:
            wk, bk = keys[f"conv{i}"]
            rows = alex_stem_rows(state_dict[wk]) if (net == "alex" and i == 0) else conv_rows(state_dict[wk])
            self.weights[i] = (rows.to(self.device), state_dict[bk].detach().to("cpu", torch.float32).contiguous().to(self.device))
        self.lins = [state_dict[keys[f"lin{t}"]].detach().to("cpu", torch.float32).reshape(-1).contiguous().to(self.device)
                     for t in range(5)]
        self._plans = OrderedDict()
        self.plans_built = 0

    def _plan(self, pairs, H, W):
        key = (self.net, pairs, H, W)
        plan = self._plans.get(key)
        if plan is None:
            plan = _Plan(self, pairs, H, W)
            self.plans_built += 1
            self._plans[key] = plan
            while len(self._plans) > self.max_plans:
                self._plans.popitem(last=False)
        else:
            self._plans.move_to_end(key)
        return plan

    def _checked(self, a, b):
        a, b = _frames("a", a), _frames("b", b)
        if a.shape != b.shape:
            raise ValueError(f"`a` {tuple(a.shape)} and `b` {tuple(b.shape)} differ in shape")
        check_sides(self.net, a.shape[-3], a.shape[-2])
        if not a.is_cuda or not b.is_cuda:
            raise hip.RcdmError("LpipsNet runs on the HIP path only: a and b must be device tensors (there is no CPU path here)")
        if a.device != self.device or b.device != self.device:
            raise ValueError(f"frames are on {a.device} and {b.device}, the network on {self.device}")
        return _view(a), _view(b)

    @torch.no_grad()
    def taps(self, a, b):
        """The five tapped feature maps of ONE chunk (all pairs at once): a list of f16 (2 P, h, w, C) views of the plan's
        buffers, the a-frames first (valid until the next call of this shape), and the (P, 5) distances.  For tests."""
        va, vb = self._checked(a, b)
        P = va.shape[0]
        out = torch.empty(5, P, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            plan = self._plan(P, va.shape[1], va.shape[2])
            plan.run(va, vb, out)
        return [x.t.view(2 * P, x.h, x.w, x.c) for x in plan.taps], out.t()

    @torch.no_grad()
    def __call__(self, a, b, return_layers=False):
        """a, b: device uint8 (..., H, W, 3) of equal shape, RGB; slices and strips are read by their pitch, without a copy.
        -> float64 with the leading shape of a: ((((d0 + d1) + d2) + d3) + d4); with return_layers (that, the (..., 5) taps)."""
        lead = tuple(a.shape[:-3]) if isinstance(a, torch.Tensor) else ()
        va, vb = self._checked(a, b)
        N, H, W = va.shape[0], va.shape[1], va.shape[2]
        out = torch.empty(5, N, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for i in range(0, N, self.batch):
                j = min(N, i + self.batch)
                self._plan(j - i, H, W).run(va[i:j], vb[i:j], out[:, i:])
        total = out[0] + out[1]
        for t in (2, 3, 4):
            total = total + out[t]
        total, layers = total.view(lead), out.t().reshape(lead + (5,))
        return (total, layers) if return_layers else total
