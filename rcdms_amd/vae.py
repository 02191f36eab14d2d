"""VAE of the stage-2 pipeline on the HIP path: decoder (`AutoencoderKLDecoder`) and, with the encoder
added, the whole module (`AutoencoderKL`).

Replaces `self.vae.decode(latents[i:i+1]).sample`, called once per frame at src/pipelines/RCDMs_pipeline.py:274-287 on
the SD-1.5 `AutoencoderKL` (diffusers==0.24.0, third party — restated from the published architecture, PARITY UNPINNED:
see oracle/vae_oracle.py).  `AutoencoderKLDecoder` holds the decoder-side parameters under the diffusers 0.24 key names
(`post_quant_conv.*`, `decoder.*`), so `load_state_dict(vae_state_dict, strict=False)` takes a real checkpoint, and
decodes all frames in one batch on the stage-2 kernels: conv3x3 implicit GEMM (nearest-2x upsampling folded into the
conv's input indexing), per-image GroupNorm(+SiLU), 1x1 shortcuts as GEMMs.  The mid-block attention has ONE head of
512 channels and two forms (mid_attention_form, switch RCDM_VAE_FLASH).  "scores", the default up to 4096 latent pixels
(512 x 512 images): per image scores = Q K^T (GEMM, scaled in the epilogue), row softmax (rcdm_softmax_rows, rows of
<= 4096), out = P V (GEMM against V^T, which a GEMM with swapped operands produces directly).  "flash", above: one
[q | k | v] GEMM and ONE rcdm_flash_attn launch over all images (head dim 512: csrc/attn_wide.hip), no hw x hw buffer,
so any image size the convolutions take.  In both the value bias is folded into the output projection (softmax rows
sum to one).

`AutoencoderKL` adds `encoder.*` / `quant_conv.*` and `encode(x).latent_dist` (RCDMs_pipeline.py:429, one call per story on
the masked source frames): the same kernels, with diffusers' Downsample2D(padding=0) — F.pad (0,1,0,1) then a stride-2
conv — as the conv kernel's pad-after-only form (rcdm_conv3x3_desc.pad_after_only).  No CPU path."""
import torch
from torch import nn

from . import hip
from . import switches as SW
from .engine import (CIN_PAD, COUT_PAD, Geo, Packer, Plan, Rows, _NS, emit_conv3x3, emit_flash_attn, emit_gemm,
                     emit_groupnorm, emit_upsample_conv)

SD15_VAE = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, out_channels=3,
                in_channels=3, norm_num_groups=32, scaling_factor=0.18215)


class _Resnet(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _Attn(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c), nn.Dropout(0.0)])


class _Mid(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(c, c, groups), _Resnet(c, c, groups)])
        self.attentions = nn.ModuleList([_Attn(c, groups)])


class _Up(nn.Module):
    def __init__(self, cin, cout, n, groups, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if j == 0 else cout, cout, groups) for j in range(n)])
        if upsample:
            up = nn.Module()
            up.conv = nn.Conv2d(cout, cout, 3, padding=1)
            self.upsamplers = nn.ModuleList([up])


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        boc, g = list(cfg["block_out_channels"]), cfg["norm_num_groups"]
        rev = boc[::-1]
        self.conv_in = nn.Conv2d(cfg["latent_channels"], rev[0], 3, padding=1)
        self.mid_block = _Mid(rev[0], g)
        ups, prev = [], rev[0]
        for i, c in enumerate(rev):
            ups.append(_Up(prev, c, cfg["layers_per_block"] + 1, g, i < len(rev) - 1))
            prev = c
        self.up_blocks = nn.ModuleList(ups)
        self.conv_norm_out = nn.GroupNorm(g, rev[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(rev[-1], cfg["out_channels"], 3, padding=1)


class _Down(nn.Module):
    def __init__(self, cin, cout, n, groups, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if j == 0 else cout, cout, groups) for j in range(n)])
        if downsample:
            dn = nn.Module()
            dn.conv = nn.Conv2d(cout, cout, 3, stride=2, padding=0)
            self.downsamplers = nn.ModuleList([dn])


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        boc, g = list(cfg["block_out_channels"]), cfg["norm_num_groups"]
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        downs, prev = [], boc[0]
        for i, c in enumerate(boc):
            downs.append(_Down(prev, c, cfg["layers_per_block"], g, i < len(boc) - 1))
            prev = c
        self.down_blocks = nn.ModuleList(downs)
        self.mid_block = _Mid(boc[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, boc[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(boc[-1], 2 * cfg["latent_channels"], 3, padding=1)


class _Sample:
    def __init__(self, sample):
        self.sample = sample


class AutoencoderKLDecoder(nn.Module):
    """Decoder half of diffusers' AutoencoderKL: `decode(z) -> .sample` for z (n, 4, h, w), any n (frames batched)."""

    def __init__(self, **cfg):
        super().__init__()
        self.cfg = dict(SD15_VAE)
        self.cfg.update(cfg)
        self.post_quant_conv = nn.Conv2d(self.cfg["latent_channels"], self.cfg["latent_channels"], 1)
        self.decoder = _Decoder(self.cfg)
        self._programs = {}

    @property
    def device(self):
        return self.post_quant_conv.weight.device

    @property
    def dtype(self):
        return self.post_quant_conv.weight.dtype

    def encode(self, x):
        raise NotImplementedError("AutoencoderKLDecoder holds the decoder half only; keep the torch AutoencoderKL for "
                                  "`encode` (one call per story, RCDMs_pipeline.py:429)")

    @torch.no_grad()
    def decode(self, z, return_dict=True):
        if self.device.type != "cuda":
            raise hip.RcdmError(f"AutoencoderKLDecoder runs on the HIP path only (module is on {self.device})")
        out = self._decode_program(z).forward(z).to(z.dtype)
        return _Sample(out) if return_dict else (out,)

    def _decode_program(self, z):
        n, c, h, w = z.shape
        key = (n, h, w, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        prog = self._programs.get((n, h, w))
        if prog is None or prog[0] != key:
            prog = (key, VaeDecodeProgram(self.cfg, self.state_dict(), n, h, w, self.device))
            self._programs[(n, h, w)] = prog
        return prog[1]

    @torch.no_grad()
    def decode_uint8(self, z):
        """z (n, 4, h, w) -> device uint8 frames (n, 8h, 8w, 3): the decode plan, then rcdm_frames_to_u8 straight from the
        decoder's f16 pixel rows — trunc(clamp(x / 2 + 0.5, 0, 1) * 255), what RCDMs_pipeline.py:274-287 and the driver's
        `(x * 255).astype(uint8)` make of `decode(z).sample`, without the fp32 NCHW tensor in between."""
        if self.device.type != "cuda":
            raise hip.RcdmError(f"AutoencoderKLDecoder runs on the HIP path only (module is on {self.device})")
        return self._decode_program(z).forward_uint8(z)

    @torch.no_grad()
    def decode_png(self, z, filter="adaptive", match=False):
        """z (n, 4, h, w) -> n PNG files as `bytes`: decode_uint8, then rcdm_png_encode on those frames (image.encode_png);
        match=True: rcdm_png_encode_match."""
        from .image import encode_png
        return encode_png(self.decode_uint8(z), filter, match)


class DiagonalGaussianDistribution:
    """`encode(x).latent_dist`: mean / logvar (clamped to [-30, 20]) of the posterior, as diffusers' class of this name."""

    def __init__(self, mean, logvar):
        self.mean, self.logvar = mean, logvar
        self.std = torch.exp(0.5 * logvar)
        self.var = torch.exp(logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean


class _Posterior:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class AutoencoderKL(AutoencoderKLDecoder):
    """Both halves under the diffusers 0.24 key names (248 tensors at the SD-1.5 shape): a drop-in for the pipeline's
    `vae` argument — `encode(x).latent_dist.sample(generator)`, `decode(z).sample`, `config.block_out_channels` /
    `config.scaling_factor`."""

    def __init__(self, **cfg):
        super().__init__(**cfg)
        lc = self.cfg["latent_channels"]
        self.encoder = _Encoder(self.cfg)
        self.quant_conv = nn.Conv2d(2 * lc, 2 * lc, 1)
        self.config = _NS(**self.cfg)
        self._enc_programs = {}

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        if self.device.type != "cuda":
            raise hip.RcdmError(f"AutoencoderKL runs on the HIP path only (module is on {self.device})")
        n, c, h, w = x.shape
        mean, logvar = self._encode_program(n, h, w).forward(x)
        dist = DiagonalGaussianDistribution(mean.to(x.dtype), logvar.to(x.dtype))
        return _Posterior(dist) if return_dict else (dist,)

    def _encode_program(self, n, h, w):
        key = (n, h, w, tuple((p.data_ptr(), p._version) for p in self.parameters()))
        prog = self._enc_programs.get((n, h, w))
        if prog is None or prog[0] != key:
            prog = (key, VaeEncodeProgram(self.cfg, self.state_dict(), n, h, w, self.device))
            self._enc_programs[(n, h, w)] = prog
        return prog[1]

    @torch.no_grad()
    def encode_frames(self, frames, transform, return_dict=True):
        """`encode(transform(frames))` for uint8 frames and an rcdms_amd.image.FrameTransform, without the fp32 tensor:
        the transform writes its f16 pixel rows straight into the encode plan's input buffer.  Same posterior, bit for bit."""
        if self.device.type != "cuda":
            raise hip.RcdmError(f"AutoencoderKL runs on the HIP path only (module is on {self.device})")
        from .image import to_device_frames
        groups = to_device_frames(frames, self.device)
        if len(groups) != 1:
            raise ValueError("encode_frames takes one batch of equally sized frames")
        n = groups[0].shape[0]
        mean, logvar = self._encode_program(n, transform.height, transform.width).forward_rows(
            lambda rows: transform(groups[0], rows=True, out=rows), keep=groups[0])
        dist = DiagonalGaussianDistribution(mean.to(self.dtype), logvar.to(self.dtype))
        return _Posterior(dist) if return_dict else (dist,)


def _pack_resnet(pk, p):
    w = _NS(cin=pk.sd[p + "conv1.weight"].shape[1], cout=pk.sd[p + "conv1.weight"].shape[0])
    w.g1, w.b1 = pk.vec(p + "norm1.weight"), pk.vec(p + "norm1.bias")
    w.g2, w.b2 = pk.vec(p + "norm2.weight"), pk.vec(p + "norm2.bias")
    w.conv1, w.cb1 = pk.conv3x3(p + "conv1.weight"), pk.vec(p + "conv1.bias")
    w.conv2, w.cb2 = pk.conv3x3(p + "conv2.weight"), pk.vec(p + "conv2.bias")
    w.shortcut = None
    if pk.has(p + "conv_shortcut.weight"):
        w.shortcut, w.sb = pk.mat_f16(p + "conv_shortcut.weight"), pk.vec(p + "conv_shortcut.bias")
    return w


def _emit_resnet2d(plan, w, x, geo, out, groups):
    """diffusers ResnetBlock2D without time embedding: GroupNorm statistics per image, eps 1e-6."""
    g = geo
    a1 = plan.rows("norm", g.M, w.cin)
    emit_groupnorm(plan, x, g.n_img, g.hw, w.g1, w.b1, 1e-6, True, a1, groups)
    h1 = plan.rows("res_h1", g.M, w.cout)
    emit_conv3x3(plan, a1, g.n_img, g.H, g.W, w.conv1, w.cin, w.cout, h1, bias=w.cb1)
    a2 = plan.rows("norm", g.M, w.cout)
    emit_groupnorm(plan, h1, g.n_img, g.hw, w.g2, w.b2, 1e-6, True, a2, groups)
    res = x
    if w.shortcut is not None:
        res = plan.rows("res_sc", g.M, w.cout)
        emit_gemm(plan, x, w.shortcut, w.cout, w.cin, res, bias=w.sb)
    emit_conv3x3(plan, a2, g.n_img, g.H, g.W, w.conv2, w.cout, w.cout, out, bias=w.cb2, residual=res)


class VaeDecodeProgram:
    """Static launch plan of AutoencoderKL.decode for n images of h x w latents."""

    def __init__(self, cfg, sd, n, h, w, device):
        hip.load()
        self.cfg, self.n, self.h, self.w = cfg, n, h, w
        self.device = torch.device(device)
        groups = cfg["norm_num_groups"]
        lc = cfg["latent_channels"]
        rev = list(cfg["block_out_channels"])[::-1]
        if lc > 8 or cfg["out_channels"] > COUT_PAD:
            raise NotImplementedError("latent_channels <= 8 and out_channels <= 8")
        pk = Packer(sd, self.device)
        self.plan = plan = Plan(self.device)
        g0 = Geo(n, 1, h, w)
        # post_quant_conv (1x1, lc -> lc) as an 8 x 8 GEMM whose output lands in the zero-padded 64-channel row conv_in reads
        pq_w = torch.zeros(8, 8, device=self.device)
        pq_w[:lc, :lc] = pk.f32("post_quant_conv.weight").reshape(lc, lc)
        self.pq_w = pq_w.to(torch.float16).contiguous()
        self.pq_b = torch.cat([pk.vec("post_quant_conv.bias"), torch.zeros(8 - lc, device=self.device)]).contiguous()
        self.z_rows = plan.rows("vae_z", g0.M, 8, unique=True)
        self.x_in = plan.rows("vae_x_in", g0.M, CIN_PAD, unique=True)
        emit_gemm(plan, self.z_rows, self.pq_w, 8, 8, self.x_in.cols(0, 8), bias=self.pq_b)
        top = rev[0]
        cur = plan.rows("vae_a", g0.M, top, unique=True)
        emit_conv3x3(plan, self.x_in, n, h, w, pk.conv3x3("decoder.conv_in.weight", cin_pad=CIN_PAD), CIN_PAD, top, cur,
                     bias=pk.vec("decoder.conv_in.bias"))
        nxt = plan.rows("vae_b", g0.M, top, unique=True)
        cur = _emit_mid_block(plan, pk, "decoder.mid_block.", cur, nxt, g0, groups)
        geo = g0
        idx = 0
        for i, c in enumerate(rev):
            for j in range(cfg["layers_per_block"] + 1):
                out = plan.rows(f"vae_s{idx}", geo.M, c, unique=True)
                idx += 1
                _emit_resnet2d(plan, _pack_resnet(pk, f"decoder.up_blocks.{i}.resnets.{j}."), cur, geo, out, groups)
                cur = out
            if i < len(rev) - 1:
                up = Geo(n, 1, geo.H * 2, geo.W * 2)
                out = plan.rows(f"vae_s{idx}", up.M, c, unique=True)
                idx += 1
                p = f"decoder.up_blocks.{i}.upsamplers.0.conv."
                emit_upsample_conv(plan, pk, p + "weight", cur, n, geo.H, geo.W, c, out, pk.vec(p + "bias"))
                cur, geo = out, up
        a = plan.rows("norm", geo.M, rev[-1])
        emit_groupnorm(plan, cur, n, geo.hw, pk.vec("decoder.conv_norm_out.weight"), pk.vec("decoder.conv_norm_out.bias"),
                       1e-6, True, a, groups)
        oc = cfg["out_channels"]
        co_w = pk.conv3x3("decoder.conv_out.weight", cout_pad=COUT_PAD)
        co_b = torch.cat([pk.vec("decoder.conv_out.bias"), torch.zeros(COUT_PAD - oc, device=self.device)]).contiguous()
        self.out_rows = plan.rows("vae_out", geo.M, COUT_PAD, unique=True)
        emit_conv3x3(plan, a, n, geo.H, geo.W, co_w, rev[-1], COUT_PAD, self.out_rows, bias=co_b)
        self.out_geo = geo
        pk.done()
        plan.materialize()
        self.stream = torch.cuda.Stream(device=self.device)

    @torch.no_grad()
    def forward(self, z):
        n, c, h, w = z.shape
        assert (n, h, w) == (self.n, self.h, self.w)
        cur = torch.cuda.current_stream(self.device)
        z32 = z.detach().to(self.device, torch.float32).contiguous()
        g = self.out_geo
        out = torch.empty(n, self.cfg["out_channels"], 1, g.H, g.W, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            hip.ncfhw_to_rows(z32.data_ptr(), n, c, 1, h, w, self.z_rows.ptr, self.z_rows.ld, 8)
            self.plan.run()
            hip.rows_to_ncfhw(self.out_rows.ptr, self.out_rows.ld, n, self.cfg["out_channels"], 1, g.H, g.W, out.data_ptr())
        cur.wait_stream(self.stream)
        z32.record_stream(self.stream)
        return out[:, :, 0]

    @torch.no_grad()
    def forward_uint8(self, z):
        """As forward, but the f16 pixel rows go straight to uint8 frames (n, H, W, 3)."""
        from .image import frames_to_uint8
        n, c, h, w = z.shape
        assert (n, h, w) == (self.n, self.h, self.w)
        cur = torch.cuda.current_stream(self.device)
        z32 = z.detach().to(self.device, torch.float32).contiguous()
        g = self.out_geo
        out = torch.empty(n, g.H, g.W, 3, dtype=torch.uint8, device=self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            hip.ncfhw_to_rows(z32.data_ptr(), n, c, 1, h, w, self.z_rows.ptr, self.z_rows.ld, 8)
            self.plan.run()
            frames_to_uint8((self.out_rows, n, g.H, g.W), out=out)
        cur.wait_stream(self.stream)
        z32.record_stream(self.stream)
        return out


class VaeEncodeProgram:
    """Static launch plan of AutoencoderKL.encode for n images of H x W pixels: -> posterior mean and clamped logvar."""

    def __init__(self, cfg, sd, n, H, W, device):
        hip.load()
        self.cfg, self.n, self.H, self.W = cfg, n, H, W
        self.device = torch.device(device)
        groups, lc = cfg["norm_num_groups"], cfg["latent_channels"]
        boc = list(cfg["block_out_channels"])
        down = 2 ** (len(boc) - 1)
        if 2 * lc != COUT_PAD or cfg["in_channels"] > 8:
            raise NotImplementedError("latent_channels == 4 and in_channels <= 8")
        if H % down or W % down:
            raise ValueError(f"image size {H}x{W} must be a multiple of {down}")
        pk = Packer(sd, self.device)
        self.plan = plan = Plan(self.device)
        geo = Geo(n, 1, H, W)
        self.x_in = plan.rows("vae_px", geo.M, CIN_PAD, unique=True)      # pixels, channels zero-padded to 64
        cur = plan.rows("vae_e0", geo.M, boc[0], unique=True)
        emit_conv3x3(plan, self.x_in, n, H, W, pk.conv3x3("encoder.conv_in.weight", cin_pad=CIN_PAD), CIN_PAD, boc[0], cur,
                     bias=pk.vec("encoder.conv_in.bias"))
        idx = 1
        for i, c in enumerate(boc):
            for j in range(cfg["layers_per_block"]):
                out = plan.rows(f"vae_e{idx}", geo.M, c, unique=True)
                idx += 1
                _emit_resnet2d(plan, _pack_resnet(pk, f"encoder.down_blocks.{i}.resnets.{j}."), cur, geo, out, groups)
                cur = out
            if i < len(boc) - 1:
                dn = Geo(n, 1, geo.H // 2, geo.W // 2)
                out = plan.rows(f"vae_e{idx}", dn.M, c, unique=True)
                idx += 1
                p = f"encoder.down_blocks.{i}.downsamplers.0.conv."
                emit_conv3x3(plan, cur, n, geo.H, geo.W, pk.conv3x3(p + "weight"), c, c, out, stride=2, pad_after_only=1,
                             bias=pk.vec(p + "bias"))
                cur, geo = out, dn
        nxt = plan.rows("vae_eb", geo.M, boc[-1], unique=True)
        cur = _emit_mid_block(plan, pk, "encoder.mid_block.", cur, nxt, geo, groups)
        a = plan.rows("norm", geo.M, boc[-1])
        emit_groupnorm(plan, cur, n, geo.hw, pk.vec("encoder.conv_norm_out.weight"), pk.vec("encoder.conv_norm_out.bias"),
                       1e-6, True, a, groups)
        mom = plan.rows("vae_mom", geo.M, COUT_PAD, unique=True)
        emit_conv3x3(plan, a, n, geo.H, geo.W, pk.conv3x3("encoder.conv_out.weight"), boc[-1], COUT_PAD, mom,
                     bias=pk.vec("encoder.conv_out.bias"))
        self.q_w = pk.f32("quant_conv.weight").reshape(2 * lc, 2 * lc).to(torch.float16).contiguous()
        self.out_rows = plan.rows("vae_moments", geo.M, COUT_PAD, unique=True)
        emit_gemm(plan, mom, self.q_w, COUT_PAD, COUT_PAD, self.out_rows, bias=pk.vec("quant_conv.bias"))
        self.out_geo = geo
        pk.done()
        plan.materialize()
        self.stream = torch.cuda.Stream(device=self.device)

    @torch.no_grad()
    def forward(self, x):
        n, c, H, W = x.shape
        assert (n, H, W) == (self.n, self.H, self.W) and c == self.cfg["in_channels"]
        cur = torch.cuda.current_stream(self.device)
        x32 = x.detach().to(self.device, torch.float32).contiguous()
        g, lc = self.out_geo, self.cfg["latent_channels"]
        out = torch.empty(n, 2 * lc, 1, g.H, g.W, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            hip.ncfhw_to_rows(x32.data_ptr(), n, c, 1, H, W, self.x_in.ptr, self.x_in.ld, CIN_PAD)
            self.plan.run()
            hip.rows_to_ncfhw(self.out_rows.ptr, self.out_rows.ld, n, 2 * lc, 1, g.H, g.W, out.data_ptr())
        cur.wait_stream(self.stream)
        x32.record_stream(self.stream)
        mean, logvar = out[:, :lc, 0], out[:, lc:, 0]
        return mean, logvar.clamp(-30.0, 20.0)

    @torch.no_grad()
    def forward_rows(self, fill, keep=None):
        """As forward, with the pixel rows written by `fill(self.x_in)` on the plan's stream (rcdms_amd.image.FrameTransform
        with rows=True) instead of converted from an fp32 tensor; keep: the device tensor `fill` reads."""
        n, H, W = self.n, self.H, self.W
        cur = torch.cuda.current_stream(self.device)
        g, lc = self.out_geo, self.cfg["latent_channels"]
        out = torch.empty(n, 2 * lc, 1, g.H, g.W, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            fill(self.x_in)
            self.plan.run()
            hip.rows_to_ncfhw(self.out_rows.ptr, self.out_rows.ld, n, 2 * lc, 1, g.H, g.W, out.data_ptr())
        cur.wait_stream(self.stream)
        if keep is not None:
            keep.record_stream(self.stream)
        mean, logvar = out[:, :lc, 0], out[:, lc:, 0]
        return mean, logvar.clamp(-30.0, 20.0)


def _emit_mid_block(plan, pk, m, cur, nxt, geo, groups):
    """UNetMidBlock2D: resnet, one-head attention, resnet; ping-pongs between the two buffers, returns the result."""
    _emit_resnet2d(plan, _pack_resnet(pk, m + "resnets.0."), cur, geo, nxt, groups)
    cur, nxt = nxt, cur
    _emit_mid_attention(plan, pk, m + "attentions.0.", cur, geo, nxt, groups)
    cur, nxt = nxt, cur
    _emit_resnet2d(plan, _pack_resnet(pk, m + "resnets.1."), cur, geo, nxt, groups)
    return nxt


SCORES_MAX_TOKENS = 4096    # rcdm_softmax_rows: columns of one row
FLASH_NARROW_MAX = 160      # rcdm_flash_attn: head dims up to here in steps of 8 ...
FLASH_WIDE_MAX = 512        # ... and up to here in steps of 64


def flash_head_ok(C):
    """Whether rcdm_flash_attn takes a head of C channels."""
    return C % 8 == 0 and (C <= FLASH_NARROW_MAX or (C <= FLASH_WIDE_MAX and C % 64 == 0))


def mid_attention_form(hw, C, switch=None):
    """Which form the one-head mid-block attention over hw latent pixels of C channels takes: "scores" (per image Q K^T
    GEMM -> rcdm_softmax_rows -> P V GEMM through an hw x hw score buffer) or "flash" (one rcdm_flash_attn launch over
    all images, nothing of size hw^2).  switch: RCDM_VAE_FLASH ("auto" / "1" / "0"; default: the process's setting).
    Raises NotImplementedError for a size no permitted form covers."""
    switch = SW.VAE_FLASH if switch is None else str(switch)
    scores_ok = hw <= SCORES_MAX_TOKENS and hw % 8 == 0
    if switch == "0" or (switch != "1" and hw <= SCORES_MAX_TOKENS):
        if not scores_ok:
            raise NotImplementedError(f"mid-block attention over {hw} tokens: rcdm_softmax_rows holds rows of <= 4096")
        return "scores"
    if not flash_head_ok(C):
        raise NotImplementedError(f"mid-block attention over {hw} tokens of {C} channels: rcdm_flash_attn takes one head of "
                                  f"<= {FLASH_NARROW_MAX} channels (multiples of 8) or <= {FLASH_WIDE_MAX} (multiples of 64)"
                                  + ("" if hw > SCORES_MAX_TOKENS else "; unset RCDM_VAE_FLASH for the score-buffer form"))
    return "flash"


def _emit_mid_attention(plan, pk, p, x, geo, out, groups):
    C, n, hw = x.C, geo.n_img, geo.hw
    form = mid_attention_form(hw, C)
    a = plan.rows("norm", geo.M, C)
    emit_groupnorm(plan, x, n, hw, pk.vec(p + "group_norm.weight"), pk.vec(p + "group_norm.bias"), 1e-6, False, a, groups)
    wo = pk.mat_f16(p + "to_out.0.weight")
    # softmax rows sum to one, so P (V0 + 1 bv^T) = P V0 + bv: the value bias moves into the output projection
    bo = (pk.vec(p + "to_out.0.bias") + hip.matmul_f32(pk.f32(p + "to_out.0.weight"), pk.vec(p + "to_v.bias"))).contiguous()
    ao = plan.rows("vae_ao", geo.M, C, unique=True)
    if form == "flash":
        # one [q | k | v] GEMM (N = 3C; any row count), then ONE launch: batch = images, one head of C channels read as
        # column views of the 3C-wide rows.  No V^T, no score buffer, no per-image loop
        wqkv = pk.mat_f16(p + "to_q.weight", p + "to_k.weight", p + "to_v.weight")
        bqkv = torch.cat([pk.vec(p + "to_q.bias"), pk.vec(p + "to_k.bias"), torch.zeros(C, device=plan.device)]).contiguous()
        qkv = plan.rows("vae_qkv", geo.M, 3 * C, unique=True)
        emit_gemm(plan, a, wqkv, 3 * C, C, qkv, bias=bqkv)
        emit_flash_attn(plan, qkv.cols(0, C), qkv.cols(C, C), qkv.cols(2 * C, C), n, 1, hw, hw, C, ao)
        emit_gemm(plan, ao, wo, C, C, out, bias=bo, residual=x)
        return
    wq, bq = pk.mat_f16(p + "to_q.weight"), pk.vec(p + "to_q.bias")
    wk, bk = pk.mat_f16(p + "to_k.weight"), pk.vec(p + "to_k.bias")
    wv = pk.mat_f16(p + "to_v.weight")
    q = plan.rows("vae_q", geo.M, C, unique=True)
    k = plan.rows("vae_k", geo.M, C, unique=True)
    emit_gemm(plan, a, wq, C, C, q, bias=bq)
    emit_gemm(plan, a, wk, C, C, k, bias=bk)
    vt = plan.rows("vae_vt", C, hw, unique=True)           # V^T of ONE image: [C][hw]
    sc = plan.rows("vae_scores", hw, hw, unique=True)      # scores / probabilities of one image
    wv_rows = Rows(_Holder16(wv), 0, C, C, C)
    scale = float(C) ** -0.5
    for i in range(n):
        img = lambda r: Rows(r.buf, r.off + i * hw * r.ld, hw, r.C, r.ld)
        a_i = _TensorLike(img(a))
        # V^T = Wv a_i^T : a GEMM whose "activation" rows are the weight rows and whose "weights" are the image's tokens
        emit_gemm(plan, wv_rows, a_i, hw, C, vt)
        emit_gemm(plan, img(q), _TensorLike(img(k)), hw, C, sc, scale=scale)
        plan.add(lambda sc=sc: hip.softmax_rows(hw, hw, sc.ld, sc.ld, 1.0, sc.ptr, sc.ptr), f"softmax_rows M={hw} N={hw}")
        emit_gemm(plan, sc, _TensorLike(vt), C, hw, img(ao))
    emit_gemm(plan, ao, wo, C, C, out, bias=bo, residual=x)
    plan.keep += [wv]


class _Holder16:
    """Adapter: a packed f16 weight tensor seen as a plan buffer (so it can be the A operand of emit_gemm)."""

    def __init__(self, t):
        self.t = t


class _TensorLike:
    """Adapter: rows of a plan buffer seen as a weight tensor (data_ptr()), for GEMMs between two activations."""

    def __init__(self, rows):
        self.rows = rows
        if rows.ld != rows.C:
            raise ValueError("a GEMM weight operand must be dense rows")

    def data_ptr(self):
        return self.rows.ptr
