"""CLIP text and vision encoders on the HIP path: the modules that produce the inputs of both stages.

Replaces the caller's `transformers` modules — the stage-2 text encoder (SD-1.5 CLIPTextModel: 768 wide, 12 layers, 12 x 64,
quick_gelu, causal; stage2_batchtest_rcdms_model.py:207-216, RCDMs_pipeline.py:_encode_prompt), the image encoder of both
stages (Kandinsky-2.2 CLIP-bigG vision: 1664 wide, 48 layers, 16 heads x 104, erf gelu, 224^2 / patch 14, projection 1280;
stage2...:200,290, stage1...:106,157-224) and the stage-1 text encoder (CLIP-bigG text, 1280 wide, 32 layers, 20 x 64;
stage1...:111-120) — restated from the published architecture of transformers' CLIPTextModelWithProjection /
CLIPVisionModelWithProjection.  transformers is third party and not vendored (the reference pins 4.40.0): PARITY UNPINNED by
any reference test; tests/golden/clip_*.npz are minted from transformers itself by tools/mint_clip_golden.py.

`CLIPTextEncoder` / `CLIPVisionEncoder` hold the fp32 parameters under the transformers state-dict key names, so a real
checkpoint loads with `load_state_dict` (`*.position_ids` buffers are ignored) and `from_transformers(module)` converts the
driver's module after its `resize_token_embeddings` / position-table resize.  They are call-compatible with what the two
pipelines do with their encoders.  A forward is a static launch plan over librcdm_hip.so in the manner of prior.py,
built per input shape and cached; the f16 weights are packed once and shared by every shape's plan:

  text    rcdm_embed_tokens -> per layer [LayerNorm -> fused [q;k;v] GEMM (+bias) -> rcdm_flash_attn_masked(causal) -> out_proj
          (+bias, +residual) -> LayerNorm -> fc1 (+bias, quick-GELU | GELU epilogue) -> fc2 (+bias, +residual)] -> final_layer_norm
          over all rows (= last_hidden_state); text_embeds = text_projection of the normed row at the pooling position
          (host-computed index: argmax of the ids for the legacy eos_token_id == 2 configs, else the first eos token).
  vision  rcdm_patch_rows -> ONE GEMM over all B * 257 rows against the zero-padded [C][592] patch weight whose residual
          operand is the position table (+ class embedding in row 0: class rows multiply zeros) -> pre_layrnorm -> the same
          layers with unmasked flash attention (head dim 104: the DS = 7 instantiation) -> last_hidden_state = the residual
          stream WITHOUT post_layernorm (what transformers returns and stage 2 consumes); image_embeds =
          visual_projection(post_layernorm(row 0)).

Every attention launch carries RCDM_ATTN_WIDE_RANGE unconditionally: the planner's weight-norm score bound
(packer.attn_score_bound) is written for the UNet's key names and these launches are not in a timed loop.  No CPU path:
hip.RcdmError without a GPU."""
import types

import torch
from torch import nn

from . import hip
from .engine import Packer, Plan, Rows, _NS, emit_flash_attn, emit_flash_attn_masked, emit_gemm, emit_layernorm
from .tokenizer import ClipTokenizer

_ACTS = ("quick_gelu", "gelu")
TEXT_DEFAULTS = dict(vocab_size=49408, hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072,
                     max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=2, projection_dim=768,
                     layer_norm_eps=1e-5)
VISION_DEFAULTS = dict(hidden_size=1664, num_attention_heads=16, num_hidden_layers=48, intermediate_size=8192, image_size=224,
                       patch_size=14, num_channels=3, hidden_act="gelu", projection_dim=1280, layer_norm_eps=1e-5)


def pooling_index(input_ids, eos_token_id):
    """Row position whose normed state is pooled (transformers CLIPTextTransformer.forward): the largest id for the legacy
    eos_token_id == 2 configs (SD-1.5), otherwise the first position holding eos_token_id.  Host tensor in, host tensor out."""
    ids = input_ids.detach().cpu().long()
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def tokenizer_keywords(tokenizer, text_encoder, tok):
    """What a pipeline's _encode_prompt adds to its text-encoder call: the device-side pooling index and the waiver of the id
    range check when the ids come from a ClipTokenizer and go to a CLIPTextEncoder, nothing for any other pair (the caller's
    transformers objects, the tests' stubs).  The waiver is earned here: every id a ClipTokenizer emits is below its len(), so a
    tokenizer that outgrew the embedding table (add_tokens without resizing it) is a ValueError, not an unchecked gather."""
    if not (isinstance(tokenizer, ClipTokenizer) and isinstance(text_encoder, CLIPTextEncoder)):
        return {}
    if len(tokenizer) > text_encoder.cfg["vocab_size"]:
        raise ValueError(f"the tokenizer holds {len(tokenizer)} tokens, the text encoder's embedding table "
                         f"{text_encoder.cfg['vocab_size']} rows: resize the table after add_tokens")
    return dict(pool_index=tok.pool_index, ids_checked=True)


class ClipOutput(dict):
    """What a forward returns: answers both `.name` and `["name"]` (the pipelines use either)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


# ---- parameter holders (transformers key names) ---------------------------------------------------------------------------
class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(C, C) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, C, inter):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, inter), nn.Linear(inter, C)


class _Layer(nn.Module):
    def __init__(self, C, inter, eps):
        super().__init__()
        self.self_attn = _Attention(C)
        self.layer_norm1 = nn.LayerNorm(C, eps=eps)
        self.mlp = _MLP(C, inter)
        self.layer_norm2 = nn.LayerNorm(C, eps=eps)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList(_Layer(cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"])
                                    for _ in range(cfg["num_hidden_layers"]))


class _TextEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])


class _TextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _TextEmbeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


class _VisionEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        C, p = cfg["hidden_size"], cfg["patch_size"]
        self.class_embedding = nn.Parameter(torch.zeros(C))
        self.patch_embedding = nn.Conv2d(cfg["num_channels"], C, p, stride=p, bias=False)
        self.position_embedding = nn.Embedding((cfg["image_size"] // p) ** 2 + 1, C)


class _VisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = _VisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])   # (transformers' spelling: the key)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


def _check_cfg(cfg):
    if cfg["hidden_act"] not in _ACTS:
        raise NotImplementedError(f"hidden_act {cfg['hidden_act']!r}: the GEMM epilogues cover {_ACTS}")
    C, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    if C % heads or (C // heads) % 8 or C % 8 or cfg["intermediate_size"] % 8 or C > 2048:
        raise ValueError(f"hidden_size {C} / heads {heads}: the kernels need head dim % 8 == 0 and a LayerNorm width <= 2048")


class _Encoder16(nn.Module):
    """Shared by the two encoders: device / dtype, the state-dict rules, the packed-weight and per-shape plan caches."""

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict(_normalise_keys(state_dict, self.PREFIX), strict=strict, **kw)

    def _weights(self, pack):
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, pack(self.cfg, {k: v for k, v in self.state_dict().items()}, self.device))
            self._programs = {}
        return self._packed[1]

    def weight_bytes_f16(self):
        """Bytes of the f16 matrices one forward streams (the weight-read floor of tools/bench_clip.py)."""
        return 2 * sum(p.numel() for n, p in self.named_parameters() if p.dim() >= 2 and "embedding" not in n)


def _normalise_keys(sd, prefix):
    """A transformers CLIP state dict under the key names of the 4.x releases: `*.position_ids` (a persistent buffer there)
    dropped, and the tower prefix ("text_model." / "vision_model.") restored where a later release's projection-less class
    (CLIPTextModel, CLIPVisionModel) saves its keys without it."""
    out = {}
    for k, v in sd.items():
        if k.endswith("position_ids"):
            continue
        if not k.startswith(prefix) and k.split(".")[0] not in ("text_projection", "visual_projection"):
            k = prefix + k
        out[k] = v
    return out


def _copy_from_transformers(cls, hf, **kw):
    sd = _normalise_keys(hf.state_dict(), cls.PREFIX)
    c = hf.config.to_dict() if hasattr(hf.config, "to_dict") else dict(vars(hf.config))
    m = cls({k: c[k] for k in cls.DEFAULTS if k in c and c[k] is not None}, _sd=sd, **kw)
    m.load_state_dict(sd)
    return m


class CLIPTextEncoder(_Encoder16):
    """transformers CLIPTextModel / CLIPTextModelWithProjection (with_projection) as a parameter holder + HIP forward.
    `enc(input_ids)` -> ClipOutput(last_hidden_state (B, L, C) fp32, text_embeds (B, projection_dim) fp32 | None,
    pooler_output (B, C), hidden_states None)."""
    DEFAULTS, PREFIX = TEXT_DEFAULTS, "text_model."

    def __init__(self, config=None, with_projection=True, _sd=None):
        super().__init__()
        self.cfg = dict(TEXT_DEFAULTS)
        self.cfg.update(config or {})
        if _sd is not None:   # from_transformers: the tables as the driver resized them, whatever the config still says
            self.cfg["vocab_size"], self.cfg["hidden_size"] = _sd["text_model.embeddings.token_embedding.weight"].shape
            self.cfg["max_position_embeddings"] = _sd["text_model.embeddings.position_embedding.weight"].shape[0]
            with_projection = "text_projection.weight" in _sd
            if with_projection:
                self.cfg["projection_dim"] = _sd["text_projection.weight"].shape[0]
        _check_cfg(self.cfg)
        self.config = types.SimpleNamespace(**self.cfg)
        self.text_model = _TextTransformer(self.cfg)
        if with_projection:
            self.text_projection = nn.Linear(self.cfg["hidden_size"], self.cfg["projection_dim"], bias=False)
        self.with_projection = bool(with_projection)
        self._packed, self._programs = None, {}

    @classmethod
    def from_transformers(cls, hf_module):
        return _copy_from_transformers(cls, hf_module)

    @property
    def max_position_embeddings(self):
        return self.text_model.embeddings.position_embedding.weight.shape[0]

    def check_shape(self, input_ids):
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"input_ids must be an integer (B, L) tensor, got {tuple(input_ids.shape)} {input_ids.dtype}")
        B, L = input_ids.shape
        if B < 1 or L < 1 or L > self.max_position_embeddings:
            raise ValueError(f"sequence length {L} outside the position table ({self.max_position_embeddings} rows)")

    def check_ids(self, input_ids):
        """The host-side guard of rcdm_embed_tokens (the kernel clamps nothing): ValueError before any launch."""
        self.check_shape(input_ids)
        ids = input_ids.detach().cpu()
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= self.cfg["vocab_size"]:
            raise ValueError(f"input_ids in [{lo}, {hi}] outside the vocabulary [0, {self.cfg['vocab_size']})")
        return ids

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, output_attentions=None,
                output_hidden_states=None, return_dict=True, pool_index=None, ids_checked=False, **_):
        """pool_index: device int (B, 2) — per row the position of the largest id and of the first eos, what ClipTokenizer
        returns — in place of the host-computed pooling index.  ids_checked=True: the caller vouches that every id lies inside
        the vocabulary (a ClipTokenizer whose len() fits the embedding table), so the range check's device -> host copy is
        skipped.  With both, a forward waits for nothing.  With neither, exactly the path as it was."""
        if ids_checked:
            self.check_shape(input_ids)
            ids = None
        else:
            ids = self.check_ids(input_ids)
        if pool_index is not None and (pool_index.device != input_ids.device or tuple(pool_index.shape) != (input_ids.shape[0], 2)
                                       or pool_index.dtype not in (torch.int32, torch.int64)):
            raise ValueError(f"pool_index must be an integer (B, 2) tensor on the ids' device, got {tuple(pool_index.shape)} "
                             f"{pool_index.dtype} on {pool_index.device}")
        if self.device.type != "cuda" or input_ids.device.type != "cuda":
            raise hip.RcdmError(f"CLIPTextEncoder runs on the HIP path only (module on {self.device}, ids on {input_ids.device})")
        if attention_mask is not None or position_ids is not None:
            raise NotImplementedError("the pipelines pass input_ids only (causal mask, positions 0 .. L-1)")
        w = self._weights(pack_text)
        shape = tuple(input_ids.shape)
        prog = self._programs.get(shape)
        if prog is None:
            prog = self._programs[shape] = ClipTextProgram(self.cfg, w, shape[0], shape[1], self.device)
        if pool_index is not None:
            pool = pool_index[:, 0 if self.cfg["eos_token_id"] == 2 else 1]
        else:
            pool = pooling_index(input_ids if ids is None else ids, self.cfg["eos_token_id"])
        last, pooled, emb = prog.forward(input_ids, pool)
        out = ClipOutput(last_hidden_state=last, pooler_output=pooled, text_embeds=emb, hidden_states=None, attentions=None)
        return out if return_dict else (emb, last) if emb is not None else (last, pooled)


class CLIPVisionEncoder(_Encoder16):
    """transformers CLIPVisionModelWithProjection as a parameter holder + HIP forward.  `enc(pixel_values)` ->
    ClipOutput(last_hidden_state (B, 1 + P, C) fp32 — the residual stream, no post_layernorm —, image_embeds
    (B, projection_dim) fp32 | None, hidden_states None)."""
    DEFAULTS, PREFIX = VISION_DEFAULTS, "vision_model."

    def __init__(self, config=None, with_projection=True, _sd=None):
        super().__init__()
        self.cfg = dict(VISION_DEFAULTS)
        self.cfg.update(config or {})
        if _sd is not None:
            with_projection = "visual_projection.weight" in _sd
            if with_projection:
                self.cfg["projection_dim"] = _sd["visual_projection.weight"].shape[0]
        _check_cfg(self.cfg)
        if self.cfg["num_channels"] != 3 or self.cfg["image_size"] % self.cfg["patch_size"]:
            raise ValueError("RGB images whose side is a multiple of the patch size")
        self.config = types.SimpleNamespace(**self.cfg)
        self.vision_model = _VisionTransformer(self.cfg)
        if with_projection:
            self.visual_projection = nn.Linear(self.cfg["hidden_size"], self.cfg["projection_dim"], bias=False)
        self.with_projection = bool(with_projection)
        self._packed, self._programs = None, {}

    @classmethod
    def from_transformers(cls, hf_module):
        return _copy_from_transformers(cls, hf_module)

    @torch.no_grad()
    def forward(self, pixel_values=None, output_attentions=None, output_hidden_states=None, return_dict=True, **_):
        S = self.cfg["image_size"]
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)}: expected (B, 3, {S}, {S})")
        if self.device.type != "cuda" or pixel_values.device.type != "cuda":
            raise hip.RcdmError(f"CLIPVisionEncoder runs on the HIP path only (module on {self.device}, pixels on "
                                f"{pixel_values.device})")
        w = self._weights(pack_vision)
        B = pixel_values.shape[0]
        prog = self._programs.get(B)
        if prog is None:
            prog = self._programs[B] = ClipVisionProgram(self.cfg, w, B, self.device)
        last, emb = prog.forward(pixel_values)
        out = ClipOutput(last_hidden_state=last, image_embeds=emb, hidden_states=None, attentions=None)
        return out if return_dict else (emb, last)


# ---- packed weights -------------------------------------------------------------------------------------------------------
def _pack_layers(pk, p, n):
    layers = []
    for i in range(n):
        q = p + f"encoder.layers.{i}."
        a = q + "self_attn."
        w = _NS()
        w.ln1 = (pk.vec(q + "layer_norm1.weight"), pk.vec(q + "layer_norm1.bias"))
        w.ln2 = (pk.vec(q + "layer_norm2.weight"), pk.vec(q + "layer_norm2.bias"))
        w.qkv = pk.mat_f16(a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight")
        w.qkv_b = torch.cat([pk.vec(a + f"{n_}_proj.bias") for n_ in "qkv"]).contiguous()
        w.o, w.o_b = pk.mat_f16(a + "out_proj.weight"), pk.vec(a + "out_proj.bias")
        w.fc1, w.fc1_b = pk.mat_f16(q + "mlp.fc1.weight"), pk.vec(q + "mlp.fc1.bias")
        w.fc2, w.fc2_b = pk.mat_f16(q + "mlp.fc2.weight"), pk.vec(q + "mlp.fc2.bias")
        layers.append(w)
    return layers


def pack_text(cfg, sd, device):
    hip.load()
    pk = Packer(sd, device)
    p = "text_model."
    w = _NS(layers=_pack_layers(pk, p, cfg["num_hidden_layers"]))
    w.table = pk.f32(p + "embeddings.token_embedding.weight")
    w.pos = pk.f32(p + "embeddings.position_embedding.weight")
    w.ln_f = (pk.vec(p + "final_layer_norm.weight"), pk.vec(p + "final_layer_norm.bias"))
    w.proj = pk.mat_f16("text_projection.weight") if pk.has("text_projection.weight") else None
    pk.done()
    return w


def pack_vision(cfg, sd, device):
    hip.load()
    pk = Packer(sd, device)
    p = "vision_model."
    w = _NS(layers=_pack_layers(pk, p, cfg["num_hidden_layers"]))
    C, K = cfg["hidden_size"], 3 * cfg["patch_size"] ** 2
    w.ldk = (K + 7) // 8 * 8
    pw = torch.zeros(C, w.ldk, dtype=torch.float32, device=pk.device)
    pw[:, :K] = pk.f32(p + "embeddings.patch_embedding.weight").reshape(C, K)      # the weight's own (c, ky, kx) order
    w.patch = torch.empty(C, w.ldk, dtype=torch.float16, device=pk.device)
    hip.pack_f16(pw.data_ptr(), w.patch.data_ptr(), pw.numel())
    pk._tmp.append(pw)
    # the patch GEMM's residual operand, one image's worth: position table, class embedding added to row 0 (fp32, one rounding)
    pos = pk.f32(p + "embeddings.position_embedding.weight").clone()
    pos[0] += pk.f32(p + "embeddings.class_embedding")
    w.postab = torch.empty(pos.shape, dtype=torch.float16, device=pk.device)
    hip.pack_f16(pos.data_ptr(), w.postab.data_ptr(), pos.numel())
    pk._tmp.append(pos)
    w.ln_pre = (pk.vec(p + "pre_layrnorm.weight"), pk.vec(p + "pre_layrnorm.bias"))
    w.ln_post = (pk.vec(p + "post_layernorm.weight"), pk.vec(p + "post_layernorm.bias"))
    w.proj = pk.mat_f16("visual_projection.weight") if pk.has("visual_projection.weight") else None
    pk.done()
    return w


# ---- launch plans ---------------------------------------------------------------------------------------------------------
def _emit_layers(plan, cfg, layers, tok, B, L, causal):
    """The transformer stack on the residual stream `tok` ((b l) rows of C), in place."""
    C, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    dh, inter, eps = C // heads, cfg["intermediate_size"], cfg["layer_norm_eps"]
    quick = cfg["hidden_act"] == "quick_gelu"
    M = B * L
    a = plan.rows("norm", M, C)
    for w in layers:
        emit_layernorm(plan, tok, w.ln1[0], w.ln1[1], a, eps=eps)
        qkv = plan.rows("qkv", M, 3 * C)
        emit_gemm(plan, a, w.qkv, 3 * C, C, qkv, bias=w.qkv_b)
        ao = plan.rows("attn_out", M, C)
        q, k, v = qkv.cols(0, C), qkv.cols(C, C), qkv.cols(2 * C, C)
        if causal:
            emit_flash_attn_masked(plan, q, k, v, B, heads, L, L, dh, ao, None, True, wide=True)
        else:
            emit_flash_attn(plan, q, k, v, B, heads, L, L, dh, ao, wide=True)
        emit_gemm(plan, ao, w.o, C, C, tok, bias=w.o_b, residual=tok)
        emit_layernorm(plan, tok, w.ln2[0], w.ln2[1], a, eps=eps)
        hid = plan.rows("mlp", M, inter)
        emit_gemm(plan, a, w.fc1, inter, C, hid, bias=w.fc1_b, gelu=not quick, quick_gelu=quick)
        emit_gemm(plan, hid, w.fc2, C, inter, tok, bias=w.fc2_b, residual=tok)


def _rows_view(rows, M, C):
    """(M, C) f16 tensor view of a dense Rows."""
    return rows.buf.t[:M * C * 2].view(torch.float16).view(M, C)


class ClipTextProgram:
    """Launch plan of one CLIP text forward for a fixed (B, L)."""

    def __init__(self, cfg, w, B, L, device):
        hip.load()
        self.cfg, self.w, self.B, self.L = cfg, w, B, L
        self.device = torch.device(device)
        C = self.C = cfg["hidden_size"]
        M = B * L
        if L > w.pos.shape[0]:
            raise ValueError(f"sequence length {L} outside the position table ({w.pos.shape[0]} rows)")
        self.ids = torch.zeros(M, dtype=torch.int32, device=self.device)
        self.plan = plan = Plan(self.device)
        tok = plan.rows("clip_tok", M, C, unique=True)
        vocab = w.table.shape[0]
        plan.add(lambda: hip.embed_tokens(self.ids.data_ptr(), M, L, w.table.data_ptr(), vocab, w.pos.data_ptr(), C, tok.ptr,
                                          tok.ld), f"embed_tokens M={M} C={C}")
        plan.n_launch += 1
        _emit_layers(plan, cfg, w.layers, tok, B, L, causal=True)
        self.out = plan.rows("clip_last", M, C, unique=True)
        emit_layernorm(plan, tok, w.ln_f[0], w.ln_f[1], self.out, eps=cfg["layer_norm_eps"])
        plan.keep += [w]
        plan.materialize()
        self.pool16 = torch.zeros(B, C, dtype=torch.float16, device=self.device)
        self.P = w.proj.shape[0] if w.proj is not None else 0
        if self.P:
            self.emb16 = torch.zeros(B, self.P, dtype=torch.float16, device=self.device)
            self._d_proj = hip.GemmDesc(B, self.P, C, C, self.P, 0, 0, 1, 0, 1.0, 0)
            self._ws = torch.zeros(max(hip.gemm_workspace_bytes(self._d_proj), 256), dtype=torch.uint8, device=self.device)

    def forward(self, input_ids, pool_idx):
        """input_ids: device (B, L) integers, already range-checked; pool_idx: (B,) positions, on the host or (ClipTokenizer's)
        on the device.  -> fp32 device tensors
        (last_hidden_state (B, L, C), pooled (B, C), text_embeds (B, P) | None)."""
        B, L, C = self.B, self.L, self.C
        self.ids.copy_(input_ids.reshape(-1))
        self.plan.run()
        last16 = _rows_view(self.out, B * L, C)
        if pool_idx.is_cuda:
            flat = torch.arange(B, device=self.device) * L + pool_idx.long()
        else:
            flat = (torch.arange(B) * L + pool_idx).to(self.device)
        torch.index_select(last16, 0, flat, out=self.pool16)       # plumbing (M = B): the pooled rows, gathered by position
        emb = None
        if self.P:
            hip.gemm(self._d_proj, self.pool16.data_ptr(), self.w.proj.data_ptr(), 0, 0, 0, self.emb16.data_ptr(),
                     self._ws.data_ptr(), self._ws.numel())
            emb = self.emb16.float()
        return last16.float().view(B, L, C), self.pool16.float(), emb


class ClipVisionProgram:
    """Launch plan of one CLIP vision forward for a fixed batch B."""

    def __init__(self, cfg, w, B, device):
        hip.load()
        self.cfg, self.w, self.B = cfg, w, B
        self.device = torch.device(device)
        C = self.C = cfg["hidden_size"]
        S, patch = cfg["image_size"], cfg["patch_size"]
        T = self.T = (S // patch) ** 2 + 1
        if w.postab.shape[0] != T:
            raise ValueError(f"position table holds {w.postab.shape[0]} rows, a {S}x{S} image has {T} tokens")
        M = B * T
        self.pix = torch.zeros(B, 3, S, S, dtype=torch.float32, device=self.device)
        self.res = w.postab.repeat(B, 1).contiguous()               # row b T + j = pos[j] (+ class embedding for j = 0)
        self.plan = plan = Plan(self.device)
        prow = plan.rows("clip_patch", M, w.ldk, unique=True)
        plan.add(lambda: hip.patch_rows(self.pix.data_ptr(), B, S, S, patch, prow.ptr, prow.ld), f"patch_rows B={B} {S}x{S}")
        plan.n_launch += 1
        res_buf = types.SimpleNamespace(t=self.res.view(torch.uint8).view(-1))
        emb = plan.rows("clip_emb", M, C, unique=True)
        emit_gemm(plan, prow, w.patch, C, w.ldk, emb, residual=Rows(res_buf, 0, M, C, C))
        tok = self.tok = plan.rows("clip_tok", M, C, unique=True)
        emit_layernorm(plan, emb, w.ln_pre[0], w.ln_pre[1], tok, eps=cfg["layer_norm_eps"])
        _emit_layers(plan, cfg, w.layers, tok, B, T, causal=False)
        self.P = w.proj.shape[0] if w.proj is not None else 0
        if self.P:
            cls = Rows(tok.buf, tok.off, B, C, T * C)               # row 0 of every image
            fin = plan.rows("clip_fin", B, C, unique=True)
            emit_layernorm(plan, cls, w.ln_post[0], w.ln_post[1], fin, eps=cfg["layer_norm_eps"])
            self.emb = plan.rows("clip_embeds", B, self.P, unique=True)
            emit_gemm(plan, fin, w.proj, self.P, C, self.emb)
        plan.keep += [w, self.res]
        plan.materialize()

    def forward(self, pixel_values):
        """pixel_values: device (B, 3, S, S).  -> fp32 device tensors (last_hidden_state (B, T, C), image_embeds (B, P) | None)."""
        B, T, C = self.B, self.T, self.C
        self.pix.copy_(pixel_values)
        self.plan.run()
        emb = _rows_view(self.emb, B, self.P).float() if self.P else None
        return _rows_view(self.tok, B * T, C).float().view(B, T, C), emb
