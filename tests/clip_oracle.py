"""Plain-torch fp32 restatement of the two CLIP forwards (transformers CLIPTextModelWithProjection /
CLIPVisionModelWithProjection) from a state dict with the transformers key names.  Test-only: the CPU tests pin it to the
goldens minted from transformers itself (tools/mint_clip_golden.py), the GPU tests use it where no golden exists."""
import torch
import torch.nn.functional as F


def _act(x, name):
    if name == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if name == "gelu":
        return F.gelu(x)
    raise ValueError(name)


def _layers(sd, p, x, cfg, causal):
    heads, eps = cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5)
    B, L, C = x.shape
    d = C // heads
    mask = torch.full((L, L), float("-inf")).triu(1) if causal else None
    for i in range(cfg["num_hidden_layers"]):
        q = p + f"encoder.layers.{i}."
        lin = lambda t, n: F.linear(t, sd[q + n + ".weight"], sd[q + n + ".bias"])
        h = F.layer_norm(x, (C,), sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"], eps)
        split = lambda t: t.reshape(B, L, heads, d).transpose(1, 2)
        s = split(lin(h, "self_attn.q_proj")) @ split(lin(h, "self_attn.k_proj")).transpose(-1, -2) * d ** -0.5
        if mask is not None:
            s = s + mask
        a = (s.softmax(-1) @ split(lin(h, "self_attn.v_proj"))).transpose(1, 2).reshape(B, L, C)
        x = x + lin(a, "self_attn.out_proj")
        h = F.layer_norm(x, (C,), sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"], eps)
        x = x + lin(_act(lin(h, "mlp.fc1"), cfg["hidden_act"]), "mlp.fc2")
    return x


def pooling_index(input_ids, eos_token_id):
    """Position of the pooled token: argmax of the ids for the legacy eos_token_id == 2 configs, else the first eos."""
    if eos_token_id == 2:
        return input_ids.argmax(dim=-1)
    return (input_ids == eos_token_id).int().argmax(dim=-1)


def text_forward(sd, cfg, input_ids):
    """-> (last_hidden_state (B, L, C), text_embeds (B, proj) or None)"""
    sd = {k: v.float() for k, v in sd.items()}
    B, L = input_ids.shape
    p = "text_model."
    x = sd[p + "embeddings.token_embedding.weight"][input_ids] + sd[p + "embeddings.position_embedding.weight"][:L]
    x = _layers(sd, p, x, cfg, causal=True)
    C = x.shape[-1]
    x = F.layer_norm(x, (C,), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], cfg.get("layer_norm_eps", 1e-5))
    emb = None
    if "text_projection.weight" in sd:
        pooled = x[torch.arange(B), pooling_index(input_ids, cfg.get("eos_token_id", 2))]
        emb = pooled @ sd["text_projection.weight"].t()
    return x, emb


def vision_forward(sd, cfg, pixel_values):
    """-> (last_hidden_state (B, T, C) WITHOUT post_layernorm, image_embeds (B, proj) or None)"""
    sd = {k: v.float() for k, v in sd.items()}
    p = "vision_model."
    eps = cfg.get("layer_norm_eps", 1e-5)
    B = pixel_values.shape[0]
    patches = F.conv2d(pixel_values.float(), sd[p + "embeddings.patch_embedding.weight"], stride=cfg["patch_size"])
    C = patches.shape[1]
    x = torch.cat([sd[p + "embeddings.class_embedding"].expand(B, 1, C), patches.flatten(2).transpose(1, 2)], dim=1)
    x = x + sd[p + "embeddings.position_embedding.weight"]
    x = F.layer_norm(x, (C,), sd[p + "pre_layrnorm.weight"], sd[p + "pre_layrnorm.bias"], eps)
    x = _layers(sd, p, x, cfg, causal=False)
    emb = None
    if "visual_projection.weight" in sd:
        pooled = F.layer_norm(x[:, 0], (C,), sd[p + "post_layernorm.weight"], sd[p + "post_layernorm.bias"], eps)
        emb = pooled @ sd["visual_projection.weight"].t()
    return x, emb
