"""Independent pin for the transformer extractors (vit_s_32, vit_b_32, vit_b_32_clip).

The reference builds timm 0.6.12 `vit_small_patch32_224_in21k`, `vit_base_patch32_224_in21k` and
`vit_base_patch32_224_clip_laion2b` with num_classes=0 (reference `model/feature_extractors.py:49-63`); timm is not
installed offline. Hugging Face `transformers` is, and carries independently written `ViTModel` and `CLIPVisionModel`. This
module holds two pieces:

  * `hf_state_dict(name, timm_sd)`: a timm-keyed state_dict re-keyed for the HF model (transformers 5.x key names; q / k / v
    split out of `attn.qkv`, CLIP's `class_embedding` / `position_embedding` from `cls_token` / `pos_embed`), and
    `hf_model(name)` building that model offline with the timm hyper-parameters. The arithmetic of the comparison values is then entirely transformers' code.
  * `TimmViT(name)`: a small CPU restatement of the timm forward in timm's module layout (state_dict keys, FiLM slot names),
    injectable as `OracleRecogniser.fe`. tests/test_vit_host.py pins it to the HF models.

timm 0.6.12 details this rests on (vision_transformer.py): the class token is prepended before `+ pos_embed`; `norm_pre`
exists only with `pre_norm=True` (the CLIP model, whose patch embedding then has no bias); qkv is
`reshape(B, N, 3, heads, 64)`; the attention scale is 64 ** -0.5; `nn.GELU()` is the erf form; the feature is
`norm(x)[:, 0]` (global_pool='token', fc_norm and head are Identity at num_classes=0); LayerNorm eps is 1e-6 for the in21k
models and 1e-5 (nn.LayerNorm) for CLIP.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

VIT = {  # name: (D, heads, eps, clip)
    "vit_s_32": (384, 6, 1e-6, False),
    "vit_b_32": (768, 12, 1e-6, False),
    "vit_b_32_clip": (768, 12, 1e-5, True),
}
DEPTH = 12
TOKENS = 50


class _Attention(nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(D, 3 * D)
        self.proj = nn.Linear(D, D)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        attn = ((q @ k.transpose(-2, -1)) * (C // self.heads) ** -0.5).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


class _Mlp(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.fc1 = nn.Linear(D, 4 * D)
        self.fc2 = nn.Linear(4 * D, D)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, D, heads, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(D, eps=eps)
        self.attn = _Attention(D, heads)
        self.norm2 = nn.LayerNorm(D, eps=eps)
        self.mlp = _Mlp(D)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class _PatchEmbed(nn.Module):
    def __init__(self, D, bias):
        super().__init__()
        self.proj = nn.Conv2d(3, D, 32, 32, bias=bias)


class TimmViT(nn.Module):
    """timm VisionTransformer forward (num_classes=0) in timm's parameter layout."""

    def __init__(self, name):
        super().__init__()
        D, heads, eps, clip = VIT[name]
        self.output_size = D
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, TOKENS, D))
        self.patch_embed = _PatchEmbed(D, bias=not clip)
        self.norm_pre = nn.LayerNorm(D, eps=eps) if clip else None
        self.blocks = nn.Sequential(*[_Block(D, heads, eps) for _ in range(DEPTH)])
        self.norm = nn.LayerNorm(D, eps=eps)

    def film_slot_names(self):
        """reference model/film.py:57-66: every LayerNorm named norm / norm1 / norm2 (not norm_pre), module order."""
        return [n for n, m in self.named_modules() if isinstance(m, nn.LayerNorm) and n.split(".")[-1] in
                ("norm", "norm1", "norm2")]

    def forward(self, x):
        if x.dim() == 5:
            x = x.flatten(end_dim=1)
        x = self.patch_embed.proj(x).flatten(2).transpose(1, 2)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1) + self.pos_embed
        if self.norm_pre is not None:
            x = self.norm_pre(x)
        return self.norm(self.blocks(x))[:, 0]


# ---- Hugging Face counterparts --------------------------------------------------------------------------------------
def hf_model(name):
    """The HF model with the timm hyper-parameters, randomly initialised (offline), eval mode, eager attention."""
    D, heads, eps, clip = VIT[name]
    if clip:
        from transformers import CLIPVisionConfig, CLIPVisionModel
        cfg = CLIPVisionConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=DEPTH, num_attention_heads=heads,
                               image_size=224, patch_size=32, hidden_act="gelu", layer_norm_eps=eps, num_channels=3)
        cfg._attn_implementation = "eager"
        return CLIPVisionModel(cfg).eval()
    from transformers import ViTConfig, ViTModel
    cfg = ViTConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=DEPTH, num_attention_heads=heads,
                    image_size=224, patch_size=32, hidden_act="gelu", layer_norm_eps=eps, qkv_bias=True, num_channels=3)
    cfg._attn_implementation = "eager"
    return ViTModel(cfg, add_pooling_layer=False).eval()


def hf_features(name, model, frames):
    """The timm feature (final LayerNorm of the class token) from the HF model's own outputs."""
    if VIT[name][3]:
        return model(pixel_values=frames).pooler_output  # post_layernorm(last_hidden_state[:, 0])
    return model(pixel_values=frames).last_hidden_state[:, 0]


def hf_key_map(name):
    """timm key -> HF key, for every timm key except the q/k/v-concatenated `attn.qkv` ones (hf_state_dict splits those)."""
    D, heads, eps, clip = VIT[name]
    m = {}
    if clip:
        m.update({"patch_embed.proj.weight": "embeddings.patch_embedding.weight",
                  "norm_pre.weight": "pre_layrnorm.weight", "norm_pre.bias": "pre_layrnorm.bias",
                  "norm.weight": "post_layernorm.weight", "norm.bias": "post_layernorm.bias"})
        for i in range(DEPTH):
            h, t = "encoder.layers.%d." % i, "blocks.%d." % i
            for leaf in ("weight", "bias"):
                m[t + "norm1." + leaf] = h + "layer_norm1." + leaf
                m[t + "norm2." + leaf] = h + "layer_norm2." + leaf
                m[t + "attn.proj." + leaf] = h + "self_attn.out_proj." + leaf
                m[t + "mlp.fc1." + leaf] = h + "mlp.fc1." + leaf
                m[t + "mlp.fc2." + leaf] = h + "mlp.fc2." + leaf
        return m
    m.update({"cls_token": "embeddings.cls_token", "pos_embed": "embeddings.position_embeddings",
              "patch_embed.proj.weight": "embeddings.patch_embeddings.projection.weight",
              "patch_embed.proj.bias": "embeddings.patch_embeddings.projection.bias",
              "norm.weight": "layernorm.weight", "norm.bias": "layernorm.bias"})
    for i in range(DEPTH):
        h, t = "layers.%d." % i, "blocks.%d." % i
        for leaf in ("weight", "bias"):
            m[t + "norm1." + leaf] = h + "layernorm_before." + leaf
            m[t + "norm2." + leaf] = h + "layernorm_after." + leaf
            m[t + "attn.proj." + leaf] = h + "attention.o_proj." + leaf
            m[t + "mlp.fc1." + leaf] = h + "mlp.fc1." + leaf
            m[t + "mlp.fc2." + leaf] = h + "mlp.fc2." + leaf
    return m


def hf_state_dict(name, timm_sd):
    """timm-keyed state_dict -> the HF model's state_dict (tensors shared or split, no arithmetic)."""
    D, heads, eps, clip = VIT[name]
    out = {}
    for tk, hk in hf_key_map(name).items():
        out[hk] = timm_sd[tk]
    if clip:
        p = "embeddings."
        out[p + "class_embedding"] = timm_sd["cls_token"].reshape(D)
        out[p + "position_embedding.weight"] = timm_sd["pos_embed"].reshape(TOKENS, D)
    for i in range(DEPTH):
        w = timm_sd["blocks.%d.attn.qkv.weight" % i]
        b = timm_sd["blocks.%d.attn.qkv.bias" % i]
        if clip:
            names = ["encoder.layers.%d.self_attn.%s_proj" % (i, n) for n in ("q", "k", "v")]
        else:
            names = ["layers.%d.attention.%s_proj" % (i, n) for n in ("q", "k", "v")]
        for j, hk in enumerate(names):
            out[hk + ".weight"] = w[j * D:(j + 1) * D]
            out[hk + ".bias"] = b[j * D:(j + 1) * D]
    return out


def load_hf(name, model, timm_sd):
    """Load a timm-keyed state_dict into the HF model; every HF parameter must be covered (buffers such as CLIP's
    position_ids are left as built)."""
    sd = hf_state_dict(name, timm_sd)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    params = {k for k, _ in model.named_parameters()}
    assert not (params & set(missing)), sorted(params & set(missing))[:5]
    return model


def film_swap_hf(name, timm_film):
    """A timm-keyed FiLM dict ({slot}.weight / .bias) re-keyed for torch.func.functional_call on the HF model."""
    m = hf_key_map(name)
    return {m[k]: v for k, v in timm_film.items()}
