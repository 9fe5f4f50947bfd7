"""Independent pin for the patch-16 transformer extractors (vit_s_16, vit_b_16, vit_b_16_clip).

The patch-16 members of the families tests/vit_pin.py pins: timm `vit_small_patch16_224_in21k`, `vit_base_patch16_224_in21k`
and the laion2b CLIP B/16, built with num_classes=0. The timm model names are given by analogy with the patch-32 ones the
reference names (`model/feature_extractors.py:49-63`); timm is not installed offline, so they cannot be checked here. What is
pinned is the architecture: timm's VisionTransformer with `patch_size=16` differs from the patch-32 model in the patch
convolution (`Conv2d(3, D, 16, 16)`), the position table (`[1, 197, D]`) and the token count (196 patches + the class token),
and in nothing else - blocks, FiLM slots, eps and the CLIP model's `norm_pre` / bias-free patch embedding are those of
tests/vit_pin.py, whose `_Block` is reused by import.

As there, two pieces: `TimmViT16(name)`, the CPU restatement in timm's parameter layout, and the Hugging Face counterparts
(`ViTConfig` / `CLIPVisionConfig` with `patch_size=16`, built offline, eager attention), keyed through vit_pin's key map - which
depends on the model family only, not on the patch size.
"""
import torch
import torch.nn as nn

import vit_pin

VIT16 = {  # name: (D, heads, eps, clip)
    "vit_s_16": (384, 6, 1e-6, False),
    "vit_b_16": (768, 12, 1e-6, False),
    "vit_b_16_clip": (768, 12, 1e-5, True),
}
PATCH = 16
TOKENS = 197
DEPTH = vit_pin.DEPTH
# the patch-32 model of the same family: vit_pin's key map and feature read-out are per family
FAMILY = {"vit_s_16": "vit_s_32", "vit_b_16": "vit_b_32", "vit_b_16_clip": "vit_b_32_clip"}


class _PatchEmbed16(nn.Module):
    def __init__(self, D, bias):
        super().__init__()
        self.proj = nn.Conv2d(3, D, PATCH, PATCH, bias=bias)


class TimmViT16(nn.Module):
    """timm VisionTransformer forward (patch_size=16, num_classes=0) in timm's parameter layout."""

    def __init__(self, name):
        super().__init__()
        D, heads, eps, clip = VIT16[name]
        self.output_size = D
        self.cls_token = nn.Parameter(torch.zeros(1, 1, D))
        self.pos_embed = nn.Parameter(torch.zeros(1, TOKENS, D))
        self.patch_embed = _PatchEmbed16(D, bias=not clip)
        self.norm_pre = nn.LayerNorm(D, eps=eps) if clip else None
        self.blocks = nn.Sequential(*[vit_pin._Block(D, heads, eps) for _ in range(DEPTH)])
        self.norm = nn.LayerNorm(D, eps=eps)

    film_slot_names = vit_pin.TimmViT.film_slot_names
    forward = vit_pin.TimmViT.forward


# ---- Hugging Face counterparts --------------------------------------------------------------------------------------
def hf_model(name):
    """The HF model with the timm hyper-parameters at patch_size=16, randomly initialised (offline), eval mode, eager attention."""
    D, heads, eps, clip = VIT16[name]
    if clip:
        from transformers import CLIPVisionConfig, CLIPVisionModel
        cfg = CLIPVisionConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=DEPTH, num_attention_heads=heads,
                               image_size=224, patch_size=PATCH, hidden_act="gelu", layer_norm_eps=eps, num_channels=3)
        cfg._attn_implementation = "eager"
        return CLIPVisionModel(cfg).eval()
    from transformers import ViTConfig, ViTModel
    cfg = ViTConfig(hidden_size=D, intermediate_size=4 * D, num_hidden_layers=DEPTH, num_attention_heads=heads,
                    image_size=224, patch_size=PATCH, hidden_act="gelu", layer_norm_eps=eps, qkv_bias=True, num_channels=3)
    cfg._attn_implementation = "eager"
    return ViTModel(cfg, add_pooling_layer=False).eval()


def hf_features(name, model, frames):
    return vit_pin.hf_features(FAMILY[name], model, frames)


def hf_state_dict(name, timm_sd):
    """timm-keyed state_dict -> the HF model's (vit_pin's map; CLIP's position table has 197 rows here)."""
    D, heads, eps, clip = VIT16[name]
    out = vit_pin.hf_state_dict(FAMILY[name], {k: (v.reshape(-1)[:vit_pin.TOKENS * D] if clip and k == "pos_embed" else v)
                                               for k, v in timm_sd.items()})
    if clip:
        out["embeddings.position_embedding.weight"] = timm_sd["pos_embed"].reshape(TOKENS, D)
    return out


def load_hf(name, model, timm_sd):
    """Load a timm-keyed state_dict into the HF model; every HF parameter must be covered."""
    sd = hf_state_dict(name, timm_sd)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    params = {k for k, _ in model.named_parameters()}
    assert not (params & set(missing)), sorted(params & set(missing))[:5]
    return model


def film_swap_hf(name, timm_film):
    return vit_pin.film_swap_hf(FAMILY[name], timm_film)


def film_features_hf(name, model, timm_film, frames):
    """The HF model's features with every FiLM LayerNorm's weight / bias replaced (torch.func.functional_call)."""
    from torch.func import functional_call
    out = functional_call(model, film_swap_hf(name, timm_film), (), {"pixel_values": frames})
    return out.pooler_output if VIT16[name][3] else out.last_hidden_state[:, 0]
