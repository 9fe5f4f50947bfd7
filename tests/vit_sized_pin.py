"""The pins of tests/vit_pin.py / tests/vit16_pin.py at other frame sizes than 224 (orbit_vit_create_sized;
VisionTransformer.resample_pos_embed).

`SizedViT(name)` is `TimmViT(name)` / `TimmViT16(name)` - the same modules, parameters and state_dict, `pos_embed` at its
checkpoint shape [1, 50 | 197, D] - whose forward adds the table resampled to the frame's grid: with G = S / patch patches per
side and g = 7 | 14, row 0 unchanged and rows 1..G^2

    F.interpolate(pos_embed[:, 1:].reshape(1, g, g, D).permute(0, 3, 1, 2), size=(G, G), mode="bicubic", align_corners=False)

permuted back (torch's bicubic: A = -0.75, source coordinate (i + 0.5) g / G - 0.5, four taps per axis clamped to [0, g - 1], no
antialiasing), in the model's own dtype. This is the operation of timm 0.6.12's `resize_pos_embed` restated (timm is not
installed: not run), and what transformers' `interpolate_pos_encoding=True` does (tests/test_vit_sized_host.py pins that). At
G == g the table is used as it is, without a resample. Everything else is the parent pin.
"""
import math

import torch
import torch.nn.functional as F

import vit16_pin
import vit_pin


def patch_of(name):
    return 16 if name in vit16_pin.VIT16 else 32


def resample_pos_embed(pos, G):
    """pos [1, g*g + 1, D] -> [1, G*G + 1, D] in pos's dtype (the module docstring's definition)."""
    g = math.isqrt(pos.shape[1] - 1)
    assert g * g + 1 == pos.shape[1]
    if G == g:
        return pos
    D = pos.shape[-1]
    grid = pos[:, 1:].reshape(1, g, g, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(G, G), mode="bicubic", align_corners=False)
    return torch.cat((pos[:, :1], grid.permute(0, 2, 3, 1).reshape(1, G * G, D)), dim=1)


def _forward(self, x):
    if x.dim() == 5:
        x = x.flatten(end_dim=1)
    assert x.shape[-1] == x.shape[-2] and x.shape[-1] % self.patch == 0, tuple(x.shape)
    pos = resample_pos_embed(self.pos_embed, x.shape[-1] // self.patch)
    x = self.patch_embed.proj(x).flatten(2).transpose(1, 2)
    x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1) + pos
    if self.norm_pre is not None:
        x = self.norm_pre(x)
    return self.norm(self.blocks(x))[:, 0]


class SizedViT32(vit_pin.TimmViT):
    patch = 32
    forward = _forward


class SizedViT16(vit16_pin.TimmViT16):
    patch = 16
    forward = _forward


def SizedViT(name):
    """The sized pin of any of the six models."""
    return SizedViT16(name) if name in vit16_pin.VIT16 else SizedViT32(name)


# ---- Hugging Face counterparts (the parents', called with interpolate_pos_encoding=True) ------------------------------
def _mod(name):
    return vit16_pin if name in vit16_pin.VIT16 else vit_pin


def hf_model(name):
    return _mod(name).hf_model(name)


def load_hf(name, model, timm_sd):
    return _mod(name).load_hf(name, model, timm_sd)


def hf_features(name, model, frames):
    out = model(pixel_values=frames, interpolate_pos_encoding=True)
    return out.pooler_output if name.endswith("_clip") else out.last_hidden_state[:, 0]
