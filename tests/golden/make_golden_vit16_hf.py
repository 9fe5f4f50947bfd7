"""Generate G17_vit16_hf.npz: features of the patch-16 transformer extractors computed by Hugging Face transformers alone.

As make_golden_vit_hf.py (G15) for vit_s_16 / vit_b_16 / vit_b_16_clip: the synthetic timm-keyed parameters
(synthetic.init_parameters_ on the timm layout of tests/vit16_pin.py) are re-keyed into `ViTModel` / `CLIPVisionModel` with
patch_size=16, and the features of a few seeded frames are recorded with and without FiLM (every FiLM LayerNorm's weight / bias
replaced through torch.func.functional_call). Checksums of the regenerated frames, parameters and FiLM vectors are stored beside
them, so that a change of the generators shows up as drift rather than as a kernel error. Features and checksums only.

    python tests/golden/make_golden_vit16_hf.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

NAMES = ("vit_s_16", "vit_b_16", "vit_b_16_clip")
FRAMES = 2
SEED = 17


def inputs(name):
    """(timm-keyed state_dict, frames [FRAMES,3,224,224], FiLM dict {slot.weight/.bias}) - deterministic."""
    import vit16_pin
    from orbit_dataset_amd import synthetic
    fe = vit16_pin.TimmViT16(name)
    synthetic.init_parameters_(fe)
    sd = {k: v.detach().clone() for k, v in fe.state_dict().items()}
    g = torch.Generator().manual_seed(SEED)
    frames = torch.randn(FRAMES, 3, 224, 224, generator=g)
    film = {}
    for slot in fe.film_slot_names():
        w, b = sd[slot + ".weight"], sd[slot + ".bias"]
        film[slot + ".weight"] = w * (1 + 0.1 * torch.randn(w.shape, generator=g))
        film[slot + ".bias"] = b + 0.1 * torch.randn(b.shape, generator=g)
    return sd, frames, film


def checksum(tensors):
    """order-independent float64 sum of |x| and of x * (index + 1) over a dict / list of tensors"""
    items = sorted(tensors.items()) if isinstance(tensors, dict) else list(enumerate(tensors))
    a = b = 0.0
    for _, t in items:
        t = t.detach().double().reshape(-1)
        a += t.abs().sum().item()
        b += (t * torch.arange(1, t.numel() + 1, dtype=torch.float64)).sum().item() / t.numel()
    return np.array([a, b])


def main():
    import vit16_pin
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    for name in NAMES:
        sd, frames, film = inputs(name)
        hf = vit16_pin.load_hf(name, vit16_pin.hf_model(name), sd)
        with torch.no_grad():
            plain = vit16_pin.hf_features(name, hf, frames)
            filmed = vit16_pin.film_features_hf(name, hf, film, frames)
        out[name + "_features"] = plain.numpy().astype(np.float32)
        out[name + "_features_film"] = filmed.numpy().astype(np.float32)
        out[name + "_sum_params"] = checksum(sd)
        out[name + "_sum_frames"] = checksum([frames])
        out[name + "_sum_film"] = checksum(film)
        print(name, "feature std %.3f, FiLM moves features by %.3f" % (plain.std().item(),
                                                                          (plain - filmed).abs().max().item()))
    path = os.path.join(HERE, "G17_vit16_hf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
