"""CPU emulation of the opt-in bf16 token GEMMs (orbit_vit_enable_bf16) on the pins of tests/vit_pin.py / tests/vit16_pin.py:
every qkv / proj / fc1 / fc2 Linear of the twelve blocks sees its weight and its input rounded to bf16 (round to nearest even),
and everything else - the patch embedding, the LayerNorms, attention, the residual stream, the accumulation itself - stays in
the model's own dtype. In float64 this is what the device computes up to its fp32 arithmetic."""
import torch
import torch.nn as nn


def round_bf16(t):
    """t rounded to the nearest bf16 (ties to even), in t's own dtype (float32 or float64 stay what they were)"""
    return t.bfloat16().to(t.dtype)


def _round_input(module, args):
    return (round_bf16(args[0]),) + tuple(args[1:])


def emulate_bf16_linears(model):
    """In place, on a TimmViT / TimmViT16: rounds the weight of every nn.Linear under model.blocks (the biases stay) and
    registers a forward pre-hook that rounds its input. Returns the model."""
    linears = [m for m in model.blocks.modules() if isinstance(m, nn.Linear)]
    assert len(linears) == 4 * len(model.blocks)
    with torch.no_grad():
        for m in linears:
            m.weight.copy_(round_bf16(m.weight))
            m.register_forward_pre_hook(_round_input)
    return model
