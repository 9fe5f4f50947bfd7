"""Pins of the three size queries of the network plans - orbit_extractor_tape_bytes, orbit_extractor_backward_workspace_bytes,
orbit_extractor_workspace_bytes - for every trainable plan at B = 1, 3 and 200. Callers allocate by these numbers, and the
graph-replay keys of the training entry points hold the addresses their allocator returns for them: a restructuring of the
tape or workspace layout must not move them. No GPU is needed: creating a plan and sizing it do not touch the device."""
import ctypes

import pytest

from orbit_dataset_amd import _lib

# recorded from commit ed62516 (the parent of the change that gave the backward workspace its per-op offsets):
# (name, frame size, plan flags, B) -> (tape bytes, backward workspace bytes, forward workspace bytes)
PINS = {
    ("resnet18", 84, 0, 1): (3264256, 48761344, 1054976),
    ("resnet18", 84, 0, 3): (9560320, 59305472, 3087104),
    ("resnet18", 84, 0, 200): (630271744, 1215657728, 150261248),
    ("efficientnet_b0", 64, 1, 1): (5138176, 75012352, 894208),
    ("efficientnet_b0", 64, 1, 3): (14398208, 82014720, 2346240),
    ("efficientnet_b0", 64, 1, 200): (935945472, 835248128, 145371392),
    ("efficientnet_b0", 224, 1, 1): (54914560, 111863040, 8958976),
    ("efficientnet_b0", 224, 1, 3): (163726592, 195408128, 26540544),
    ("efficientnet_b0", 224, 1, 200): (10862065920, 8431483392, 1688078592),
    ("efficientnet_v2_s", 64, 7, 1): (10269440, 95110400, 2004224),
    ("efficientnet_v2_s", 64, 7, 3): (27113216, 103034624, 4781312),
    ("efficientnet_v2_s", 64, 7, 200): (1698808064, 1098585088, 129230080),
    ("set_encoder", 84, 0, 1): (5673984, 16212224, 593152),
    ("set_encoder", 84, 0, 3): (17004544, 48037376, 1773312),
    ("set_encoder", 84, 0, 200): (1133613824, 2985834240, 118020608),
}


@pytest.mark.parametrize("name,size,flags", sorted({k[:3] for k in PINS}))
def test_size_queries_are_pinned(lib, name, size, flags):
    h = ctypes.c_void_p()
    assert lib.orbit_extractor_create_ex(name.encode(), size, size, flags, ctypes.byref(h)) == 0, _lib.last_error()
    try:
        assert lib.orbit_extractor_supports_training(h) == 1
        for B in (1, 3, 200):
            got = (lib.orbit_extractor_tape_bytes(h, B), lib.orbit_extractor_backward_workspace_bytes(h, B),
                   lib.orbit_extractor_workspace_bytes(h, B))
            assert got == PINS[(name, size, flags, B)], (name, size, flags, B, got)
    finally:
        lib.orbit_extractor_destroy(h)
