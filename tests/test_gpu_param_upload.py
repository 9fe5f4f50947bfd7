"""The three ways a parameter reaches a native handle's pool (csrc/param_pool.hip) give the same bits: `load` from host memory,
`load_async` per key from device tensors, and `load_all_async` (one gather launch from a table of device pointers), for the
convolutional runtime (set_encoder, 4-float alignment), the transformer runtime (vit_s_32, 64-float alignment) and the FiLM
generator. A re-upload through `load_all_async` follows tensors that changed in place (same pointers: the table is kept) and
tensors that moved (the table is refreshed). Both models hold tensors above 32 x 256 elements (the gather's grid-stride loop),
set_encoder and the generator also tensors below 256 (one partial block). Every comparison is torch.equal: an upload is a copy."""
import ctypes

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

pytestmark = pytest.mark.gpu

MODELS = {"set_encoder": ("extractor", 32, 2), "vit_s_32": ("vit", 224, 1)}  # entry-point family, frame size, batch


class Net:
    """One orbit_extractor / orbit_vit handle behind the calls the two families share."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        self.api, self.size, self.B = MODELS[name]
        self.h = ctypes.c_void_p()
        _lib.check(self.fn("create")(name.encode(), self.size, self.size, ctypes.byref(self.h)), "create")

    def fn(self, what):
        return getattr(self.lib, "orbit_%s_%s" % (self.api, what))

    def close(self):
        self.fn("destroy")(self.h)

    def keys(self):
        n = self.fn("num_params")(self.h)
        return [(self.fn("param_name")(self.h, i).decode(), self.fn("param_numel")(self.h, i)) for i in range(n)]

    def load(self, params):  # host memory
        for k, t in params.items():
            c = t.cpu()
            _lib.check(self.fn("load")(self.h, k.encode(), ctypes.c_void_p(c.data_ptr()), c.numel()), "load " + k)

    def load_async(self, params):  # device tensors, key by key
        for k, t in params.items():
            _lib.check(self.fn("load_async")(self.h, k.encode(), _lib.dptr(t), t.numel(), _lib.stream_handle()), "load_async " + k)

    def load_all_async(self, tensors, n=None):  # returns the code: the refusals are tested too
        ptrs = (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
        return self.fn("load_all_async")(self.h, ptrs, len(tensors) if n is None else n, _lib.stream_handle())

    def features(self, frames):
        _lib.check(self.fn("finalize")(self.h, _lib.stream_handle()), "finalize")
        ws = torch.empty(self.fn("workspace_bytes")(self.h, self.B), dtype=torch.uint8, device=frames.device)
        feats = torch.empty(self.B, self.fn("output_size")(self.h), device=frames.device)
        _lib.check(self.fn("forward")(self.h, _lib.dptr(frames), self.B, None, None, _lib.dptr(feats),
                                      ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_handle()), "forward")
        torch.cuda.synchronize()
        return feats


def _random_params(net, device, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, n in net.keys():
        t = 0.05 * torch.randn(n, generator=g)
        if k.endswith("running_var"):
            t = t.abs() + 0.5
        out[k] = t.to(device)
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_three_upload_paths_and_two_re_uploads_give_the_same_features(lib, device, name):
    _lib.require_gpu()
    nets = [Net(lib, name) for _ in range(3)]
    try:
        host, per_key, batched = nets
        params = _random_params(host, device, 1)
        sizes = [t.numel() for t in params.values()]
        assert max(sizes) > 32 * 256                  # the gather's grid-stride loop
        assert min(sizes) < 256 or name == "vit_s_32"  # one partial block (the transformer's smallest tensor is D = 384)
        frames = torch.randn(host.B, 3, host.size, host.size, generator=torch.Generator().manual_seed(2)).to(device)
        host.load(params)
        per_key.load_async(params)
        assert batched.load_all_async(list(params.values())) == 0, _lib.last_error()
        want = host.features(frames)
        assert torch.isfinite(want).all() and want.abs().max() > 0
        assert torch.equal(per_key.features(frames), want)
        assert torch.equal(batched.features(frames), want)

        def fresh():  # a new handle, loaded key by key with the current values
            net = Net(lib, name)
            nets.append(net)
            net.load_async(params)
            return net.features(frames)

        big = max(params, key=lambda k: params[k].numel())
        small = min(params, key=lambda k: params[k].numel())
        params[big].mul_(1.5)  # in place: same pointers, the pointer table is kept
        assert batched.load_all_async(list(params.values())) == 0, _lib.last_error()
        got = batched.features(frames)
        assert not torch.equal(got, want)
        assert torch.equal(got, fresh())
        old = params[small]  # (kept alive: the copy below gets a new address)
        params[small] = old * 0.5 + 0.25
        assert params[small].data_ptr() != old.data_ptr()
        assert batched.load_all_async(list(params.values())) == 0, _lib.last_error()
        got2 = batched.features(frames)
        assert not torch.equal(got2, got)
        assert torch.equal(got2, fresh())
    finally:
        for net in nets:
            net.close()


# ---- FiLM generator ------------------------------------------------------------------------------------------------------
FILM_TENSORS = ("w1", "b1", "ln_w", "ln_b", "w2", "b2", "reg", "init")
Z, HID, OUTS, KINDS, DST = 8, 8, (5, 16, 33), (0, 1, 0), (0, 0, 5)  # gamma: 5 + 33 floats, beta: 16; w2 of the third: 264 floats


class FilmGen:
    def __init__(self, lib):
        self.lib, self.h = lib, ctypes.c_void_p()
        arr = lambda v: (ctypes.c_int * len(v))(*v)
        _lib.check(lib.orbit_filmgen_create(len(OUTS), Z, HID, arr(OUTS), arr(KINDS), arr(DST), ctypes.byref(self.h)), "create")

    def close(self):
        self.lib.orbit_filmgen_destroy(self.h)

    def load(self, tensors):  # per tensor, from host memory
        for i, t in enumerate(tensors):
            c = t.cpu()
            _lib.check(self.lib.orbit_filmgen_load(self.h, i // 8, FILM_TENSORS[i % 8].encode(), ctypes.c_void_p(c.data_ptr()),
                                                   c.numel()), "filmgen_load")

    def load_all_async(self, tensors, n=None):
        ptrs = (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
        return self.lib.orbit_filmgen_load_all_async(self.h, ptrs, len(tensors) if n is None else n, _lib.stream_handle())

    def forward(self, z):
        gamma, beta = torch.full((38,), 7.0, device=z.device), torch.full((16,), 7.0, device=z.device)
        l2 = torch.zeros(1, device=z.device)
        _lib.check(self.lib.orbit_filmgen_forward(self.h, _lib.dptr(z), _lib.dptr(gamma), _lib.dptr(beta), _lib.dptr(l2),
                                                  _lib.stream_handle()), "filmgen_forward")
        torch.cuda.synchronize()
        return torch.cat([gamma, beta, l2])


def _film_tensors(device, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for o in OUTS:
        for n in (HID * Z, HID, HID, HID, o * HID, o, o, o):
            out.append(torch.randn(n, generator=g).to(device))
    return out


def test_filmgen_per_tensor_and_batched_upload_give_the_same_vectors(lib, device):
    _lib.require_gpu()
    a, b, c = FilmGen(lib), FilmGen(lib), FilmGen(lib)
    try:
        tensors = _film_tensors(device, 3)
        assert any(n % 4 for n in OUTS) and max(t.numel() for t in tensors) > 256
        z = torch.randn(Z, generator=torch.Generator().manual_seed(4)).to(device)
        a.load(tensors)
        assert b.load_all_async(tensors) == 0, _lib.last_error()
        want = a.forward(z)
        assert torch.isfinite(want).all() and not (want[:54] == 7.0).any()
        assert torch.equal(b.forward(z), want)
        old = tensors[8 * 2 + 4]  # w2 of the third generator moves to new storage with new values
        tensors[8 * 2 + 4] = old * 0.5 + 0.25
        assert tensors[8 * 2 + 4].data_ptr() != old.data_ptr()
        assert b.load_all_async(tensors) == 0, _lib.last_error()
        c.load(tensors)
        got = b.forward(z)
        assert not torch.equal(got, want)
        assert torch.equal(got, c.forward(z))
    finally:
        for g in (a, b, c):
            g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_batched_upload_refuses_a_wrong_count_and_a_null_tensor(lib, device, name):
    """Both refusals come before the gather launch (a launch would read the null pointer, and would mark every parameter
    loaded): the plan still reports its parameters as never loaded."""
    _lib.require_gpu()
    net = Net(lib, name)
    try:
        tensors = list(_random_params(net, device, 5).values())
        n = len(tensors)
        assert net.load_all_async(tensors[:-1]) != 0
        assert "%s_load_all_async: %d pointers for %d parameters" % (net.api, n - 1, n) in _lib.last_error()
        assert net.load_all_async(tensors[:3] + [None] + tensors[4:]) != 0
        assert "%s_load_all_async: null tensor 3" % net.api in _lib.last_error()
        assert net.fn("finalize")(net.h, None) != 0 and "never loaded" in _lib.last_error()
        torch.cuda.synchronize()
    finally:
        net.close()


def test_filmgen_batched_upload_refuses_a_wrong_count_and_a_null_tensor(lib, device):
    """... and the generator's pool is untouched: its vectors are those of the tensors loaded before."""
    _lib.require_gpu()
    g = FilmGen(lib)
    try:
        tensors = _film_tensors(device, 6)
        z = torch.randn(Z, generator=torch.Generator().manual_seed(7)).to(device)
        g.load(tensors)
        want = g.forward(z)
        other = [t + 1.0 for t in tensors]
        assert g.load_all_async(other, n=len(other) - 1) != 0
        assert "filmgen_load_all_async: 23 pointers for 3 generators x 8 tensors" in _lib.last_error()
        assert g.load_all_async(other[:9] + [None] + other[10:]) != 0
        assert "filmgen_load_all_async: null tensor 9" in _lib.last_error()
        assert torch.equal(g.forward(z), want)
    finally:
        g.close()
