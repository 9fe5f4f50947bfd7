"""The FiLM generator kernels of csrc/film.hip (filmgen_kernel, film_l2_kernel, filmgen_bwd_kernel, filmgen_dz_kernel) through
the C ABI, forward and backward, against a float64 CPU evaluation of the same operation on the same fp32 inputs, and the Python
path on top of them (model/feature_adapters.FilmParameterGenerator with model/autograd.FilmGeneratorFunction) against
oracle.blocks.FilmParameterGenerator in float64.

Reference: plain torch, Linear -> layer_norm(eps 1e-5) -> relu -> Linear, times `reg`, then init * (g + 1) for a weight generator
and init + g for a bias generator, l2 = sum reg^2; gradients from autograd of sum(gamma * Dg) + sum(beta * Db) + c * l2 with
seeded random Dg, Db and c = 0.37. It runs once in float64 and once in float32; e32 is the float32 run's error against float64.

Gate (tests/test_gpu_vit_ops.gate), per tensor - gamma, beta, l2, each of the seven gradient tensors of each generator, dz:

    max |got - ref64|  <=  max(4 * e32, 8 * 2**-24 * max |ref64|)

Inputs: `reg` ~ randn at full strength (an error in the MLP output reaches gamma / beta and d reg undiluted), w1 ~ randn / sqrt(z),
w2 ~ randn / sqrt(hid), ln_w = 1 +- 0.1, non-zero b1 / ln_b / b2, |init| in [0.5, 1.5]. The seeds are chosen so that the float64
ReLU pre-activations keep |pre| > 1e-4 (asserted on the CPU): the float32 and float64 masks are then the same.

Shapes (z_dim, hid): (64, 64) the product's, (256, 256) both limits, (5, 3), (64, 200), (200, 64). Every handle has twelve
generators, a bias and a weight generator for each of the widths 1, 5, 255, 256, 257, 1152, the two of a width sharing one slot
offset as in the product and the slots laid out in another order than the generators: max_out = 1152 next to out = 1 runs the
forward kernel's early return of whole 256-output chunks beside the backward kernel's o += 256 loop. gamma, beta, dz and the
flat gradient sit between guard bands and start out holding a sentinel: the forward must write every destination element and
nothing else, the backward every element of the seven parameter ranges of every generator and neither the `init` ranges nor
the pool's alignment padding nor the guards.

Largest err / e32 seen on the MI355X, over all shapes and variants (every case prints its ratios; run with -s):
  gamma 1.94  beta 2.45  l2 1.83  dz 1.22  d w1 3.37  d b1 3.69  d ln_w 5.20  d ln_b 2.29  d w2 3.35  d b2 1.00  d reg 19.43
  through the module (z 48, hid 80): film 2.02  l2 0.10  d x 1.05  d Linear 1 2.16  d LayerNorm 1.42  d Linear 2 2.22  d reg 1.78
Three tensors are beyond the factor 4 and above the floor, all of a one-output generator, where e32 is the rounding error of
very few numbers: d ln_w of generator 1 at (200, 64) 5.20, and d reg of generator 0 at (64, 64) - a single number - 7.33 without
dl2 and 19.43 at the second z (d reg 12.24 at (200, 64) and 4.56 at (64, 64) are under the floor). tests/film_emulation.py
restates the backward kernel in float32 in its own summation order on the CPU: its error against float64 is the same 5.20,
7.33 and 19.43 and the kernel's distance from it is 0, so the excess is the order of the sums (the LayerNorm statistics and
the 64-term dot products are index-ordered chains on the GPU, blocked sums in torch). WIDENED gives these three tensors, and no
other, the measured ratio plus a quarter, and the test holds each of them to the unwidened gate against the emulation. e32 is
torch's float32 CPU arithmetic and so depends on the host: where torch sums in index order too, e32 is larger.
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from oracle import blocks  # noqa: E402
from orbit_dataset_amd import _lib  # noqa: E402
from test_gpu_vit_ops import gate  # noqa: E402

TENSORS = ("w1", "b1", "ln_w", "ln_b", "w2", "b2", "reg", "init")
SHAPES = [(64, 64), (256, 256), (5, 3), (64, 200), (200, 64)]
WIDTHS = (1, 5, 255, 256, 257, 1152)        # generator order (the product sorts its names) ...
SLOTS = (257, 1, 1152, 5, 256, 255)         # ... and destination order (the extractor's module order)
SLOT_OFFSET = {w: sum(SLOTS[:i]) for i, w in enumerate(SLOTS)}
LAYOUT = [(w, kind, SLOT_OFFSET[w]) for w in WIDTHS for kind in (1, 0)]  # (out, kind, dst): 'x.bias' sorts before 'x.weight'
FILM = sum(SLOTS)
C_L2 = 0.37
GUARD = 256          # floats on either side of gamma, beta, dz and the flat gradient
SENTINEL = 7777.0
MIN_PRE = 1e-4
# (z_dim, hid) -> seed of the parameters; z seeds below. Chosen on the CPU for min |pre| > MIN_PRE, see _reference.
SEED = {(64, 64): 1, (256, 256): 2, (5, 3): 3, (64, 200): 4, (200, 64): 5}
Z_SEED, Z_SEED_2 = 11, 12
U = 2.0 ** -24
# (z_dim, hid, z seed, c, generator, tensor) -> factor in place of 4: the ratio measured on the MI355X plus a quarter, see the
# docstring. All three are one-output generators; the kernel and its emulation (tests/film_emulation.py) agree to the last bit.
# e32 is the host's float32 arithmetic: the figures were measured with the CPU reference of torch 2.10.0 (ROCm 7.0 build) at
# the 16 intra-op threads tests/conftest.py sets; another torch build or thread count can move e32 and so these ratios.
WIDENED = {
    (200, 64, 11, C_L2, 1, "ln_w"): 5.45,   # kernel 5.20, emulation 5.20: err 5.8e-9 on values up to 9.7e-3
    (64, 64, 11, None, 0, "reg"): 7.58,     # kernel 7.33: d reg is ONE number (0.886, err 4.8e-7), e32 one draw of a rounding error
    (64, 64, 12, C_L2, 0, "reg"): 19.68,    # kernel 19.43: the same number at the second z (0.0647, err 2.0e-7, e32 1.0e-8)
}


def _numel(z_dim, hid, out):
    return dict(zip(TENSORS, (hid * z_dim, hid, hid, hid, out * hid, out, out, out)))


@functools.lru_cache(maxsize=None)
def _inputs(z_dim, hid):
    """fp32 parameters of the twelve generators and the upstream gradients Dg, Db."""
    g = torch.Generator().manual_seed(SEED[(z_dim, hid)])
    rn = lambda *s: torch.randn(*s, generator=g)
    gens = []
    for out, _, _ in LAYOUT:
        init = (0.5 + torch.rand(out, generator=g)) * (2.0 * torch.randint(0, 2, (out,), generator=g) - 1.0)
        gens.append(dict(w1=rn(hid, z_dim) / math.sqrt(z_dim), b1=0.3 * rn(hid), ln_w=1.0 + 0.1 * rn(hid), ln_b=0.3 * rn(hid),
                         w2=rn(out, hid) / math.sqrt(hid), b2=0.3 * rn(out), reg=rn(out), init=init))
    return gens, rn(FILM), rn(FILM)


def _z(z_dim, seed):
    return torch.randn(z_dim, generator=torch.Generator().manual_seed(seed))


def _evaluate(gens, Dg, Db, z, c, dtype):
    """The operation in plain torch at `dtype`: gamma, beta, l2, per-generator gradients, dz, smallest |ReLU pre-activation|."""
    z = z.clone().to(dtype).requires_grad_(True)
    leaves = [{k: v.clone().to(dtype).requires_grad_(k != "init") for k, v in p.items()} for p in gens]
    gamma, beta = torch.zeros(FILM, dtype=dtype), torch.zeros(FILM, dtype=dtype)
    loss, l2, min_pre = 0.0, 0.0, float("inf")
    for p, (out, kind, dst) in zip(leaves, LAYOUT):
        pre = F.layer_norm(F.linear(z, p["w1"], p["b1"]), (p["b1"].numel(),), p["ln_w"], p["ln_b"], 1e-5)
        min_pre = min(min_pre, pre.detach().abs().min().item())
        g = F.linear(torch.relu(pre), p["w2"], p["b2"]) * p["reg"]
        film = p["init"] * (g + 1.0) if kind == 0 else p["init"] + g
        (gamma if kind == 0 else beta)[dst:dst + out] = film.detach()
        loss = loss + (film * (Dg if kind == 0 else Db)[dst:dst + out].to(dtype)).sum()
        l2 = l2 + (p["reg"] ** 2).sum()
    (loss + c * l2).backward()
    grads = [{k: p[k].grad.reshape(-1) for k in TENSORS[:7]} for p in leaves]
    return dict(gamma=gamma, beta=beta, l2=l2.detach().reshape(1), grads=grads, dz=z.grad, min_pre=min_pre)


@functools.lru_cache(maxsize=None)
def _reference(z_dim, hid, z_seed=Z_SEED, c=C_L2):
    """(float64 run, float32 run) of one case; computed once and shared, never modified."""
    gens, Dg, Db = _inputs(z_dim, hid)
    z = _z(z_dim, z_seed)
    ref64 = _evaluate(gens, Dg, Db, z, c, torch.float64)
    # a condition on the inputs, not on the kernel: away from the ReLU's kink the fp32 and fp64 masks are the same
    assert ref64["min_pre"] > MIN_PRE, "pick another seed: min |pre| = %.3g" % ref64["min_pre"]
    return ref64, _evaluate(gens, Dg, Db, z, c, torch.float32)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


class Gen:
    """One orbit_filmgen handle with the twelve generators of LAYOUT, loaded tensor by tensor from host memory."""

    def __init__(self, lib, device, z_dim, hid):
        self.lib, self.device, self.z_dim, self.hid, self.h = lib, device, z_dim, hid, ctypes.c_void_p()
        _lib.check(lib.orbit_filmgen_create(len(LAYOUT), z_dim, hid, _ints([l[0] for l in LAYOUT]), _ints([l[1] for l in LAYOUT]),
                                            _ints([l[2] for l in LAYOUT]), ctypes.byref(self.h)), "filmgen_create")
        gens, Dg, Db = _inputs(z_dim, hid)
        for i, p in enumerate(gens):
            for k in TENSORS:
                t = p[k].contiguous()
                _lib.check(lib.orbit_filmgen_load(self.h, i, k.encode(), ctypes.c_void_p(t.data_ptr()), t.numel()), "filmgen_load")
        self.Dg, self.Db = Dg.to(device), Db.to(device)
        self.floats = lib.orbit_filmgen_grad_floats(self.h)
        # [first, last) of every parameter range of the flat gradient
        self.ranges = []
        for i, (out, _, _) in enumerate(LAYOUT):
            n = _numel(z_dim, hid, out)
            self.ranges.append({k: (lib.orbit_filmgen_param_offset(self.h, i, k.encode()), n[k]) for k in TENSORS[:7]})

    def close(self):
        self.lib.orbit_filmgen_destroy(self.h)

    def _buf(self, n):
        return torch.full((n + 2 * GUARD,), SENTINEL, device=self.device)

    @staticmethod
    def _inner(buf):
        return ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)

    def forward(self, z):
        """-> gamma, beta (each with its guard bands) and l2, on the host."""
        gamma, beta, l2 = self._buf(FILM), self._buf(FILM), self._buf(1)
        zd = z.to(self.device)
        _lib.check(self.lib.orbit_filmgen_forward(self.h, _lib.dptr(zd), self._inner(gamma), self._inner(beta), self._inner(l2),
                                                  _lib.stream_handle()), "filmgen_forward")
        torch.cuda.synchronize()
        return gamma.cpu(), beta.cpu(), l2.cpu()

    def backward_async(self, z, c=C_L2, with_dz=True):
        """-> device buffers (flat gradient, dz), guard bands included; the caller synchronises."""
        flat, dz = self._buf(self.floats), self._buf(self.z_dim)
        zd = z.to(self.device)
        dl2 = None if c is None else torch.tensor([c], device=self.device)
        _lib.check(self.lib.orbit_filmgen_backward(self.h, _lib.dptr(zd), _lib.dptr(self.Dg), _lib.dptr(self.Db), _lib.dptr(dl2),
                                                   self._inner(flat), self._inner(dz) if with_dz else None, _lib.stream_handle()),
                   "filmgen_backward")
        self._keep = (zd, dl2)  # alive until the caller's synchronize
        return flat, dz

    def backward(self, z, c=C_L2, with_dz=True):
        flat, dz = self.backward_async(z, c, with_dz)
        torch.cuda.synchronize()
        return flat.cpu(), dz.cpu()


@pytest.fixture(scope="module")
def gen64(lib, device):
    _lib.require_gpu()
    g = Gen(lib, device, 64, 64)
    yield g
    g.close()


def _guards_intact(buf, what):
    assert torch.all(buf[:GUARD] == SENTINEL) and torch.all(buf[-GUARD:] == SENTINEL), "%s: a guard band was written" % what


class Check:
    """The gate, tensor by tensor, without stopping at the first tensor over its bound: finish() reports them all."""

    def __init__(self, tag, case=None):
        self.tag, self.case, self.ratios, self.failures, self.over4 = tag, case, {}, [], []

    def gate(self, cls, got, r64, r32, what, key=None):
        e32 = (r32.double() - r64).abs().max().item()
        factor = WIDENED.get(self.case + key, 4.0) if (self.case and key) else 4.0
        err = (got.double() - r64).abs().max().item()
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        self.ratios[cls] = max(self.ratios.get(cls, 0.0), ratio)
        what = "%s %s" % (self.tag, what)
        try:
            if factor == 4.0:
                gate(got, r64, e32, what)
            else:
                tol = max(factor * e32, 8 * U * r64.abs().max().item())
                print("[vit-ops] %-58s err %.3g  e32 %.3g  err/e32 %.2f (factor %.2f)" % (what, err, e32, ratio, factor))  # gate()'s tag
                assert torch.isfinite(got).all() and err <= tol, \
                    "%s: max |got - ref64| = %.4g > %.4g (e32 = %.4g, err / e32 = %.2f)" % (what, err, tol, e32, ratio)
        except AssertionError as e:
            self.failures.append(str(e))
        if key and err > max(4.0 * e32, 8 * U * r64.abs().max().item()):
            self.over4.append((key, ratio))

    def finish(self):
        print("[film-ops] %s largest err / e32: %s" % (self.tag, "  ".join("%s %.2f" % kv for kv in self.ratios.items())))
        for key, ratio in self.over4:
            print("[film-ops] over 4 e32: %r: %.2f," % (self.case + key, ratio))
        assert not self.failures, "\n".join(self.failures)


def _check_forward(chk, gamma, beta, l2, ref64, ref32):
    for name, buf in (("gamma", gamma), ("beta", beta), ("l2", l2)):
        _guards_intact(buf, chk.tag + " " + name)
        got = buf[GUARD:-GUARD]
        assert not (got == SENTINEL).any(), "%s %s: destination elements left unwritten" % (chk.tag, name)
        chk.gate(name, got, ref64[name], ref32[name], name)


def _check_backward(chk, gen, flat, dz, ref64, ref32, with_dz=True):
    """Gates the seven gradient tensors of every generator and dz; checks what was written and what was not."""
    tag = chk.tag
    _guards_intact(flat, tag + " grads")
    _guards_intact(dz, tag + " dz")
    inner = flat[GUARD:-GUARD]
    written = torch.zeros(gen.floats, dtype=torch.bool)
    for i, rng in enumerate(gen.ranges):
        for k, (off, n) in rng.items():
            assert off + n <= gen.floats and not written[off:off + n].any(), "%s: parameter ranges overlap" % tag
            written[off:off + n] = True
            got = inner[off:off + n]
            assert not (got == SENTINEL).any(), "%s: d %s of generator %d was left to the caller's fill" % (tag, k, i)
            chk.gate(k, got, ref64["grads"][i][k], ref32["grads"][i][k], "gen %d (out %d) d%s" % (i, LAYOUT[i][0], k), key=(i, k))
    # the `init` ranges and the alignment padding between tensors: 2 * FILM floats of init at the least
    assert (~written).sum().item() >= 2 * FILM
    assert torch.all(inner[~written] == SENTINEL), "%s: the backward wrote outside the seven parameter ranges" % tag
    if with_dz:
        got = dz[GUARD:-GUARD]
        assert not (got == SENTINEL).any(), "%s: dz elements left unwritten" % tag
        chk.gate("dz", got, ref64["dz"], ref32["dz"], "dz")
    else:
        assert torch.all(dz == SENTINEL)


def _explain_over4(chk, gen, flat, ref64, ref32):
    """For every gradient tensor beyond 4 e32: the same figure for the fp32 emulation of the kernel's summation order
    (tests/film_emulation.py), and the kernel's distance from that emulation. A tensor with a widened factor must meet the
    unwidened gate with the emulation as its reference: its distance from float64 is then that of the summation order."""
    if not chk.over4:
        return
    import film_emulation
    emu = film_emulation.backward(_inputs(gen.z_dim, gen.hid), LAYOUT, _z(gen.z_dim, chk.case[2]), chk.case[3])
    for (i, k), ratio in chk.over4:
        off, n = gen.ranges[i][k]
        got, want = flat[GUARD + off:GUARD + off + n], torch.from_numpy(emu[i][k]).reshape(-1)
        r64, r32 = ref64["grads"][i][k], ref32["grads"][i][k]
        e32 = (r32.double() - r64).abs().max().item()
        emu_ratio = (want.double() - r64).abs().max().item() / e32
        dist = (got.double() - want.double()).abs().max().item()
        print("[film-ops] %s gen %d d%s: kernel err / e32 %.2f, emulation err / e32 %.2f, |kernel - emulation| / e32 %.3f"
              % (chk.tag, i, k, ratio, emu_ratio, dist / e32))
        if chk.case + (i, k) in WIDENED:
            assert dist <= max(4.0 * e32, 8 * U * r64.abs().max().item()), "gen %d d%s: the kernel is not its emulation" % (i, k)


# ---- the kernels at every shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_dim,hid", SHAPES, ids=["z%d-hid%d" % s for s in SHAPES])
def test_filmgen_forward_backward_match_fp64(lib, device, z_dim, hid):
    _lib.require_gpu()
    assert min(WIDTHS) <= 256 < max(WIDTHS) and {l[1] for l in LAYOUT} == {0, 1}
    ref64, ref32 = _reference(z_dim, hid)
    gen = Gen(lib, device, z_dim, hid)
    try:
        chk = Check("z %d hid %d" % (z_dim, hid), (z_dim, hid, Z_SEED, C_L2))
        z = _z(z_dim, Z_SEED)
        _check_forward(chk, *gen.forward(z), ref64, ref32)
        flat, dz = gen.backward(z)
        _check_backward(chk, gen, flat, dz, ref64, ref32)
        _explain_over4(chk, gen, flat, ref64, ref32)
        chk.finish()
    finally:
        gen.close()


# ---- variants at the product's shape ------------------------------------------------------------------------------------
def test_filmgen_backward_without_dl2_is_the_gradient_at_c_0(gen64):
    ref64, ref32 = _reference(64, 64, Z_SEED, 0.0)
    chk = Check("dl2 = NULL", (64, 64, Z_SEED, None))
    flat, dz = gen64.backward(_z(64, Z_SEED), c=None)
    _check_backward(chk, gen64, flat, dz, ref64, ref32)
    _explain_over4(chk, gen64, flat, ref64, ref32)
    chk.finish()
    # ... and the l2 term is there when dl2 is: d reg differs from the call above by 2 c reg
    with_l2, _ = gen64.backward(_z(64, Z_SEED))
    off, n = gen64.ranges[-1]["reg"]
    assert (with_l2[GUARD + off:GUARD + off + n] - flat[GUARD + off:GUARD + off + n]).abs().max().item() > 0.1


def test_filmgen_backward_without_dz_gives_the_same_parameter_gradients(gen64):
    z = _z(64, Z_SEED)
    flat, dz = gen64.backward(z)
    flat_no_dz, dz_untouched = gen64.backward(z, with_dz=False)
    assert torch.equal(flat_no_dz, flat)  # bit for bit, sentinels included
    assert torch.all(dz_untouched == SENTINEL) and not (dz[GUARD:-GUARD] == SENTINEL).any()
    chk = Check("dz = NULL", (64, 64, Z_SEED, C_L2))
    _check_backward(chk, gen64, flat_no_dz, dz_untouched, *_reference(64, 64), with_dz=False)
    chk.finish()


def test_filmgen_two_backward_calls_on_one_handle_keep_their_own_dz(gen64):
    """The per-generator dz partials live in one buffer owned by the handle: two calls in stream order, read afterwards."""
    z1, z2 = _z(64, Z_SEED), _z(64, Z_SEED_2)
    a = gen64.backward_async(z1)
    keep = gen64._keep
    b = gen64.backward_async(z2)
    torch.cuda.synchronize()
    del keep
    for tag, z_seed, (flat, dz) in (("first call", Z_SEED, a), ("second call", Z_SEED_2, b)):
        chk = Check(tag, (64, 64, z_seed, C_L2))
        _check_backward(chk, gen64, flat.cpu(), dz.cpu(), *_reference(64, 64, z_seed))
        _explain_over4(chk, gen64, flat.cpu(), *_reference(64, 64, z_seed))
        chk.finish()
    assert not torch.equal(a[1], b[1])


def test_filmgen_forward_and_backward_repeat_bit_for_bit(gen64):
    z = _z(64, Z_SEED)
    first, again = gen64.forward(z), gen64.forward(z)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    first, again = gen64.backward(z), gen64.backward(z)
    assert all(torch.equal(x, y) for x, y in zip(first, again))


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gen,z_dim,hid", [(2, 257, 64), (2, 64, 257), (0, 64, 64)], ids=["z257", "hid257", "no-generators"])
def test_filmgen_create_refuses_bad_sizes(lib, device, n_gen, z_dim, hid):
    _lib.require_gpu()
    h = ctypes.c_void_p()
    rc = lib.orbit_filmgen_create(n_gen, z_dim, hid, _ints([5, 16]), _ints([0, 1]), _ints([0, 0]), ctypes.byref(h))
    assert rc != 0 and h.value is None
    assert "filmgen_create: bad sizes (n_gen=%d z=%d hid=%d)" % (n_gen, z_dim, hid) in _lib.last_error()


def test_filmgen_init_has_no_gradient_slot_and_load_checks_the_count(gen64):
    lib = gen64.lib
    assert lib.orbit_filmgen_param_offset(gen64.h, 0, b"init") == ctypes.c_size_t(-1).value
    assert lib.orbit_filmgen_param_offset(gen64.h, 0, b"reg") < gen64.floats
    w1 = torch.zeros(64 * 64 + 1)
    assert lib.orbit_filmgen_load(gen64.h, 0, b"w1", ctypes.c_void_p(w1.data_ptr()), 64 * 64 + 1) != 0
    assert "filmgen_load: w1 of generator 0 has 4097 elements, expected 4096" in _lib.last_error()
    assert lib.orbit_filmgen_load(gen64.h, 3, b"b2", ctypes.c_void_p(w1.data_ptr()), 4) != 0
    assert "filmgen_load: b2 of generator 3 has 4 elements, expected 5" in _lib.last_error()
    # the refused loads changed nothing
    chk = Check("after refused loads")
    _check_forward(chk, *gen64.forward(_z(64, Z_SEED)), *_reference(64, 64))
    chk.finish()


# ---- the Python path -----------------------------------------------------------------------------------------------------
PY_Z, PY_HID = 48, 80
PY_WIDTHS = {"m0": 8, "m1": 40, "m2": 257, "m3": 600}
PY_SLOTS = ["m2", "m0", "m3", "m1"]  # not the sorted order
PY_SEED = 21


def _python_pair(device):
    from orbit_dataset_amd.model.feature_adapters import FilmParameterGenerator
    g = torch.Generator().manual_seed(PY_SEED)
    rn = lambda *s: torch.randn(*s, generator=g)
    sizes = {"%s.%s" % (m, k): w for m, w in PY_WIDTHS.items() for k in ("weight", "bias")}
    init = {n: (0.5 + torch.rand(w, generator=g)) * (2.0 * torch.randint(0, 2, (w,), generator=g) - 1.0) for n, w in sizes.items()}
    gen = FilmParameterGenerator(sizes, {k: v.clone() for k, v in init.items()}, PY_Z, PY_HID, slot_names=PY_SLOTS)
    with torch.no_grad():
        for blk, reg in zip(gen.generators, gen.regularizers):
            lin1, ln, _, lin2 = blk.block
            lin1.weight.copy_(rn(PY_HID, PY_Z) / math.sqrt(PY_Z)), lin1.bias.copy_(0.3 * rn(PY_HID))
            ln.weight.copy_(1.0 + 0.1 * rn(PY_HID)), ln.bias.copy_(0.3 * rn(PY_HID))
            lin2.weight.copy_(rn(lin2.out_features, PY_HID) / math.sqrt(PY_HID)), lin2.bias.copy_(0.3 * rn(lin2.out_features))
            reg.copy_(rn(reg.numel()))
    state = {k: v.clone() for k, v in gen.state_dict().items()}
    x = rn(1, PY_Z)
    R = {n: rn(w) for n, w in sizes.items()}
    refs = []
    for dtype in (torch.float64, torch.float32):
        ref = blocks.FilmParameterGenerator(sizes, {k: v.to(dtype) for k, v in init.items()}, PY_Z, PY_HID).to(dtype)
        ref.load_state_dict(state)
        xr = x.clone().to(dtype).requires_grad_(True)
        film = ref(xr)
        (sum((film[n] * R[n].to(dtype)).sum() for n in sizes) + 0.001 * ref.regularization_term()).backward()
        if dtype == torch.float64:
            pre = torch.cat([b.block[1](b.block[0](xr)).detach().reshape(-1) for b in ref.generators])
            assert pre.abs().min().item() > MIN_PRE, "pick another seed: min |pre| = %.3g" % pre.abs().min().item()
        refs.append(({n: v.detach() for n, v in film.items()}, {n: p.grad for n, p in ref.named_parameters()}, xr.grad,
                     ref.regularization_term().detach()))
    return gen.to(device), x, R, refs


def test_film_parameter_generator_module_matches_oracle_fp64(device):
    """Non-default sizes and a slot order that is not the sorted one: pins which flat-gradient range reaches which Parameter
    (b1, ln_w and ln_b have the same shape) and where each generator's output lands in gamma / beta."""
    _lib.require_gpu()
    gen, x, R, ((film64, grad64, dx64, l2_64), (film32, grad32, dx32, l2_32)) = _python_pair(device)
    assert gen.film_parameter_names == sorted(gen.film_parameter_names)
    assert [n.rsplit(".", 1)[0] for n in gen.film_parameter_names[::2]] != PY_SLOTS
    xd = x.to(device).requires_grad_(True)
    film = gen(xd)
    assert set(film) == set(film64)
    (sum((film[n] * R[n].to(device)).sum() for n in film64) + 0.001 * gen.regularization_term()).backward()
    torch.cuda.synchronize()
    chk = Check("module")

    def check(cls, got, r64, r32, what):
        assert got.shape == r64.shape, what
        chk.gate(cls, got.detach().cpu(), r64, r32, what)

    for n in film64:
        check("film", film[n], film64[n], film32[n], n)
    check("l2", gen.regularization_term().reshape(1), l2_64.reshape(1), l2_32.reshape(1), "l2")
    params = dict(gen.named_parameters())
    assert set(params) == set(grad64)
    for n, p in params.items():
        assert p.grad is not None, n
        check(n.split(".", 2)[-1] if n.startswith("generators") else "reg", p.grad, grad64[n], grad32[n], "d " + n)
    check("dx", xd.grad, dx64, dx32, "dx")
    chk.finish()
    # the no-grad forward is the same launch: bit for bit
    l2_grad = gen.regularization_term().detach().clone()
    with torch.no_grad():
        plain = gen(x.to(device))
    torch.cuda.synchronize()
    for n in film64:
        assert not plain[n].requires_grad and torch.equal(plain[n], film[n].detach()), n
    assert torch.equal(gen.regularization_term(), l2_grad)
