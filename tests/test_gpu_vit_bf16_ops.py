"""The opt-in bf16 token GEMM of csrc/vit.hip (orbit_op_vit_linear_bf16, orbit_op_vit_pack_bf16) by the method of
tests/test_gpu_vit_ops.py, whose helpers, gate and guard-row scheme it imports.

The kernel promises: x and w are each rounded to bf16 once (round to nearest even), their products are exact, the sum is an
fp32 accumulation in ascending k, the epilogue is fp32. So the yardstick is measured on the ROUNDED operands, on the reference
side only: xr = x.bfloat16().float(), wr = w.bfloat16().float() on the CPU; ref64 is the float64 evaluation on (xr, wr); e32
the sequential fp32 chain on (xr, wr); the gate is the file's own, max |got - ref64| <= max(4 e32, 8 u max |ref64|), and the
elementwise gamma_(K+2) bound on the rounded operands applies too. The device is handed the UNROUNDED fp32 x and the weight
packed by orbit_op_vit_pack_bf16: a kernel that truncates instead of rounding, rounds twice, or leaves a layer's operand in
another precision is far outside the gate (bf16 rounding is 2**-9 relative, the gate about 2**-20).

Largest err / e32 seen on the MI355X (every case prints its ratio; run with -s): 0.61 (384x1536 gelu at M = 5376); 0.16 on the
3072-deep one_sign chain. Below 1 because the kernel sums each 64-deep K step apart from the running sum, which is more
accurate than the sequential chain that e32 measures.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

from test_gpu_vit_ops import (EPI_BIAS, EPI_GELU, EPI_RESIDUAL, GUARD, NAN, SENTINEL, SWITCH, TILES, _prof_rows, _st,  # noqa: E402
                              _switch_rows, _sync, check_linear, linear_e32, linear_inputs, linear_ref64)

# the four ViT-S layers and the long chain of ViT-B's fc2: (K, N, epilogue)
LAYERS = [(384, 1152, EPI_BIAS), (384, 384, EPI_RESIDUAL), (384, 1536, EPI_GELU), (1536, 384, EPI_RESIDUAL),
          (3072, 768, EPI_RESIDUAL)]
LAYER_IDS = ["%dx%d-%s" % (k, n, ("bias", "gelu", "residual")[e]) for k, n, e in LAYERS]
M_SWEEP = (1, 49, 50, 63, 64, 65, 127, 128, 129, 275)
M_MAX = max(M_SWEEP)
WHAT = {EPI_BIAS: "vit_op_linear_bf16", EPI_GELU: "vit_op_linear_gelu_bf16", EPI_RESIDUAL: "vit_op_linear_residual_bf16"}


def rounded(t):
    """the bf16 rounding the kernel promises, on the CPU: round to nearest even, back in fp32"""
    return t.bfloat16().float()


def pack(lib, device, w):
    """orbit_op_vit_pack_bf16 of a device fp32 tensor -> int16 device tensor of the same shape (bf16 bit patterns)"""
    out = torch.empty(w.shape, dtype=torch.int16, device=device)
    _lib.check(lib.orbit_op_vit_pack_bf16(_lib.dptr(w), ctypes.c_void_p(out.data_ptr()), w.numel(), _st()), "orbit_op_vit_pack_bf16")
    return out


def run_linear_bf16(lib, device, x, wb, bias, res, M, epi, tile, in_place=False):
    """orbit_op_vit_linear_bf16 on the first M rows of x / res, with the NaN rows, the NaN-filled output and the guard rows of
    test_gpu_vit_ops.run_linear; returns (rc, the M result rows on the CPU)."""
    N, K = wb.shape
    xp = torch.full((M + GUARD, K), NAN, device=device)
    xp[:M] = x[:M]
    y = torch.full((M + GUARD, N), NAN, device=device)
    y[M:] = SENTINEL
    rp = None
    if epi == EPI_RESIDUAL:
        if in_place:
            y[:M] = res[:M]
            rp = y
        else:
            rp = torch.zeros(M + GUARD, N, device=device)
            rp[:M] = res[:M]
    rc = lib.orbit_op_vit_linear_bf16(_lib.dptr(xp), ctypes.c_void_p(wb.data_ptr()), _lib.dptr(bias), _lib.dptr(rp), _lib.dptr(y),
                                      M, N, K, epi, tile, _st())
    _lib.check(rc, "orbit_op_vit_linear_bf16")
    _sync()
    assert bool((y[M:] == SENTINEL).all()), "rows past M were written (M=%d N=%d K=%d tile=%d)" % (M, N, K, tile)
    return y[:M].cpu()


# ---- pack ----------------------------------------------------------------------------------------------------------------
def _tie_inputs(n, seed):
    """fp32 values whose low 16 bits are exactly 0x8000 (a tie between two bf16 neighbours), with bit 16 - the parity of the
    bf16 result rounded down - set in every other element, both signs, exponents around 1"""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n, dtype=torch.int64)
    hi = torch.randint(0x3e00, 0x4100, (n,), generator=g, dtype=torch.int64)  # sign 0, exponents 124..129, 7 mantissa bits
    hi = (hi & ~1) | (i & 1)                                                  # bit 16: even, odd, even, ...
    hi = hi | (((i >> 1) & 1) << 15)                                          # sign: + + - - ...
    bits = (hi << 16) | 0x8000
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)                 # as two's complement int32
    return bits.to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("numel", [1, 7, 8, 9, 2047, 2049, 384 * 384 + 5])
def test_pack_equals_torch_bfloat16_bit_for_bit(lib, device, numel):
    """orbit_op_vit_pack_bf16 == w.bfloat16() bit for bit on random values and on exact ties of both parities, at sizes that
    are no multiple of the 8 elements a thread converts, on 16-byte aligned and on merely 2-byte aligned outputs; the elements
    behind the output keep their sentinel."""
    g = torch.Generator().manual_seed(numel)
    for what, w in (("random", 3.0 * torch.randn(numel, generator=g)), ("ties", _tie_inputs(numel, numel))):
        want = w.bfloat16().view(torch.int16)
        if what == "ties":  # the inputs are what they claim: half of them round up, half down
            lo = w.view(torch.int32) & 0xffff
            assert bool((lo == 0x8000).all())
            up = (want.int() & 0xffff) != ((w.view(torch.int32) >> 16) & 0xffff)
            assert numel < 2 or (bool(up.any()) and not bool(up.all()))
            assert bool(((want.int() & 1) == 0).all())  # ties go to even
        wd = w.to(device)
        for shift in (0, 1):  # out + 2 bytes: the element-by-element path
            buf = torch.full((numel + 64 + shift,), 0x5a5a, dtype=torch.int16, device=device)
            out = buf[shift:shift + numel]
            _lib.check(lib.orbit_op_vit_pack_bf16(_lib.dptr(wd), ctypes.c_void_p(out.data_ptr()), numel, _st()),
                       "orbit_op_vit_pack_bf16")
            _sync()
            assert torch.equal(out.cpu(), want), "%s numel=%d shift=%d" % (what, numel, shift)
            assert bool((buf[shift + numel:] == 0x5a5a).all()) and bool((buf[:shift] == 0x5a5a).all()), "guard overwritten"


# ---- linear --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,epi", LAYERS, ids=LAYER_IDS)
def test_linear_bf16_every_row_count_at_both_tile_heights(lib, device, K, N, epi):
    """Both instantiations at M = 1 .. 275 against float64 on the rounded operands; rows of x past M are NaN, guard rows after y
    are intact; every row is BITWISE the same whatever M and whatever the tile height; the profiler rows are
    vit_op_linear[_gelu|_residual]_bf16<64|128>, one launch each per M."""
    x, w, bias, res = linear_inputs(K, N, M_MAX, "normal", 100 + K + N)
    xr, wr = rounded(x), rounded(w)
    ref64, bound = linear_ref64(xr, wr, bias, res, epi)
    xd, bd, rd = x.to(device), bias.to(device), res.to(device)
    wb = pack(lib, device, w.to(device))
    assert torch.equal(wb.cpu(), w.bfloat16().view(torch.int16))
    lib.orbit_prof_enable(1)
    try:
        out = {}
        for M in M_SWEEP:
            e32 = linear_e32(xr, wr, bias, res, epi, ref64, M, seed=M)
            for tile in TILES:
                got = run_linear_bf16(lib, device, xd, wb, bd, rd, M, epi, tile)
                check_linear(got, ref64[:M], bound[:M], e32, "bf16 linear %dx%d M=%d tile=%d" % (K, N, M, tile))
                out[M, tile] = got
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    for tile in TILES:
        assert rows.get("%s<%d>" % (WHAT[epi], tile), 0) == len(M_SWEEP), rows
    big = out[M_MAX, 64]
    for (M, tile), got in out.items():
        assert torch.equal(got, big[:M]), "rows depend on M or on the tile height (M=%d, tile=%d)" % (M, tile)


@pytest.mark.parametrize("K,N,epi", [(384, 1152, EPI_BIAS), (1536, 384, EPI_RESIDUAL)], ids=["384x1152-bias", "1536x384-residual"])
def test_linear_bf16_rounds_once_to_nearest_even(lib, device, K, N, epi):
    """The same call with x rounded to bf16 on the CPU beforehand gives torch.equal output: the kernel's conversion is RNE (a
    truncating kernel differs on about half of the elements of x) and idempotent on bf16 values."""
    M = 129
    x, w, bias, res = linear_inputs(K, N, M, "normal", 600 + K + N)
    assert not torch.equal(x, rounded(x))
    xd, xrd, bd, rd = x.to(device), rounded(x).to(device), bias.to(device), res.to(device)
    wb = pack(lib, device, w.to(device))
    for tile in TILES:
        a = run_linear_bf16(lib, device, xd, wb, bd, rd, M, epi, tile)
        b = run_linear_bf16(lib, device, xrd, wb, bd, rd, M, epi, tile)
        assert torch.equal(a, b), "x is not rounded to nearest even exactly once (tile=%d)" % tile


@pytest.mark.parametrize("family", ["outlier", "one_sign"])
@pytest.mark.parametrize("K,N,epi", [(384, 384, EPI_RESIDUAL), (3072, 768, EPI_RESIDUAL)], ids=["384x384", "3072x768"])
def test_linear_bf16_input_families(lib, device, K, N, epi, family):
    """Outlier K-columns and all-positive operands (no cancellation: the accumulation's worst case, and the case in which a
    matrix unit that truncates against a large running sum would drift), with the residual in place and without a bias."""
    M = 275
    x, w, _, res = linear_inputs(K, N, M, family, 200 + K + N)
    xr, wr = rounded(x), rounded(w)
    ref64, bound = linear_ref64(xr, wr, None, res, epi)
    e32 = linear_e32(xr, wr, None, res, epi, ref64, M, seed=1)
    xd, rd = x.to(device), res.to(device)
    wb = pack(lib, device, w.to(device))
    got = {}
    for tile in TILES:
        got[tile] = run_linear_bf16(lib, device, xd, wb, None, rd, M, epi, tile, in_place=True)
        check_linear(got[tile], ref64, bound, e32, "bf16 linear %dx%d %s in place tile=%d" % (K, N, family, tile))
    assert torch.equal(got[64], got[128])
    assert torch.equal(got[64], run_linear_bf16(lib, device, xd, wb, None, rd, M, epi, 64))


@pytest.mark.parametrize("K,N,epi", [(384, 1152, EPI_BIAS), (384, 384, EPI_RESIDUAL), (384, 1536, EPI_GELU)], ids=lambda v: str(v))
def test_linear_bf16_auto_rule_switches_where_the_fp32_kernel_does(lib, device, K, N, epi):
    """tile_rows = 0 at the last M of the 64-row side and the first M of the 128-row side of the fp32 kernel's rule: the
    profiling row names the instantiation that ran, and the result equals the forced run."""
    below = _switch_rows(N)
    assert -(-below // 128) * (N // 128) < SWITCH <= -(-(below + 1) // 128) * (N // 128)
    x, w, bias, res = linear_inputs(K, N, below + 1, "normal", 300 + K + N)
    xd, bd, rd = x.to(device), bias.to(device), res.to(device)
    wb = pack(lib, device, w.to(device))
    for M, tile in ((below, 64), (below + 1, 128)):
        lib.orbit_prof_enable(1)
        try:
            got = run_linear_bf16(lib, device, xd, wb, bd, rd, M, epi, 0)
            rows = {k: v for k, v in _prof_rows(lib).items() if k.startswith("vit_")}
        finally:
            lib.orbit_prof_enable(0)
        assert rows == {"%s<%d>" % (WHAT[epi], tile): 1}, (M, rows)
        assert torch.equal(got, run_linear_bf16(lib, device, xd, wb, bd, rd, M, epi, tile))
        # the last rows, against float64 on the rounded operands (the whole M x N reference is not needed to see a wrong tail)
        tail = slice(M - 200, M)
        ref64, bound = linear_ref64(rounded(x[tail]), rounded(w), bias, res[tail], epi)
        e32 = linear_e32(rounded(x[tail]), rounded(w), bias, res[tail], epi, ref64, 200, seed=M)
        check_linear(got[tail], ref64, bound, e32, "bf16 linear auto N=%d K=%d M=%d -> <%d>" % (N, K, M, tile))


def test_linear_bf16_refuses_shapes_with_the_shape_in_the_message(lib, device):
    """K % 64 != 0 (a K the fp32 kernel takes) and N % 128 != 0 are argument errors that carry the shape, before any launch."""
    x = torch.zeros(50, 384, device=device)
    wb = torch.zeros(384, 384, dtype=torch.int16, device=device)
    y = torch.full((50, 384), SENTINEL, device=device)
    for N, K in ((384, 96), (384, 352), (192, 384)):
        rc = lib.orbit_op_vit_linear_bf16(_lib.dptr(x), ctypes.c_void_p(wb.data_ptr()), None, None, _lib.dptr(y), 50, N, K, 0, 0,
                                          _st())
        assert rc == -1, rc
        msg = _lib.last_error()
        assert "N=%d" % N in msg and "K=%d" % K in msg and "M=50" in msg, msg
    _sync()
    assert bool((y == SENTINEL).all())
