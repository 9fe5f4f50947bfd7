"""Host side of the device JPEG encoder, no GPU: the encoder's own code (csrc/jpeg_enc_core.h: colour conversion and chroma
downsampling, forward DCT and quantisation, the code walk, byte stuffing - the functions the kernels of csrc/jpeg_enc.hip
call) run serially on the CPU by the stand-alone program tools/jpeg_enc_host_check.cpp, built with AddressSanitizer +
UndefinedBehaviorSanitizer, must write Pillow's file byte for byte; and the host-only entry points of the C-ABI (parameters,
header, bound, argument checks) through ctypes, without a launch. The program is never loaded into Python."""
import ctypes

import pytest

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

import jpeg_cases
from jpeg_enc_cases import SIZES, build_host_check, content, grid, pillow_bytes, run_host_check

ERR_ARG = -1


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_enc_host")
    return build_host_check(str(d)), str(d)


def params(lib, quality, rows):
    p = _lib.JpegEnc()
    assert lib.orbit_jpeg_encode_params(quality, rows, ctypes.byref(p), ctypes.sizeof(p)) == 0, _lib.last_error()
    return p


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_program_writes_pillows_bytes(host_check, size):
    exe, work = host_check
    cases = [c for c in grid() if c[:2] == size]
    assert len(cases) >= 5
    for H, W, quality, kind, rows in cases:
        rc, got, err = run_host_check(exe, content(kind, H, W), quality, rows, work)
        assert rc == 0, (H, W, quality, kind, rows, err[-2000:])
        assert got == pillow_bytes(H, W, quality, kind, rows), (H, W, quality, kind, rows)


def test_grid_holds_every_size_quality_content_and_restart_rows():
    g = grid()
    assert {c[:2] for c in g} == set(SIZES) and {c[2] for c in g} == {100, 95, 75, 30, 1}
    assert {(c[0], c[1], c[3]) for c in g} == {(H, W, k) for H, W in SIZES for k in ("noise", "smooth", "constant", "checker", "redblue")}
    for size in ((18, 22), (37, 53)):
        assert {c[4] for c in g if c[:2] == size} == {0, 1, 2}


def test_host_program_carries_a_comment(host_check):
    exe, work = host_check
    for H, W, rows in ((17, 23, 0), (18, 22, 1)):
        rc, got, err = run_host_check(exe, content("noise", H, W), 95, rows, work, comment="Lavc58.134.100")
        assert rc == 0, err[-2000:]
        assert got == pillow_bytes(H, W, 95, "noise", rows, comment=b"Lavc58.134.100")


def test_header_entry_equals_pillows_header(lib):
    out = (ctypes.c_uint8 * 70000)()
    for H, W, quality, rows, comment in ((37, 53, 95, 0, b""), (224, 224, 75, 1, b""), (18, 22, 30, 2, b"Lavc58.134.100"),
                                        (1, 1, 100, 0, b"x"), (33, 16, 1, 0, bytes(range(256)) * 8)):
        ref = pillow_bytes(H, W, quality, "smooth", rows, comment or None)
        p = params(lib, quality, rows)
        n = lib.orbit_jpeg_encode_header(ctypes.byref(p), H, W, comment or None, len(comment), out, len(out))
        assert n == jpeg_cases.ecs_start(ref), _lib.last_error()
        assert bytes(out[:n]) == ref[:n], (H, W, quality, rows)
        if comment:
            assert ref[20:24] == b"\xff\xfe" + (len(comment) + 2).to_bytes(2, "big") and ref[24:24 + len(comment)] == comment


def test_bound_is_never_below_pillows_file(lib):
    for H, W, quality, kind, rows in grid():
        assert lib.orbit_jpeg_encode_bound(H, W, rows, 0) >= len(pillow_bytes(H, W, quality, kind, rows)), (H, W, quality, kind, rows)
    assert lib.orbit_jpeg_encode_bound(18, 22, 1, 14) >= len(pillow_bytes(18, 22, 95, "noise", 1, b"Lavc58.134.100"))
    assert lib.orbit_jpeg_encode_bound(16, 16, 0, 100) == lib.orbit_jpeg_encode_bound(16, 16, 0, 0) + 104
    assert lib.orbit_jpeg_encode_bound(0, 16, 0, 0) == 0 and lib.orbit_jpeg_encode_bound(16, 16, -1, 0) == 0
    assert lib.orbit_jpeg_encode_workspace_bytes(0, 16, 16) == 0
    assert lib.orbit_jpeg_encode_workspace_bytes(3, 37, 53) == 3 * lib.orbit_jpeg_encode_workspace_bytes(1, 37, 53) > 0


def test_quantisation_tables_follow_jpeg_set_quality(lib):
    from PIL import Image
    import io
    for quality in (100, 95, 75, 50, 49, 30, 1):
        p = params(lib, quality, 0)
        q = Image.open(io.BytesIO(pillow_bytes(16, 16, quality, "smooth", 0))).quantization  # natural order
        assert [list(p.qt[0][:]), list(p.qt[1][:])] == [list(q[0]), list(q[1])]
        for t in range(2):
            for k in range(64):
                d = 8 * p.qt[t][k]
                assert p.qrecip[t][k] == -(-(1 << 32) // d)
    # the reciprocal divides exactly over the whole range of numerators the quantiser meets (< 2^15 + half a divisor)
    for d in sorted({8 * v for v in range(1, 256)}):
        m = -(-(1 << 32) // d)
        assert all((n * m) >> 32 == n // d for n in range(0, 1 << 16, 7)) and ((1 << 16) * m) >> 32 == (1 << 16) // d


def test_every_refusal_is_loud(lib):
    p = _lib.JpegEnc()
    size = ctypes.sizeof(p)
    for args, word in (((0, 0, ctypes.byref(p), size), "quality"), ((101, 0, ctypes.byref(p), size), "quality"),
                       ((95, -1, ctypes.byref(p), size), "restart_rows"), ((95, 0, None, size), "null pointer"),
                       ((95, 0, ctypes.byref(p), size - 4), "p_bytes")):
        assert lib.orbit_jpeg_encode_params(*args) == ERR_ARG and word in _lib.last_error(), (args[:2], _lib.last_error())
    p = params(lib, 95, 0)
    out = (ctypes.c_uint8 * 1024)()
    assert lib.orbit_jpeg_encode_header(None, 16, 16, None, 0, out, 1024) == ERR_ARG and "null pointer" in _lib.last_error()
    assert lib.orbit_jpeg_encode_header(ctypes.byref(p), 16, 16, None, 0, None, 1024) == ERR_ARG and "null pointer" in _lib.last_error()
    big = bytes(65534)
    assert lib.orbit_jpeg_encode_header(ctypes.byref(p), 16, 16, big, len(big), out, 1024) == ERR_ARG and "comment" in _lib.last_error()
    assert lib.orbit_jpeg_encode_header(ctypes.byref(p), 16, 16, None, 0, out, 100) == ERR_ARG and "out holds" in _lib.last_error()
    # the launcher refuses before any launch: the pointers below are never dereferenced
    fake = ctypes.c_void_p(4096)
    H, W, B = 37, 53, 2
    bound, ws = lib.orbit_jpeg_encode_bound(H, W, 0, 0), lib.orbit_jpeg_encode_workspace_bytes(1, H, W)

    def launch(frames=fake, prm=ctypes.byref(p), outp=fake, stride=bound, sizes=fake, wsp=fake, ws_bytes=ws, b=B, offsets=None):
        return lib.orbit_frames_to_jpeg(frames, b, H, W, prm, None, offsets, outp, stride, sizes, wsp, ws_bytes, None)

    for kw, word in (({"frames": None}, "null pointer"), ({"prm": None}, "null pointer"), ({"outp": None}, "null pointer"),
                     ({"sizes": None}, "null pointer"), ({"wsp": None}, "null pointer"), ({"stride": bound - 1}, "out_stride"),
                     ({"ws_bytes": ws - 1}, "workspace"), ({"b": 0}, "bad sizes"),
                     ({"offsets": (ctypes.c_uint32 * 3)(0, 0, 0)}, "null pointer")):
        assert launch(**kw) == ERR_ARG and word in _lib.last_error(), (kw, _lib.last_error())
    blank = _lib.JpegEnc()
    assert launch(prm=ctypes.byref(blank)) == ERR_ARG and "orbit_jpeg_encode_params" in _lib.last_error()
    assert lib.orbit_jpeg_compact(None, bound, fake, B, fake, 1 << 20, fake, None) == ERR_ARG and "null pointer" in _lib.last_error()
    assert lib.orbit_frames_resize_u8(None, 1, 1, 8, 8, 4, 4, 2, fake, None) == ERR_ARG and "null pointer" in _lib.last_error()
    assert lib.orbit_frames_resize_u8(fake, 1, 1, 8, 8, 4, 4, 7, fake, None) == ERR_ARG and "unknown filter" in _lib.last_error()
