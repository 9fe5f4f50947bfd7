"""Host side of the device JPEG decoder, no GPU: orbit_jpeg_parse against Pillow, and the decoder's own code
(csrc/jpeg_core.h: the walker, inverse DCT, upsampling and colour conversion the kernels of csrc/jpeg.hip call) run on the
CPU by the stand-alone program tools/jpeg_host_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer - on
valid files, where the output must equal Pillow's exactly, and on damaged ones, where it must end cleanly with a status.
The program is never loaded into Python."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import _lib

from jpeg_cases import (ENCODINGS, ROOT, SAMPLING, SIZES, build_host_check, content, damaged_sources, damaged_variants, encode,
                        pillow_rgb, run_host_check)

DESC = ctypes.sizeof(_lib.JpegDesc)


def parse(lib, data):
    d = _lib.JpegDesc()
    return lib.orbit_jpeg_parse(data, len(data), ctypes.byref(d), DESC), d


@pytest.mark.parametrize("enc", sorted(ENCODINGS))
def test_parse_agrees_with_pillow(lib, enc):
    for H, W in ((37, 53), (8, 8), (1, 1)):
        data = encode(content("noise", H, W), enc)
        code, d = parse(lib, data)
        im = Image.open(io.BytesIO(data))
        assert code == 0 and d.status == 0
        assert (d.width, d.height) == im.size and d.ncomp == len(im.layer) == (1 if enc == "gray" else 3)
        for c, (_, hs, vs, tq) in enumerate(im.layer):
            assert (d.hs[c], d.vs[c]) == (hs, vs)
            assert list(d.qt[c][:]) == list(im.quantization[tq])  # both in natural (de-zigzagged) order
        assert (d.hs[0], d.vs[0]) == SAMPLING[enc]
        assert d.restart_interval == (2 if enc == "restart" else 0)
        assert d.ecs_offset + d.ecs_bytes == len(data)
        assert data[:d.ecs_offset].rfind(b"\xff\xda") == d.ecs_offset - (8 + 2 * d.ncomp)  # right behind the SOS header
        # the Huffman tables in decode form reproduce the DHT segments: every code of the look-ahead table decodes to itself
        for slot in (0, 2):
            t = d.huff[slot]
            assert t.maxcode[17] == 0xFFFFF and any(t.look[:])
            for bits in range(256):
                e = t.look[bits]
                if e:
                    length, code8 = e >> 8, bits >> (8 - (e >> 8))
                    assert 1 <= length <= 8 and code8 <= t.maxcode[length] and t.huffval[(t.valptr[length] + code8) & 255] == e & 255


def test_out_of_scope_files_get_a_fallback_code(lib):
    a = content("smooth", 24, 40)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", progressive=True)
    code, d = parse(lib, buf.getvalue())
    assert code == 1 and d.status == 1 and (d.width, d.height, d.ncomp) == (40, 24, 3)  # ORBIT_JPEG_PROGRESSIVE
    buf = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(buf, format="JPEG")
    code, d = parse(lib, buf.getvalue())
    assert code == 5 and d.ncomp == 4  # ORBIT_JPEG_COMPONENTS
    header = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    assert re.search(r"#define\s+ORBIT_JPEG_PROGRESSIVE\s+1\b", header) and re.search(r"#define\s+ORBIT_JPEG_COMPONENTS\s+5\b", header)


def test_not_a_jpeg_is_an_argument_error(lib):
    buf = io.BytesIO()
    Image.fromarray(content("smooth", 8, 8)).save(buf, format="PNG")
    good = encode(content("noise", 24, 40), "default")
    sof = good.index(b"\xff\xc0")
    for data, word in ((buf.getvalue(), "not a JPEG"), (b"", "not a JPEG"), (good[:sof + 7], "past the end"),
                       (good[:good.index(b"\xff\xc4") + 30], "past the end"), (good[:2], "not a JPEG"), (good[:sof], "past the end")):
        code, d = parse(lib, data)
        assert code == -1 and word in _lib.last_error(), (code, _lib.last_error())
    # a length field that points past the buffer, in every header segment of the file
    i = 2
    while good[i + 1] != 0xDA:
        length = (good[i + 2] << 8) | good[i + 3]
        bad = good[:i + 2] + b"\xff\xff" + good[i + 4:]
        assert parse(lib, bad[:i + 4 + 40])[0] == -1
        i += 2 + length


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_host_check"))
    return build_host_check(out), out


@pytest.mark.parametrize("enc", sorted(ENCODINGS))
def test_valid_files_through_the_host_program_equal_pillow(host_check, enc):
    exe, work = host_check
    for H, W in SIZES:
        for kind in ("noise", "smooth"):
            data = encode(content(kind, H, W), enc)
            rc, code, status, pixels, err = run_host_check(exe, data, work)
            assert rc == 0 and err == "", err
            assert code == 0 and status == 0, (H, W, kind, code, status)
            assert np.array_equal(pixels, pillow_rgb(data)), (H, W, kind)


@pytest.mark.parametrize("name", ["420", "444", "gray"])
def test_damaged_files_through_the_host_program(host_check, name):
    """Every variant ends cleanly: exit code 0, nothing from the sanitizers. A cut stream and a removed restart marker cannot
    be decoded, so their status is non-zero. An inverted byte usually breaks the stream as well - but where it leaves a
    well-formed one (the Huffman code resynchronises and every check of the walker holds: all blocks present, restart markers
    in place, EOI behind the last block), a decoder has nothing to report; what is required then is that the pixels are
    again exactly Pillow's for that damaged file."""
    import warnings
    exe, work = host_check
    good = damaged_sources()[name]
    assert run_host_check(exe, good, work)[1:3] == (0, 0)
    broken = 0
    for variant, data in damaged_variants(good).items():
        rc, code, status, pixels, err = run_host_check(exe, data, work)
        assert rc == 0 and err == "", (variant, err)
        assert code == 0
        if variant.startswith("flip") and status == 0:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(pixels, pillow_rgb(data)), variant
        else:
            assert status > 0 and pixels is None, (variant, status)
            broken += 1
    assert broken >= 4 + 5  # the cuts, the marker, and most inverted bytes


def test_gpu_test_damaged_cases_have_a_status_on_the_host(host_check):
    """the two damaged files of tests/test_gpu_jpeg.py and test_gpu_jpeg_pipeline.py"""
    exe, work = host_check
    for name, variant in (("420", "cut50"), ("444", "flip3")):
        rc, code, status, pixels, err = run_host_check(exe, damaged_variants(damaged_sources()[name])[variant], work)
        assert rc == 0 and err == "" and code == 0 and status > 0


def test_entry_points_are_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "orbit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, res, nargs in (("orbit_jpeg_parse", "int", 4), ("orbit_frames_from_jpeg", "int", 11), ("orbit_jpeg_workspace_bytes", "size_t", 3)):
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), code)
        assert len(_lib._SIGNATURES[name][1]) == nargs
    assert re.search(r"#define\s+ORBIT_JPEG_STAGE_BYTES\s+%d\b" % _lib.JPEG_STAGE_BYTES, header)
    # the ctypes mirror of the descriptor: the library refuses any other size
    d = _lib.JpegDesc()
    assert lib.orbit_jpeg_parse(b"\xff\xd8\xff\xd9", 4, ctypes.byref(d), DESC - 4) == -1 and "descriptor" in _lib.last_error()
    assert lib.orbit_jpeg_parse(b"\xff\xd8\xff\xd9", 4, None, DESC) == -1
    sources = open(os.path.join(ROOT, "orbit-dataset_amd", "build.py")).read()
    assert '"jpeg.hip"' in sources


def test_null_and_oversize_arguments_of_the_launcher_are_refused_before_the_gpu(lib):
    """argument checks come first: no device is touched (this runs on a host without one)"""
    P = ctypes.c_void_p
    ok = dict(arena=P(64), arena_bytes=64, descs=P(64), B=1, H=8, W=8, out=P(64), status=P(64), ws=P(64), ws_bytes=1 << 20, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.orbit_frames_from_jpeg(a["arena"], a["arena_bytes"], a["descs"], a["B"], a["H"], a["W"], a["out"], a["status"],
                                          a["ws"], a["ws_bytes"], a["stream"])

    for key in ("arena", "descs", "out", "status", "ws"):
        assert call(**{key: None}) == -1 and "null" in _lib.last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -1 and "sizes" in _lib.last_error()
    assert call(H=1 << 20) == -1 and "limit" in _lib.last_error()
    assert call(arena_bytes=0) == -1 and "arena" in _lib.last_error()
    assert call(ws_bytes=lib.orbit_jpeg_workspace_bytes(1, 8, 8) - 1) == -1 and "workspace" in _lib.last_error()
    assert call(ws=P(72)) == -1 and "aligned" in _lib.last_error()
    assert lib.orbit_jpeg_workspace_bytes(0, 8, 8) == 0 and lib.orbit_jpeg_workspace_bytes(1, 1 << 20, 8) == 0
    # 2 bytes x 64 per coefficient block plus one byte per sample, at the block count of the densest sampling
    assert lib.orbit_jpeg_workspace_bytes(1, 8, 8) == 3 * 2 * 2 * 64 * 3
    assert lib.orbit_jpeg_workspace_bytes(200, 224, 224) == 200 * 3 * 28 * 28 * 64 * 3


def test_decode_flag_and_python_arguments():
    import inspect
    from orbit_dataset_amd import learner
    from orbit_dataset_amd.data import pipeline
    p = learner.build_parser()
    assert p.parse_args([]).decode == "host" and p.parse_args(["--decode", "device"]).decode == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--decode", "gpu"])
    assert inspect.signature(pipeline.DirectoryTaskSource.__init__).parameters["decode"].default == "host"
    with pytest.raises(ValueError, match="decode"):
        pipeline.DirectoryTaskSource(None, decode="gpu")


def test_read_jpeg_frames_parses_and_leaves_out_of_scope_files_to_pil(tmp_path):
    from orbit_dataset_amd.data import pipeline
    H, W = 24, 40
    files = [encode(content("noise", H, W, k), "420") for k in range(3)]
    buf = io.BytesIO()
    Image.fromarray(content("smooth", H, W)).save(buf, format="JPEG", progressive=True)
    files.append(buf.getvalue())
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.jpg" % i)))
        open(paths[-1], "wb").write(f)
    jf = pipeline.read_jpeg_frames(paths, lead=(2, 2))
    assert jf.shape == (2, 2, H, W, 3) and jf.codes == [0, 0, 0, 1] and list(jf.pixels) == [3] and jf.files == files
    assert np.array_equal(jf.pixels[3], pillow_rgb(files[3]))
    both = pipeline.JpegFrames.cat([jf.flatten(end_dim=1), jf.flatten(end_dim=1)]).unsqueeze(1)
    assert both.shape == (8, 1, H, W, 3) and sorted(both.pixels) == [3, 7] and len(both) == 8
    open(paths[0], "wb").write(encode(content("noise", 8, 8), "420"))
    with pytest.raises(ValueError, match="different sizes"):
        pipeline.read_jpeg_frames(paths)
