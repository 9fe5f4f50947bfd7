"""tools/resize_videos.py: the reference's offline pass (scripts/resize_videos.py: PIL open -> convert('RGB') -> resize
LANCZOS -> save(quality=95)) with decode, resize and encode on the device writes the same tree, file for file and byte for
byte - with a source that carries a comment, a progressive one (decoded by PIL on the host) and a grayscale one - and with
--restart_rows 1 the files PIL writes with restart_marker_rows=1, which learner.py then decodes on the device."""
import glob
import io
import json
import os
import subprocess
import sys

import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd.data import pipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 32


def reference_bytes(path, **kw):
    """what the reference's script writes for one source file"""
    im = Image.open(path)
    if im.mode != "RGB":
        im = im.convert("RGB")
    buf = io.BytesIO()
    im.resize((SIZE, SIZE), resample=Image.LANCZOS).save(buf, format="JPEG", quality=95, **kw)
    return buf.getvalue()


def run_tool(src, dst, *flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resize_videos.py"), "--data_path", src, "--save_path", dst,
                        "--size", str(SIZE), "--nthreads", "4", "--batch", "16", *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "frames/s" in r.stdout and "host-decoded" in r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


def write_tree(root, clean_videos, frames_per_video):
    """a 64 x 48 tree with a commented, a progressive and a grayscale file and one already at the target size"""
    n = pipeline.write_synthetic_orbit_directory(root, users=1, objects_per_user=2, clean_videos=clean_videos, clutter_videos=1,
                                                 frames_per_video=frames_per_video, frame_size=64)
    files = sorted(glob.glob(os.path.join(root, "*", "*", "*", "*", "*.jpg")))
    assert len(files) == n >= 42
    for f in files:  # 64 wide, 48 high
        Image.open(f).resize((64, 48), Image.BILINEAR).save(f, quality=90)
    Image.open(files[2]).save(files[2], quality=90, comment=b"Lavc58.134.100")
    Image.open(files[11]).save(files[11], quality=90, progressive=True)
    Image.open(files[20]).convert("L").save(files[20], quality=90)
    Image.open(files[30]).resize((SIZE, SIZE)).save(files[30], quality=90)  # already at --size: re-encoded all the same
    return root, files


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("raw")), 2, 7)


def test_default_flags_reproduce_the_reference_tree(device, tree, tmp_path):
    root, files = tree
    out = str(tmp_path / "out")
    stats = run_tool(root, out)
    assert stats["frames"] == len(files) and stats["host_decoded"] == 1  # the progressive file
    written = sorted(glob.glob(os.path.join(out, "**", "*.jpg"), recursive=True))
    assert [os.path.relpath(f, out) for f in written] == [os.path.relpath(f, root) for f in files]
    for src, dst in zip(files, written):
        with open(dst, "rb") as f:
            assert f.read() == reference_bytes(src), os.path.relpath(src, root)
    with open(os.path.join(out, os.path.relpath(files[2], root)), "rb") as f:
        assert b"\xff\xfe\x00\x10Lavc58.134.100" in f.read()[:64]


def test_restart_rows_tree_is_decoded_on_the_device(device, tmp_path):
    root, files = write_tree(str(tmp_path / "raw"), 1, 50)  # (the directory reader takes target videos of 50 frames or more)
    out = str(tmp_path / "out_rst")
    stats = run_tool(root, out, "--restart_rows", "1")
    assert stats["host_decoded"] == 1
    for src in files:
        with open(os.path.join(out, os.path.relpath(src, root)), "rb") as f:
            data = f.read()
        assert data == reference_bytes(src, restart_marker_rows=1), os.path.relpath(src, root)
        assert b"\xff\xdd\x00\x04\x00\x02" in data  # DRI: 1 row x 2 MCUs
    from orbit_dataset_amd import learner
    test = learner.main(["--mode", "test", "--feature_extractor", "resnet18", "--data_root", out, "--num_workers", "2",
                         "--subsample_factor", "5", "--batch_size", "16", "--frame_size", str(SIZE), "--decode", "device"])["test"]
    assert test["decode"] == "device" and test["decode_fallback_frames"] == 0 and test["stored_frame_size"] == [[SIZE, SIZE]]
    assert test["target_frames"] == 2 * 50
