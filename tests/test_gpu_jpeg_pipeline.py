"""decode="device" through the input pipeline: TaskPrefetcher fed with JpegFrames yields clips torch.equal to the ones it
yields from PIL-decoded frames - with and without --frame_size, with an out-of-scope file and with damaged files in the
tree - and learner.py --mode test --decode device reports what --decode host reports."""
import glob
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd.data import pipeline  # noqa: E402

from jpeg_cases import damaged_variants  # noqa: E402


def _write_tree(root, **kw):
    pipeline.write_synthetic_orbit_directory(root, users=1, objects_per_user=2, clean_videos=2, clutter_videos=1,
                                             frames_per_video=4, **kw)
    return root


@pytest.fixture(scope="module")
def tree224(tmp_path_factory):
    return _write_tree(str(tmp_path_factory.mktemp("orbit224")), frame_size=224)


def _collect(tree, device, decode, **kw):
    source = pipeline.DirectoryTaskSource(pipeline.ORBITDirectory(tree), workers=4, decode=decode)
    pf = pipeline.TaskPrefetcher(source, device, depth=2, **kw)
    out = [{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in t.items()} for t in pf]
    pf.close()
    return out, pf


def _assert_same_tasks(got, want):
    assert len(got) == len(want) >= 1
    for g, w in zip(got, want):
        for key in ("context_clips", "target_clips"):
            assert g[key].is_cuda and g[key].dtype == torch.float32 and torch.equal(g[key], w[key])
        assert torch.equal(g["context_labels"], w["context_labels"]) and g["target_videos"] == w["target_videos"]


def test_prefetcher_device_decode_equals_host_decode(device, tree224):
    host, _ = _collect(tree224, device, "host")
    dev, pf = _collect(tree224, device, "device")
    _assert_same_tasks(dev, host)
    assert dev[0]["context_clips"].shape == (16, 1, 3, 224, 224) and dev[0]["target_clips"].shape == (8, 1, 3, 224, 224)
    assert pf.fallback_frames == 0 and pf.device_frames == 24 and dev[0]["decode_fallbacks"] == 0
    # 224 -> 84, lanczos: the resize reads the decoder's 8-bit buffer
    host84, _ = _collect(tree224, device, "host", frame_size=84)
    dev84, pf = _collect(tree224, device, "device", frame_size=84)
    _assert_same_tasks(dev84, host84)
    assert dev84[0]["context_clips"].shape == (16, 1, 3, 84, 84) and pf.fallback_frames == 0 and pf.stored_sizes == {(224, 224)}


def test_prefetcher_with_out_of_scope_and_damaged_files(device, tmp_path):
    from PIL import Image
    tree = _write_tree(str(tmp_path / "tree"), frame_size=64, quality=95)
    files = sorted(glob.glob(os.path.join(tree, "*", "*", "*", "*", "*.jpg")))
    assert len(files) == 24
    Image.open(files[1]).save(files[1], progressive=True)  # out of scope: PIL decodes it at staging
    # an inverted byte the walker reports (the same rule as jpeg_cases.damaged_variants, restart markers apart)
    Image.open(files[5]).save(files[5], quality=95, restart_marker_blocks=2)
    data = open(files[5], "rb").read()
    open(files[5], "wb").write(damaged_variants(data)["flip3"])
    host, _ = _collect(tree, device, "host")
    dev, pf = _collect(tree, device, "device")
    _assert_same_tasks(dev, host)
    assert pf.fallback_frames == 2 and pf.device_frames == 22 and dev[0]["decode_fallbacks"] == 2
    # a cut file: PIL raises, on either path, out of __next__
    open(files[9], "wb").write(damaged_variants(data)["cut50"])
    for decode in ("host", "device"):
        with pytest.raises(OSError):
            _collect(tree, device, decode)


def test_learner_reports_the_same_with_device_decode(device, tmp_path, capsys):
    from orbit_dataset_amd import learner
    tree = str(tmp_path / "tree")
    pipeline.write_synthetic_orbit_directory(tree, users=1, objects_per_user=2, clean_videos=2, clutter_videos=1,
                                             frames_per_video=50, frame_size=64)
    base = ["--mode", "test", "--feature_extractor", "resnet18", "--data_root", tree, "--num_workers", "3", "--subsample_factor", "5",
            "--batch_size", "16", "--frame_size", "64"]
    host = learner.main(base + ["--decode", "host"])["test"]
    dev = learner.main(base + ["--decode", "device"])["test"]
    assert host["decode"] == "host" and host["decode_fallback_frames"] is None
    assert dev["decode"] == "device" and dev["decode_fallback_frames"] == 0
    assert dev["frame_acc"] == host["frame_acc"] and dev["orbit_metrics"] == host["orbit_metrics"]
    assert dev["target_frames"] == host["target_frames"] == 2 * 1 * 50 and dev["stored_frame_size"] == [[64, 64]]
    assert "JPEG decode on the GPU" in capsys.readouterr().out
