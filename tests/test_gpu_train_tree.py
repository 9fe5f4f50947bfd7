"""learner.py --data_path on hardware: meta-training, validation and the finetuner's test loop on an ORBIT JPEG tree.

The tree is written once (ROOT/{train,validation,test}: 2 users x 3 objects x (2 clean + 1 clutter) videos x 50 frames at 64 x 64 -
the target-video floor, and a random way in [2, 3]). With --num_train_tasks 2 an epoch is 4 tasks: at --tasks_per_batch 3 one full
and one partial optimizer step; the query sets are no multiple of --batch_size 16 and the way changes between tasks.

Every comparison between two runs is torch.equal: training is bitwise repeatable (tests/test_gpu_train.py) and the ingest -
8-bit or compressed upload, decode, resize, normalisation - is bit-identical to the host transform (tests/test_gpu_pipeline.py,
test_gpu_resize_pipeline.py, test_gpu_jpeg_pipeline.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import learner  # noqa: E402
from orbit_dataset_amd.data import pipeline  # noqa: E402

MODEL = ["--feature_extractor", "resnet18", "--frame_size", "64", "--batch_size", "16", "--subsample_factor", "5", "--num_workers", "3"]
TRAIN = MODEL + ["--num_lite_samples", "4", "--num_train_tasks", "2", "--tasks_per_batch", "3", "--epochs", "2"]
LITE = ["--with_lite", "--learn_extractor"]
TREE_FIELDS = ("data_path", "decode", "decode_fallback_frames", "stored_frame_size", "train_task_type", "data_wait_ms", "frames_per_task")


def _write(root, splits, seed, frame_size=64):
    for k, split in enumerate(splits):
        pipeline.write_synthetic_orbit_directory(os.path.join(root, split), users=2, objects_per_user=3, clean_videos=2,
                                                 clutter_videos=1, frames_per_video=50, frame_size=frame_size, seed=seed + k)
    return root


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return _write(str(tmp_path_factory.mktemp("orbit_root")), ("train", "validation", "test"), 1991)


def _run(argv):
    """-> (stats, state dict on the host, per-task losses, the state dict before training)"""
    L = learner.Learner(learner.build_parser().parse_args(argv))
    before = {k: v.detach().cpu().clone() for k, v in L.model.state_dict().items()}
    stats = L.run()
    return stats, {k: v.detach().cpu() for k, v in L.model.state_dict().items()}, list(getattr(L, "task_losses", [])), before


def _assert_same_state(got, want):
    assert sorted(got) == sorted(want) and len(got) > 20
    for k in want:
        assert torch.equal(got[k], want[k]), k


def _moved(state, before):
    return [k for k in before if before[k].dtype.is_floating_point and not torch.equal(state[k], before[k])]


@pytest.fixture(scope="module")
def host_run(device, root, tmp_path_factory):
    """--mode train --with_lite --learn_extractor --data_path ROOT with one validation task per user and epoch, --decode host"""
    path = str(tmp_path_factory.mktemp("models") / "A.pt")
    argv = TRAIN + LITE + ["--mode", "train", "--data_path", root, "--num_val_tasks", "1", "--save_model_path", path]
    stats, state, losses, before = _run(argv)
    return {"argv": argv, "stats": stats["train"], "state": state, "losses": losses, "before": before, "path": path}


def _train_on_host_tensors(argv):
    """the same loop, fed from build_dataset("train", frames="float") in train_order order instead of the tree's prefetcher"""
    L = learner.Learner(learner.build_parser().parse_args(argv))
    ds = L.build_dataset("train", frames="float")
    tasks = (ds[i] for epoch in range(L.args.epochs) for i in L.train_order(epoch))
    stats = L.train(task_source=tasks)
    return stats, {k: v.detach().cpu() for k, v in L.model.state_dict().items()}, list(L.task_losses)


def test_training_on_the_tree_equals_the_loop_on_host_tensors(device, root, host_run):
    stats = host_run["stats"]
    assert stats["num_tasks"] == 2 * 2 * 2 and len(host_run["losses"]) == 8  # users x --num_train_tasks x epochs
    assert stats["data_path"] == root and stats["decode"] == "host" and stats["decode_fallback_frames"] is None
    assert stats["stored_frame_size"] == [[64, 64]] and stats["resample"] is None and stats["train_task_type"] == "user_centric"
    assert stats["data_wait_ms"][0] >= 0 and stats["frames_per_task"][0] > 8
    saved = torch.load(host_run["path"], map_location="cpu")
    _assert_same_state(saved, host_run["state"])
    assert len(_moved(host_run["state"], host_run["before"])) > 20
    host_stats, state, losses = _train_on_host_tensors(host_run["argv"][:-2])  # (without --save_model_path)
    assert losses == host_run["losses"]
    _assert_same_state(state, host_run["state"])
    assert host_stats["frames_per_task"] == stats["frames_per_task"] and host_stats["validation"] == stats["validation"]


def test_clips_of_two_frames_on_the_tree_equal_the_loop_on_host_tensors(device, root):
    # (the sampler forms clips of more than one frame for the 'max' clip methods only, as the reference's does)
    argv = TRAIN + LITE + ["--mode", "train", "--data_path", root, "--clip_length", "2", "--train_context_clip_method", "max",
                           "--train_target_clip_method", "max", "--epochs", "1"]
    stats, state, losses, before = _run(argv)
    # at least 2 objects with one clean and one clutter video each: 25 clips of 2 frames per video
    assert stats["train"]["num_tasks"] == 4 and stats["train"]["frames_per_task"][0] >= 2 * 2 * 25 * 2
    _, host_state, host_losses = _train_on_host_tensors(argv)
    assert host_losses == losses
    _assert_same_state(host_state, state)
    assert len(_moved(state, before)) > 20


def test_device_decode_equals_host_decode(device, root, host_run):
    stats, state, losses, _ = _run(host_run["argv"][:-2] + ["--decode", "device"])
    stats = stats["train"]
    assert stats["decode"] == "device" and stats["decode_fallback_frames"] == 0
    assert losses == host_run["losses"]
    _assert_same_state(state, host_run["state"])
    assert stats["validation"] == host_run["stats"]["validation"] and len(stats["validation"]) == 2
    assert stats["frames_per_task"] == host_run["stats"]["frames_per_task"]


def test_device_decode_equals_host_decode_with_a_resize(device, tmp_path):
    big = _write(str(tmp_path / "root96"), ("train",), 7, frame_size=96)
    argv = TRAIN + LITE + ["--mode", "train", "--data_path", big, "--epochs", "1"]
    host, host_state, host_losses, _ = _run(argv + ["--decode", "host"])
    dev, dev_state, dev_losses, _ = _run(argv + ["--decode", "device"])
    for stats in (host["train"], dev["train"]):
        assert stats["stored_frame_size"] == [[96, 96]] and stats["frame_size"] == [64, 64] and stats["resample"] == "lanczos"
    assert dev["train"]["decode_fallback_frames"] == 0
    assert dev_losses == host_losses and len(dev_losses) == 4
    _assert_same_state(dev_state, host_state)


def test_train_test_with_validation_tests_the_final_and_the_best_model(device, root, tmp_path):
    final, best = str(tmp_path / "final.pt"), str(tmp_path / "best.pt")
    stats = learner.main(TRAIN + LITE + ["--mode", "train_test", "--data_path", root, "--num_val_tasks", "1", "--save_model_path", final,
                                         "--save_best_model_path", best])
    history = stats["train"]["validation"]
    assert [h[0] for h in history] == [1, 2] and history[0][2] is True  # one entry per epoch; the first one is the best so far
    assert os.path.exists(best) and os.path.exists(final)
    assert stats["test"]["data_root"] == os.path.join(root, "test") and stats["test"]["num_tasks"] == 2
    test = MODEL + ["--mode", "test", "--data_root", os.path.join(root, "test")]
    same = ("frame_acc", "orbit_metrics", "num_tasks", "target_frames", "data_root", "stored_frame_size")
    for block, path in (("test", final), ("test_best_validation", best)):
        alone = learner.main(test + ["--model_path", path])["test"]
        assert {k: alone[k] for k in same} == {k: stats[block][k] for k in same}, block
    # --data_path ROOT reports what --data_root ROOT/test reports, and --test_set moves it to the validation split
    by_path = learner.main(MODEL + ["--mode", "test", "--data_path", root, "--model_path", final])["test"]
    assert {k: by_path[k] for k in same} == {k: stats["test"][k] for k in same}
    on_val = learner.main(MODEL + ["--mode", "test", "--data_path", root, "--test_set", "validation", "--model_path", final])["test"]
    assert on_val["data_root"] == os.path.join(root, "validation") and on_val["num_tasks"] == 2


@pytest.mark.parametrize("flags,tasks", [(["--adapt_features"], 8),
                                         (LITE + ["--train_task_type", "object_centric", "--num_train_tasks", "1", "--epochs", "1"], 6)],
                         ids=["film-without-lite", "object-centric"])
def test_other_training_forms_run_on_the_tree(device, root, flags, tasks):
    stats, state, losses, before = _run(TRAIN + flags + ["--mode", "train", "--data_path", root])
    stats = stats["train"]
    assert stats["num_tasks"] == len(losses) == tasks and all(l == l for l in losses)
    assert all(k in stats for k in TREE_FIELDS) and stats["data_path"] == root and stats["stored_frame_size"] == [[64, 64]]
    assert stats["train_task_type"] == ("object_centric" if "object_centric" in flags else "user_centric")
    moved = _moved(state, before)
    assert moved and ("--learn_extractor" not in flags or sum(k.startswith("feature_extractor.") for k in moved) > 20)


def test_the_data_is_used(device, host_run, tmp_path):
    other = _write(str(tmp_path / "other"), ("train",), 4242)
    base = TRAIN + LITE + ["--mode", "train"]
    _, other_state, other_losses, _ = _run(base + ["--data_path", other])
    synthetic, synthetic_state, _, _ = _run(base + ["--way", "2", "--shots", "1", "--frames_per_shot", "8", "--num_query_videos", "1",
                                                    "--frames_per_video", "20"])
    assert synthetic["train"]["data_path"] is None and synthetic["train"]["data_wait_ms"] is None
    assert other_losses != host_run["losses"]
    for a, b in ((other_state, host_run["state"]), (other_state, synthetic_state), (synthetic_state, host_run["state"])):
        assert sum(not torch.equal(a[k], b[k]) for k in a) > 20


def test_finetuner_on_the_tree(device, root):
    argv = ["--feature_extractor", "resnet18", "--frame_size", "64", "--batch_size", "16", "--subsample_factor", "5", "--num_workers", "3",
            "--personalize_num_grad_steps", "3", "--data_root", os.path.join(root, "test")]
    host = learner.main_multistep(argv)["test"]
    assert host["data_root"] == os.path.join(root, "test") and host["num_tasks"] == 2 and host["target_frames"] == 2 * 3 * 50
    assert host["orbit_metrics"] is not None and set(host["orbit_metrics"]) == {"user", "object", "task", "video"}
    assert 0.0 <= host["frame_acc"][0] <= 1.0
    dev = learner.main_multistep(argv + ["--decode", "device"])["test"]
    assert dev["decode"] == "device" and dev["decode_fallback_frames"] == 0
    assert dev["frame_acc"] == host["frame_acc"] and dev["orbit_metrics"] == host["orbit_metrics"]
    by_path = learner.main_multistep(argv[:-2] + ["--data_path", root])["test"]
    assert by_path["data_root"] == host["data_root"] and by_path["orbit_metrics"] == host["orbit_metrics"]
