"""The annotation filters and loaded annotations through the tree loops on hardware: the existing device paths (8-bit upload,
device JPEG decode, LITE training, the finetuner) consume filtered tasks unchanged.

Tree F (F/train = F/test: 2 users x 3 objects x (2 clean + 2 clutter) videos x 60 frames at 64 x 64) is annotated by explicit rules:
most clutter videos lose 5-10 frames without the object, one loses 15 (45 left: below the target floor, dropped), one object
loses 12 on both clutter videos (dropped with its clean videos), one clean video has 4 blurred frames and one 2 frames without
the object (what `no_blur_issue` drops from the context set). Tree P is a copy with every frame the filters drop deleted and no
annotations at all: a filtered run on F must equal the plain run on P.

Every comparison is torch.equal or equality of lists: the loops are bitwise repeatable and the ingest equals the host transform
(tests/test_gpu_train_tree.py, test_gpu_pipeline.py, test_gpu_jpeg_pipeline.py pin that); no tolerance is introduced."""
import json
import os
import shutil

import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import learner  # noqa: E402
from orbit_dataset_amd.data import pipeline  # noqa: E402

MODEL = ["--feature_extractor", "resnet18", "--frame_size", "64", "--batch_size", "16", "--subsample_factor", "5", "--num_workers", "3"]
ONP = "no_object_not_present_issue"
FRAMES = 60


def _name(u, o, kind, v):
    return "P%03d--obj%02d--%s--%02d" % (u, o, kind, v)


# frames (0-based) without the object, per video
ABSENT = {_name(0, 0, "clutter", 0): range(2, FRAMES, 12),   # 5
          _name(0, 0, "clutter", 1): range(0, FRAMES, 6),    # 10 -> 50 left: exactly the floor
          _name(0, 1, "clutter", 0): range(5, FRAMES, 9),    # 7
          _name(0, 1, "clutter", 1): range(0, FRAMES, 4),    # 15 -> 45 left: dropped
          _name(0, 2, "clutter", 0): range(1, FRAMES, 10),   # 6
          _name(0, 2, "clutter", 1): range(50, 58),          # 8
          _name(1, 0, "clutter", 0): range(3, FRAMES, 11),   # 6
          _name(1, 0, "clutter", 1): (0, 1, 2, 30, 59),      # 5
          _name(1, 1, "clutter", 0): range(4, FRAMES, 8),    # 7
          _name(1, 1, "clutter", 1): range(0, FRAMES, 7),    # 9
          _name(1, 2, "clutter", 0): range(0, FRAMES, 5),    # 12 -> 48 left: dropped ...
          _name(1, 2, "clutter", 1): range(2, FRAMES, 5),    # 12 -> 48 left: ... and with both the object
          _name(1, 0, "clean", 1): (0, 1)}
ISSUES = {_name(0, 0, "clean", 0): {"blur_issue": (3, 4, 5, 20)}}
ABSENT_COUNT = {k: len(list(v)) for k, v in ABSENT.items()}


def _prune(root, split, kinds):
    """delete from root/<split> the frames of the videos of `kinds` that the rules above mark: without the object (clutter and
    clean), or blurred (clean)"""
    removed = 0
    for u in range(2):
        for o in range(3):
            for kind in kinds:
                for v in range(2):
                    name = _name(u, o, kind, v)
                    gone = set(ABSENT.get(name, ())) | set(ISSUES.get(name, {}).get("blur_issue", ()))
                    for k in gone:
                        os.remove(os.path.join(root, split, "P%03d" % u, "obj%02d" % o, kind, name, "%s-%05d.jpg" % (name, k + 1)))
                        removed += 1
    return removed


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """-> (F, P): F/{train,test} annotated, P/test without the clutter frames the target filter drops, P/train also without the
    clean frames `no_blur_issue` drops; P has no annotations/ directory"""
    F, P = (str(tmp_path_factory.mktemp(n)) for n in ("orbit_F", "orbit_P"))
    pipeline.write_synthetic_orbit_directory(os.path.join(F, "test"), users=2, objects_per_user=3, clean_videos=2, clutter_videos=2,
                                             frames_per_video=FRAMES, frame_size=64, seed=1616)
    pipeline.write_synthetic_orbit_annotations(os.path.join(F, "test"), absent=ABSENT, issues=ISSUES)
    shutil.copytree(os.path.join(F, "test"), os.path.join(F, "train"))
    shutil.copytree(os.path.join(F, "annotations", "test"), os.path.join(F, "annotations", "train"))
    for split in ("train", "test"):
        shutil.copytree(os.path.join(F, split), os.path.join(P, split))
    assert _prune(P, "test", ("clutter",)) == sum(n for k, n in ABSENT_COUNT.items() if "clutter" in k) == 102
    assert _prune(P, "train", ("clutter", "clean")) == 102 + 2 + 4
    return F, P


def _test(argv, out=None):
    stats = learner.main(MODEL + ["--mode", "test"] + argv + (["--save_predictions", out] if out else []))["test"]
    if out is None:
        return stats, None
    with open(os.path.join(out, "results.json")) as f:
        return stats, json.load(f)


SAME = ("frame_acc", "orbit_metrics", "num_tasks", "target_frames", "stored_frame_size")
# target videos x frames the filter leaves: P000 5 videos (55 + 50 + 53 + 54 + 52), P001 4 videos (54 + 55 + 53 + 51)
FILTERED_FRAMES = 264 + 213


@pytest.fixture(scope="module")
def filtered_run(device, trees, tmp_path_factory):
    return _test(["--data_path", trees[0], "--test_filter_target", ONP], str(tmp_path_factory.mktemp("pred_F")))


def test_filtered_test_loop_equals_the_pruned_tree(device, trees, filtered_run, tmp_path):
    F, P = trees
    stats, predictions = filtered_run
    plain, plain_predictions = _test(["--data_path", P], str(tmp_path / "pred_P"))
    assert stats["target_frames"] == FILTERED_FRAMES and stats["num_tasks"] == 2 and stats["orbit_metrics"] is not None
    assert {k: stats[k] for k in SAME} == {k: plain[k] for k in SAME}
    assert predictions == plain_predictions and len(predictions) > 0
    assert stats["filter_target"] == [ONP] and stats["filter_context"] == [] and stats["annotations_to_load"] == []
    assert stats["index"] == {"kept": {"users": 2, "objects": 5, "context_videos": 10, "target_videos": 9,
                                       "context_frames": 10 * FRAMES, "target_frames": FILTERED_FRAMES},
                              "dropped": {"users": 0, "objects": 1, "context_videos": 2, "target_videos": 3,
                                          "context_frames": 2 * FRAMES, "target_frames": 12 * FRAMES - FILTERED_FRAMES}}
    assert plain["index"]["kept"] == stats["index"]["kept"] and plain["index"]["dropped"] is None and plain["filter_target"] == []


def test_filtered_test_loop_with_device_decode(device, trees, filtered_run, tmp_path):
    stats, predictions = filtered_run
    dev, dev_predictions = _test(["--data_path", trees[0], "--test_filter_target", ONP, "--decode", "device"], str(tmp_path / "pred_dev"))
    assert dev["decode"] == "device" and dev["decode_fallback_frames"] == 0
    assert {k: dev[k] for k in SAME} == {k: stats[k] for k in SAME} and dev_predictions == predictions
    assert dev["index"] == stats["index"]


def test_without_the_flag_the_same_tree_yields_more_frames(device, trees, filtered_run):
    stats, _ = filtered_run
    plain, _ = _test(["--data_path", trees[0]])
    assert plain["target_frames"] == 12 * FRAMES > stats["target_frames"]
    assert plain["index"] == {"kept": {"users": 2, "objects": 6, "context_videos": 12, "target_videos": 12,
                                       "context_frames": 12 * FRAMES, "target_frames": 12 * FRAMES}, "dropped": None}


def _train(argv):
    L = learner.Learner(learner.build_parser().parse_args(
        MODEL + ["--mode", "train", "--with_lite", "--learn_extractor", "--num_lite_samples", "4", "--epochs", "1",
                 "--num_train_tasks", "2"] + argv))
    stats = L.run()["train"]
    return stats, {k: v.detach().cpu() for k, v in L.model.state_dict().items()}, list(L.task_losses)


def test_filtered_training_equals_the_pruned_tree(device, trees):
    F, P = trees
    stats, state, losses = _train(["--data_path", F, "--train_filter_context", "no_blur_issue", "--train_filter_target", ONP])
    plain, plain_state, plain_losses = _train(["--data_path", P])
    assert len(losses) == 4 and losses == plain_losses and all(l == l for l in losses)
    assert sorted(state) == sorted(plain_state) and len(state) > 20
    for k in state:
        assert torch.equal(state[k], plain_state[k]), k
    assert stats["frames_per_task"] == plain["frames_per_task"]
    assert stats["filter_context"] == ["no_blur_issue"] and stats["filter_target"] == [ONP]
    assert stats["index"]["kept"] == plain["index"]["kept"] and plain["index"]["dropped"] is None
    assert stats["index"]["dropped"] == {"users": 0, "objects": 1, "context_videos": 2, "target_videos": 3,
                                         "context_frames": 2 * FRAMES + 6, "target_frames": 12 * FRAMES - FILTERED_FRAMES}


def test_filtered_finetuner_equals_the_pruned_tree(device, trees):
    F, P = trees
    argv = MODEL + ["--personalize_num_grad_steps", "2"]
    got = learner.main_multistep(argv + ["--data_path", F, "--test_filter_target", ONP])["test"]
    plain = learner.main_multistep(argv + ["--data_path", P])["test"]
    assert got["target_frames"] == FILTERED_FRAMES and got["orbit_metrics"] is not None
    assert {k: got[k] for k in SAME} == {k: plain[k] for k in SAME}
    assert got["filter_target"] == [ONP] and got["index"]["kept"] == plain["index"]["kept"]
    assert got["index"]["dropped"]["objects"] == 1 and got["index"]["dropped"]["target_videos"] == 3


@pytest.mark.parametrize("filtered", [False, True], ids=["loaded", "loaded-and-filtered"])
def test_annotations_ride_through_the_prefetcher_on_the_host(device, trees, filtered):
    F, key = trees[0], "object_not_present_issue"
    argv = MODEL + ["--mode", "test", "--data_path", F, "--annotations_to_load", key] + (["--test_filter_target", ONP] if filtered else [])
    L = learner.Learner(learner.build_parser().parse_args(argv))
    prefetch = L._prefetch(L.build_dataset("test"), [0, 1], depth=3)
    seen = 0
    try:
        for task in prefetch:
            ann = task["target_annotations"][key]
            assert not ann.is_cuda and ann.dtype == torch.float32 and ann.shape == (len(task["target_clips"]), 1)
            assert task["target_clips"].is_cuda and not task["context_annotations"][key].is_cuda
            assert task["context_annotations"][key].shape == (len(task["context_clips"]), 1, 1)
            want = []
            for paths in task["target_paths"]:
                with open(os.path.join(F, "annotations", "test", os.path.basename(os.path.dirname(paths[0])) + ".json")) as f:
                    anns = json.load(f)
                want += [float(anns[os.path.basename(p)][key]) for p in paths]
            assert ann.reshape(-1).tolist() == want and len(want) == task["target_videos"][-1][1]
            assert (sum(want) == 0) if filtered else (0 < sum(want) < len(want))
            seen += 1
    finally:
        prefetch.close()
        L._close_decode_pool()
    assert seen == 2
    stats = L.test()  # the loop runs on such tasks as on any other
    assert stats["annotations_to_load"] == [key] and stats["target_frames"] == (FILTERED_FRAMES if filtered else 12 * FRAMES)
