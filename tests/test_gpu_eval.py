"""orbit_video_metrics (csrc/eval.hip) and the evaluators on it, on hardware. Every kernel case compares EXACTLY - integer
equality, no tolerance - with np.argmax / np.bincount / np.where on the same float32 logits; the end-to-end cases drive
TestEvaluator over fixture G15_eval (the reference's own statistics and results.json) and Learner.test()."""
import ctypes
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402
from orbit_dataset_amd.utils import eval_metrics  # noqa: E402
from orbit_dataset_amd.utils.eval_metrics import TestEvaluator  # noqa: E402

import eval_golden  # noqa: E402


def _run(device, logits, sizes, labels, want_preds=True):
    """the launch on `logits` [M, C] (numpy float32) cut into videos of `sizes` frames -> host (correct, first, hist, preds)"""
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out, V, C = eval_metrics.video_metrics(torch.from_numpy(logits).to(device), offsets, labels, want_preds)
    assert out.dtype == torch.int32 and out.numel() == 2 * V + V * C + (len(logits) if want_preds else 0)
    return eval_metrics.split_video_metrics(out.cpu().numpy(), V, C, M=len(logits) if want_preds else None)


def _check(device, logits, sizes, labels, want_preds=True):
    correct, first, hist, preds = _run(device, logits, sizes, labels, want_preds)
    lo = 0
    for v, (n, label) in enumerate(zip(sizes, labels)):
        p, c, f, h = eval_golden.numpy_integers(logits[lo:lo + n], label)
        what = "video %d (n = %d, label %d)" % (v, n, label)
        assert correct[v] == c, what
        assert first[v] == f, what
        assert np.array_equal(hist[v], h), what
        if want_preds:
            assert np.array_equal(preds[lo:lo + n], p), what
        lo += n
    return correct, first, hist, preds


@pytest.mark.parametrize("C", [1, 2])
def test_one_frame(device, C):
    logits = np.array([[0.25, 0.5][:C]], dtype=np.float32)
    correct, first, hist, preds = _check(device, logits, [1], [C - 1])
    assert correct.tolist() == [1] and first.tolist() == [0] and preds.tolist() == [C - 1]


@pytest.mark.parametrize("C", [5, 10, 64, 65])
def test_ragged_videos_across_the_block_stride(device, C):
    """63 / 64 / 65 frames (one wave, its edge), 257 and 1025 (the block loops twice and five times) and an empty video"""
    sizes = [63, 0, 64, 65, 257, 1025]
    rng = np.random.default_rng(C)
    logits = rng.standard_normal((sum(sizes), C)).astype(np.float32)
    labels = rng.integers(0, C, len(sizes)).tolist()
    lo = 0
    for n, label in zip(sizes, labels):  # half of every video's frames are won by its label
        logits[lo:lo + n:2, label] += 4.0
        lo += n
    correct, first, hist, _ = _check(device, logits, sizes, labels)
    assert correct[1] == 0 and first[1] == 0 and not hist[1].any()  # the empty video
    assert hist.sum(1).tolist() == sizes
    correct2, first2, hist2, preds2 = _check(device, logits, sizes, labels, want_preds=False)  # preds = NULL
    assert preds2 is None and np.array_equal(correct, correct2) and np.array_equal(first, first2) and np.array_equal(hist, hist2)


def test_labels_outside_the_columns_match_no_frame(device):
    C, sizes = 5, [7, 7]
    logits = np.random.default_rng(3).standard_normal((14, C)).astype(np.float32)
    correct, first, hist, _ = _check(device, logits, sizes, [-1, C])
    assert correct.tolist() == [0, 0] and first.tolist() == sizes and hist.sum() == 14


def test_argmax_rule_and_histogram_tie(device):
    C = 5
    flat = np.full((3, C), 1.5, dtype=np.float32)                       # all columns equal: column 0
    last = np.tile(np.arange(C, dtype=np.float32), (3, 1))               # the maximum is the last column
    pair = np.zeros((4, C), dtype=np.float32)                            # exact ties between two columns: the lower one
    pair[:, [1, 3]] = 2.0
    tie = np.zeros((64, C), dtype=np.float32)                            # 32 frames of class 2, 32 of class 4
    tie[::2, 2] = 1.0
    tie[1::2, 4] = 1.0
    logits = np.concatenate([flat, last, pair, tie])
    correct, first, hist, preds = _check(device, logits, [3, 3, 4, 64], [0, C - 1, 3, 4])
    assert preds[:10].tolist() == [0] * 3 + [C - 1] * 3 + [1] * 4
    assert correct.tolist() == [3, 3, 0, 32] and first.tolist() == [0, 0, 4, 1]
    assert hist[3].tolist() == [0, 0, 32, 0, 32] and int(np.argmax(hist[3])) == 2  # bincount().argmax(): the lower class


def test_no_frames_is_a_no_op(device, lib):
    buf = torch.full((16,), -7, dtype=torch.int32, device=device)
    logits = torch.zeros(1, 5, device=device)
    offsets, labels = torch.zeros(2, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int64, device=device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.orbit_video_metrics(P(logits), 0, 5, P(offsets), P(labels), 1, None, P(buf), P(buf), P(buf), _lib.stream_handle()) == 0
    assert lib.orbit_video_metrics(P(logits), 1, 5, P(offsets), P(labels), 0, None, P(buf), P(buf), P(buf), _lib.stream_handle()) == 0
    assert buf.cpu().tolist() == [-7] * 16
    # rejected arguments: return codes only
    assert lib.orbit_video_metrics(P(logits), 1, 0, P(offsets), P(labels), 1, None, P(buf), P(buf), P(buf), None) == -1
    assert lib.orbit_video_metrics(P(logits), 1, 1 << 20, P(offsets), P(labels), 1, None, P(buf), P(buf), P(buf), None) == -1
    assert lib.orbit_video_metrics(None, 1, 5, P(offsets), P(labels), 1, None, P(buf), P(buf), P(buf), None) == -1


def test_preds_equal_the_heads_argmax(device):
    """one 5-way task: the head's fused `argmax` output and the metrics kernel's predictions come from one device function"""
    from orbit_dataset_amd.model.classifier_heads import PrototypicalClassifier
    g = torch.Generator().manual_seed(11)
    feats, labels = torch.randn(50, 512, generator=g), torch.arange(5).repeat(10)
    queries = torch.randn(200, 512, generator=g)
    queries[:8] = 0.0  # a zero query scores every class by its bias alone
    head = PrototypicalClassifier(1.0, "euclidean")
    head.configure(feats.to(device), labels.to(device))
    logits, amax = head.predict(queries.to(device), return_argmax=True)
    out, V, C = eval_metrics.video_metrics(logits, [0, 200], [2])
    _, _, hist, preds = eval_metrics.split_video_metrics(out.cpu().numpy(), V, C, M=200)
    assert np.array_equal(preds, amax.cpu().numpy().reshape(-1))
    assert np.array_equal(preds, logits.cpu().numpy().argmax(-1)) and hist.sum() == 200


def _prof_rows(lib):
    lib.orbit_prof_collect(None, None, None)
    buf, n = ctypes.create_string_buffer(48), ctypes.c_long(0)
    rows = {}
    for i in range(lib.orbit_prof_num_variants()):
        lib.orbit_prof_variant(i, buf, ctypes.byref(n), None, None, None)
        rows[buf.value.decode()] = rows.get(buf.value.decode(), 0) + n.value
    return rows


def test_golden_through_the_device_evaluator(device, lib, tmp_path):
    """G15_eval through TestEvaluator.append_video on device logits: the reference's statistics to 1e-12 (float64 ratios of the
    same integers), its results.json content, and one launch per task."""
    golden = eval_golden.load()
    names = [str(s) for s in golden["stat_names"]]

    def append(ev, v):
        ev.append_video(torch.from_numpy(v["logits"]).to(device), torch.tensor(v["label"]), np.array(v["paths"]))

    lib.orbit_prof_enable(1)
    try:
        ev = eval_golden.drive(TestEvaluator(names, save_dir=str(tmp_path)), golden, append)
        got = eval_golden.stats_array(ev.get_mean_stats(), names)
        rows = _prof_rows(lib)
    finally:
        lib.orbit_prof_enable(0)
    assert rows.get("video_metrics") == 4, rows  # 2 users x 2 tasks
    print("max |stat - reference| = %.3g" % np.abs(got - golden["stats"]).max())
    assert np.abs(got - golden["stats"]).max() <= 1e-12
    assert np.abs(eval_golden.stats_array(ev.get_mean_stats(current_user=True), names) - golden["stats_last_user"]).max() <= 1e-12
    video, _ = ev.get_video_and_object_stats()
    assert abs(video["video_acc"][0] - golden["video_acc"].mean()) <= 1e-12
    ev.save()
    results = json.load(open(tmp_path / "results.json"))
    assert list(results) == golden["users"]
    assert np.array_equal(eval_golden.flat_results(results, golden["users"]), golden["results_flat"])


def test_per_frame_labels_are_cut_into_runs(device):
    """a video appended with one label per frame: frame statistics of the concatenation, every run in its own object"""
    rng = np.random.default_rng(21)
    logits = rng.standard_normal((40, 4)).astype(np.float32)
    labels = np.repeat([2, 0, 2], [10, 25, 5])
    ev = TestEvaluator(["frame_acc", "frames_to_recognition"])
    ev.append_video(torch.from_numpy(logits).to(device), torch.from_numpy(labels))
    ev.append_video(torch.from_numpy(logits[:9]).to(device), torch.tensor(1))
    user, obj, task, video = ev.get_mean_stats()
    preds = logits.argmax(-1)
    hits, hits1 = np.where(preds == labels)[0], np.where(preds[:9] == 1)[0]
    want = [len(hits) / 40, len(hits1) / 9]
    assert abs(video["frame_acc"][0] - np.mean(want)) <= 1e-15
    assert task["frame_acc"][0] == (len(hits) + len(hits1)) / 49 == user["frame_acc"][0]
    per_object = [np.mean(preds[labels == 2] == 2), np.mean(preds[labels == 0] == 0), len(hits1) / 9]  # first appearance: 2, 0, 1
    assert abs(obj["frame_acc"][0] - np.mean(per_object)) <= 1e-15
    assert video["frames_to_recognition"][0] == np.mean([hits[0] / 40, hits1[0] / 9 if len(hits1) else 1.0])
    video_acc, _ = ev.get_video_and_object_stats()
    assert video_acc["video_acc"][0] == float(np.bincount(preds[:9]).argmax() == 1)  # only the video that has a video label


def test_train_evaluator_on_device_logits(device):
    from orbit_dataset_amd.utils.eval_metrics import TrainEvaluator
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((70, 5)).astype(np.float32)
    labels = np.repeat([3, 1, 1, 4], [20, 5, 25, 20])
    ev = TrainEvaluator(["frame_acc", "frames_to_recognition"])
    ev.update_stats(torch.from_numpy(logits).to(device), torch.from_numpy(labels))
    hits = np.where(logits.argmax(-1) == labels)[0]
    assert ev.get_current_stats() == {"frame_acc": len(hits) / 70, "frames_to_recognition": hits[0] / 70}
    assert ev.get_mean_stats()["frame_acc"] == [len(hits) / 70, 0.0]


def test_learner_reports_orbit_metrics(device, capsys):
    """Learner.test() on two synthetic tasks: the new key beside the old ones; its video-level frame accuracy is the mean of the
    per-video accuracies the existing path averages (a float32 mean there: 1e-6)."""
    from orbit_dataset_amd import learner
    args = learner.build_parser().parse_args(
        ["--mode", "test", "--feature_extractor", "resnet18", "--frame_size", "32", "--way", "3", "--shots", "1",
         "--frames_per_shot", "2", "--num_query_videos", "3", "--frames_per_video", "7", "--num_test_tasks", "2", "--batch_size", "16"])
    stats = learner.Learner(args).test()
    assert {"frame_acc", "personalise_ms", "inference_ms_per_frame", "num_tasks", "world_size"} <= set(stats)
    report = stats["orbit_metrics"]
    assert set(report) == {"user", "object", "task", "video"}
    assert set(report["task"]) == set(report["user"]) == {"frame_acc", "frames_to_recognition"}
    # (a synthetic "video" mixes objects - it is fed with one label per frame and has no video accuracy; every object has)
    assert set(report["object"]) == {"frame_acc", "frames_to_recognition", "video_acc"}
    assert {"frame_acc", "frames_to_recognition"} <= set(report["video"])
    # every task has 3 videos, so the mean over tasks of the mean over videos is the mean over the 6 videos
    assert abs(report["video"]["frame_acc"][0] - stats["frame_acc"][0]) <= 1e-6
    # one user is one task in synthetic mode, every video has 7 frames: per user == per task == (here) per video
    assert report["user"]["frame_acc"] == report["task"]["frame_acc"]
    assert abs(report["task"]["frame_acc"][0] - report["video"]["frame_acc"][0]) <= 1e-12
    out = capsys.readouterr().out
    assert "test: frame_acc" in out and "orbit metrics" in out and "per object" in out


def test_learner_saves_predictions_in_directory_mode(device, tmp_path):
    """--data_root with --save_predictions DIR: results.json in the challenge layout, one prediction per frame id of every target
    video; the ORBIT videos have a video label, so video accuracy is reported per video too."""
    from orbit_dataset_amd import learner
    from orbit_dataset_amd.data import pipeline
    tree = str(tmp_path / "test")
    pipeline.write_synthetic_orbit_directory(tree, users=2, objects_per_user=2, clean_videos=1, clutter_videos=2,
                                             frames_per_video=50, frame_size=32)
    args = learner.build_parser().parse_args(
        ["--mode", "test", "--feature_extractor", "resnet18", "--frame_size", "32", "--data_root", tree, "--num_workers", "2",
         "--subsample_factor", "5", "--batch_size", "16", "--save_predictions", str(tmp_path / "pred")])
    stats = learner.Learner(args).run()["test"]
    report = stats["orbit_metrics"]
    assert stats["num_tasks"] == 2 and set(report["video"]) == {"frame_acc", "frames_to_recognition", "video_acc"}
    assert abs(report["video"]["frame_acc"][0] - stats["frame_acc"][0]) <= 1e-6  # 4 videos of 50 frames per task
    results = json.load(open(tmp_path / "pred" / "results.json"))
    assert len(results) == 2
    frames = 0
    for user, tasks in results.items():
        assert len(tasks) == 1 and len(tasks[0]["task_object_list"]) == 2 and len(tasks[0]["task_videos"]) == 4
        for video_id, preds in tasks[0]["task_videos"].items():
            assert sorted(int(k) for k in preds) == list(range(1, 51)) and set(preds.values()) <= {0, 1}
            frames += len(preds)
    assert frames == stats["target_frames"] == 400
