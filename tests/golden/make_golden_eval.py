"""Generate G15_eval.npz: the REFERENCE's evaluators (utils/eval_metrics.py) run on a small fixed set of logits.

Run once where the reference is mounted (it never travels):

    python tests/golden/make_golden_eval.py [/root/reference]

The reference's `utils.eval_metrics` is imported as it is, with the absent third-party `thop` and the reference's
`utils.ops_counter` (which needs it) stubbed in sys.modules, as make_golden.py does for `timm`. Its real TestEvaluator is
driven over 2 users x 2 tasks x 3..4 videos of n in {1, 7, 64, 65} frames, C = 5, among them a video whose first frame is
correct, one with only its last frame correct, one with no correct frame, one with exact logit ties on the label column, one
with a tie in its histogram of predictions and one padded with a repeated last frame. Stored: the logits, labels and frame
ids, the reference's get_mean_stats() for frame_acc and frames_to_recognition, its per-video video accuracy, its results.json
flattened to arrays, and the public method names of its four classes. Only data - no reference source.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REF)

C = 5
STATS = ["frame_acc", "frames_to_recognition"]


def stub_ops_counter():
    thop = types.ModuleType("thop")
    thop.clever_format = lambda values, fmt: tuple(fmt % v for v in values)
    sys.modules["thop"] = thop
    ops = types.ModuleType("utils.ops_counter")
    ops.OpsCounter = type("OpsCounter", (), {})
    sys.modules["utils.ops_counter"] = ops


def make_video(g, kind, n, label):
    """float32 logits [n, C] whose argmax is placed by hand per `kind`; every non-tied margin is >= 0.5"""
    logits = torch.randn(n, C, generator=g) * 0.25

    def put(rows, col):
        logits[rows, col] = 3.0 + torch.rand(len(rows), generator=g)

    wrong = [c for c in range(C) if c != label]
    rows = torch.arange(n)
    if kind == "random":
        put(rows, torch.randint(0, C, (n,), generator=g))
    elif kind == "first_correct":
        put(rows, torch.tensor([label] + [wrong[i % 4] for i in range(n - 1)], dtype=torch.long))
    elif kind == "last_only":
        put(rows, torch.tensor([wrong[i % 4] for i in range(n - 1)] + [label], dtype=torch.long))
    elif kind == "none_correct":
        put(rows, torch.tensor([wrong[(3 * i) % 4] for i in range(n)], dtype=torch.long))
    elif kind == "logit_tie":
        # the label column holds the row maximum in every frame, tied EXACTLY with one other column: a lower one on even
        # frames (the first maximal column wins: wrong), a higher one on odd frames (correct)
        lower, higher = [c for c in range(C) if c < label], [c for c in range(C) if c > label]
        assert lower and higher
        for i in range(n):
            other = lower[i % len(lower)] if i % 2 == 0 else higher[i % len(higher)]
            logits[i, label] = logits[i, other] = 4.0 + 0.125 * (i % 5)
    elif kind == "hist_tie":
        # two classes predicted equally often, the label being the HIGHER column: bincount().argmax() names the lower one
        assert n % 2 == 0 and label > 0
        put(rows, torch.tensor([label if i % 2 else label - 1 for i in range(n)], dtype=torch.long))
    else:
        raise KeyError(kind)
    return logits


# (user, [task: [(kind, n, label, repeated_last_frames)]])
LAYOUT = [
    ("P100", [[("first_correct", 64, 2, 0), ("last_only", 65, 0, 0), ("random", 7, 4, 1)],
              [("none_correct", 7, 2, 0), ("logit_tie", 64, 2, 0), ("random", 1, 0, 0), ("random", 65, 4, 0)]]),
    ("P204", [[("hist_tie", 64, 3, 0), ("random", 65, 3, 0), ("random", 7, 1, 0), ("random", 1, 1, 0)],
              [("random", 64, 0, 0), ("first_correct", 7, 3, 0), ("random", 65, 1, 3)]]),
]
OBJECTS = ["keys", "mug", "phone", "wallet", "remote"]


def main():
    stub_ops_counter()
    from utils.eval_metrics import Evaluator, TestEvaluator, TrainEvaluator, ValidationEvaluator

    g = torch.Generator().manual_seed(1505)
    tmp = tempfile.mkdtemp()
    ev = TestEvaluator(STATS, save_dir=tmp)
    all_logits, rows = [], []  # rows: (user, task, video, label, raw frames)
    frame_ids, video_acc = [], []
    vid = 0
    for u, (user, tasks) in enumerate(LAYOUT):
        for t, videos in enumerate(tasks):
            ev.set_task_object_list(OBJECTS)
            for kind, n, label, repeats in videos:
                logits = make_video(g, kind, n, label)
                ids = [30 * i + 1 for i in range(n)]
                if repeats:  # padding to a multiple of the clip length repeats the last frame
                    logits = torch.cat([logits, logits[-1:].expand(repeats, C)])
                    ids = ids + [ids[-1]] * repeats
                name = "%s--%s--clutter--v%02d" % (user, OBJECTS[label], vid)
                paths = ["/data/%s/%s/clutter/%s/%s-%05d.jpg" % (user, OBJECTS[label], name, name, i) for i in ids]
                assert paths == sorted(paths)
                probs = torch.softmax(logits, dim=-1).numpy()
                assert np.array_equal(probs.argmax(-1), logits.numpy().argmax(-1))  # softmax merged no two logits
                ev.append_video(logits, torch.tensor(label), np.array(paths))
                video_acc.append(ev.get_video_accuracy(np.array(label), probs[:n]))
                all_logits.append(logits.numpy())
                rows.append((u, t, vid, label, len(ids)))
                frame_ids.extend(ids)
                vid += 1
            if t + 1 < len(tasks):
                ev.next_task()
        ev.set_current_user(user)
        if u + 1 < len(LAYOUT):
            ev.next_user()
    stats = np.array([[level[s] for s in STATS] for level in ev.get_mean_stats()], dtype=np.float64)  # [user|object|task|video][stat][mean|ci]
    stats_last_user = np.array([[level[s] for s in STATS] for level in ev.get_mean_stats(current_user=True)], dtype=np.float64)
    ev.save()
    with open(os.path.join(tmp, "results.json")) as f:
        results = json.load(f)
    flat = []  # (user index, task index, video number, frame id, prediction)
    for u, (user, _) in enumerate(LAYOUT):
        for t, task in enumerate(results[user]):
            assert task["task_object_list"] == OBJECTS
            for video_id, frames in task["task_videos"].items():
                flat.extend((u, t, int(video_id[-2:]), int(fid), int(pred)) for fid, pred in frames.items())

    def names(cls):
        return sorted(k for k in dir(cls) if not k.startswith("_") and callable(getattr(cls, k)))

    out = os.path.join(HERE, "G15_eval.npz")
    np.savez_compressed(
        out, logits=np.concatenate(all_logits).astype(np.float32), videos=np.array(rows, dtype=np.int64),
        frame_ids=np.array(frame_ids, dtype=np.int64), users=np.array([u for u, _ in LAYOUT]), objects=np.array(OBJECTS),
        stat_names=np.array(STATS), stats=stats, stats_last_user=stats_last_user, video_acc=np.array(video_acc, dtype=np.float64),
        results_flat=np.array(flat, dtype=np.int64),
        **{"methods_" + c.__name__: np.array(names(c)) for c in (Evaluator, TrainEvaluator, TestEvaluator, ValidationEvaluator)})
    print(out, os.path.getsize(out), "bytes;", len(rows), "videos,", len(frame_ids), "frames")
    print(stats)


if __name__ == "__main__":
    main()
