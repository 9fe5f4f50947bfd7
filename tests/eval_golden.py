"""Shared by test_eval_host.py and test_gpu_eval.py: fixture G15_eval (tests/golden/make_golden_eval.py) unpacked into videos,
the numpy restatement of the per-video integers, and the loop that drives an evaluator over the fixture's users and tasks."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G15_eval.npz")


def load():
    g = dict(np.load(GOLDEN))
    users, objects = [str(u) for u in g["users"]], [str(o) for o in g["objects"]]
    videos, row, fid = [], 0, 0
    for u, t, vid, label, n in g["videos"].tolist():
        name = "%s--%s--clutter--v%02d" % (users[u], objects[label], vid)
        ids = g["frame_ids"][fid:fid + n].tolist()
        videos.append({"user": u, "task": t, "vid": vid, "label": label, "logits": g["logits"][row:row + n],
                       "paths": ["/data/%s/%s/clutter/%s/%s-%05d.jpg" % (users[u], objects[label], name, name, i) for i in ids]})
        row, fid = row + n, fid + n
    g["users"], g["objects"], g["video_list"] = users, objects, videos
    return g


def numpy_integers(logits, label):
    """(preds, correct, first_correct, hist) of one video with numpy on the same float32 logits"""
    logits = np.asarray(logits, dtype=np.float32)
    n, C = logits.shape
    preds = np.argmax(logits, axis=-1) if n else np.zeros(0, dtype=np.int64)
    hits = np.where(preds == label)[0]
    return preds, len(hits), int(hits[0]) if len(hits) else n, np.bincount(preds, minlength=C)


def first_occurrences(paths):
    seen, keep = set(), []
    for i, p in enumerate(paths):
        if p not in seen:
            seen.add(p)
            keep.append(i)
    return keep


def drive(evaluator, g, append):
    """the generator's loop: append(evaluator, video) per video, next_task / next_user between, user ids and object lists set"""
    videos = g["video_list"]
    for i, v in enumerate(videos):
        if i and v["user"] != videos[i - 1]["user"]:
            evaluator.set_current_user(g["users"][videos[i - 1]["user"]])
            evaluator.next_user()
        elif i and v["task"] != videos[i - 1]["task"]:
            evaluator.next_task()
        if i == 0 or (v["user"], v["task"]) != (videos[i - 1]["user"], videos[i - 1]["task"]):
            evaluator.set_task_object_list(g["objects"])
        append(evaluator, v)
    evaluator.set_current_user(g["users"][videos[-1]["user"]])
    return evaluator


def stats_array(levels, names):
    return np.array([[level[s] for s in names] for level in levels], dtype=np.float64)


def flat_results(results, users):
    flat = []
    for u, user in enumerate(users):
        for t, task in enumerate(results[user]):
            for video_id, frames in task["task_videos"].items():
                flat.extend((u, t, int(video_id[-2:]), int(fid), int(pred)) for fid, pred in frames.items())
    return np.array(flat, dtype=np.int64)
