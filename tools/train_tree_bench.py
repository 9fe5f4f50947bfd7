"""LITE meta-training of efficientnet_b0 on a 224 x 224 JPEG tree sized like the headline task, --decode host against --decode
device, beside the synthetic-task step at the same way and frame counts. Usage: train_tree_bench.py OUT.json [reversed]
(reversed: the three runs in the opposite order, to tell a run's place in the process from its decode mode)"""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import orbit_dataset_amd  # noqa
from orbit_dataset_amd import learner
from orbit_dataset_amd.data import pipeline

root = tempfile.mkdtemp()
t0 = time.time()
# 4 users x 5 objects x (2 clean videos of 20 frames + 1 clutter video of 50): every clip of every video ('max' methods below)
# makes a task of 5 x 40 = 200 context and 5 x 50 = 250 target frames. (Two calls, so that the video lengths differ: an object's
# clutter video does not share its clean videos' template - the accuracies of these runs mean nothing, the times do.)
n = pipeline.write_synthetic_orbit_directory(os.path.join(root, "train"), users=4, objects_per_user=5, clean_videos=2, clutter_videos=0,
                                             frames_per_video=20, frame_size=224, seed=11)
n += pipeline.write_synthetic_orbit_directory(os.path.join(root, "train"), users=4, objects_per_user=5, clean_videos=0, clutter_videos=1,
                                              frames_per_video=50, frame_size=224, seed=12)
print("wrote %d frames in %.1f s" % (n, time.time() - t0), flush=True)
common = ["--mode", "train", "--with_lite", "--learn_extractor", "--feature_extractor", "efficientnet_b0", "--num_workers", "16",
          "--epochs", "1"]
tree = common + ["--data_path", root, "--num_train_tasks", "10", "--train_way_method", "max", "--train_context_shot_method", "max",
                 "--train_target_shot_method", "max", "--train_context_clip_method", "max", "--train_target_clip_method", "max"]
runs = {"decode_host": tree + ["--decode", "host"], "decode_device": tree + ["--decode", "device"],
        "synthetic": common + ["--way", "5", "--shots", "5", "--frames_per_shot", "8", "--num_query_videos", "5", "--frames_per_video", "50",
                               "--num_train_tasks", "20"]}
if sys.argv[2:] == ["reversed"]:
    runs = dict(reversed(list(runs.items())))
out = {"tree": {"frames": n, "frame_size": 224, "users": 4, "objects_per_user": 5, "context_frames_per_task": 200,
                "target_frames_per_task": 250}, "runs": {}}
SKIP = 5  # warm-up tasks left out of the steady figures (plan build, first touches)
for name, argv in runs.items():
    L = learner.Learner(learner.build_parser().parse_args(argv))
    stats = L.train()
    step, wait = np.array(L.task_ms[SKIP:]), np.array(L.task_wait_ms[SKIP:]) if L.task_wait_ms else None
    steady = {"tasks": len(step), "step_ms_median": float(np.median(step)), "step_ms_mean": float(step.mean()),
              "wait_ms_median": float(np.median(wait)) if wait is not None else None,
              "wait_ms_mean": float(wait.mean()) if wait is not None else None,
              "tasks_per_s": float(1e3 / ((wait.mean() if wait is not None else 0.0) + step.mean()))}
    out["runs"][name] = {"argv": [a if a != root else "ROOT" for a in argv], "stats": {k: (v if k != "data_path" else "ROOT")
                                                                                       for k, v in stats.items()},
                         "tasks_per_s_of_wall": stats["num_tasks"] / stats["wall_s"], "steady": steady,
                         "task_ms": [round(x, 3) for x in L.task_ms], "task_wait_ms": [round(x, 3) for x in L.task_wait_ms]}
    print(name, json.dumps(steady), flush=True)
    del L
with open(sys.argv[1] if len(sys.argv) > 1 else "train_tree_efficientnet_b0_224.json", "w") as f:
    json.dump(out, f, indent=1)
import shutil  # noqa: E402
shutil.rmtree(root)
