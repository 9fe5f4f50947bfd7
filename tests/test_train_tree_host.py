"""--data_path without a GPU: the task queue's order (learner.task_order / Learner.train_order), which split directory every
loop reads and what verify_args refuses, and the train-layout tasks Learner.build_dataset("train") samples from a written
tree. Nothing here loads the library: Learner.__init__ needs a GPU, so the hooks are called on a bare instance."""
import os
import random

import pytest
import torch

import orbit_dataset_amd  # noqa: F401
from orbit_dataset_amd import learner
from orbit_dataset_amd.data.pipeline import write_synthetic_orbit_directory

BASE = ["--feature_extractor", "resnet18", "--frame_size", "64", "--learn_extractor", "--subsample_factor", "5"]


def _args(extra, multistep=False):
    return (learner.build_multistep_parser() if multistep else learner.build_parser()).parse_args(BASE + extra)


def _bare_learner(args, rank=0, world=1):
    L = object.__new__(learner.Learner)
    L.args, L.rank, L.world = args, rank, world
    return L


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    """ROOT/{train,validation,test}: 2 users x 3 objects x (2 clean + 1 clutter) videos of 50 frames (the target floor), 16 x 16"""
    root = str(tmp_path_factory.mktemp("orbit_root"))
    for k, split in enumerate(("train", "validation", "test")):
        write_synthetic_orbit_directory(os.path.join(root, split), users=2, objects_per_user=3, clean_videos=2, clutter_videos=1,
                                        frames_per_video=50, frame_size=16, seed=100 + k)
    return root


def test_task_order_lists_every_item_and_shuffles_per_epoch():
    plain = learner.task_order(3, 2)
    assert plain == [0, 0, 1, 1, 2, 2]  # validation and test queues: unshuffled, item-major
    rng = random.Random(77)
    want = []
    for _ in range(3):  # ONE stream, advanced epoch by epoch
        order = list(plain)
        rng.shuffle(order)
        want.append(order)
    got = [learner.task_order(3, 2, seed=77, epoch=e) for e in range(3)]
    assert got == want
    assert all(sorted(o) == plain for o in got)
    assert got[0] != got[1] and got[1] != got[2]
    assert learner.task_order(3, 2, seed=77, epoch=1) == got[1]       # reproducible from the seed, in any call order
    assert learner.task_order(3, 2, seed=78, epoch=0) != got[0]
    assert learner.task_order(0, 5, seed=1) == [] and learner.task_order(4, 0) == []


def test_train_order_deals_one_shuffled_order_to_the_ranks(root):
    args = _args(["--mode", "train", "--data_path", root, "--num_train_tasks", "3", "--seed", "5"])
    for epoch in range(2):
        whole = learner.task_order(2, 3, seed=5, epoch=epoch)  # 2 users x 3 tasks
        assert _bare_learner(args).train_order(epoch) == whole
        dealt = [_bare_learner(args, rank, 4).train_order(epoch) for rank in range(4)]
        assert dealt == [whole[rank::4] for rank in range(4)]          # every rank cuts the SAME order
        assert sorted(i for d in dealt for i in d) == [0, 0, 0, 1, 1, 1]
    # object-centric: the queue lists objects
    args = _args(["--mode", "train", "--data_path", root, "--num_train_tasks", "2", "--train_task_type", "object_centric"])
    assert sorted(_bare_learner(args).train_order(0)) == sorted(list(range(6)) * 2)


def test_split_roots(root):
    j = os.path.join
    assert learner.split_roots(_args(["--mode", "test"])) == {}
    assert learner.split_roots(_args(["--mode", "train_test"])) == {}
    assert learner.split_roots(_args(["--mode", "test", "--data_path", root])) == {"test": j(root, "test")}
    assert learner.split_roots(_args(["--mode", "test", "--data_path", root, "--test_set", "validation"])) == \
        {"test": j(root, "validation")}
    assert learner.split_roots(_args(["--mode", "train", "--data_path", root])) == {"train": j(root, "train")}
    assert learner.split_roots(_args(["--mode", "train_test", "--data_path", root, "--num_val_tasks", "2"])) == \
        {"train": j(root, "train"), "validation": j(root, "validation"), "test": j(root, "test")}
    # --data_root keeps its meaning: one split directory, the test loop only
    assert learner.split_roots(_args(["--mode", "test", "--data_root", j(root, "test")])) == {"test": j(root, "test")}
    assert learner.split_roots(_args(["--mode", "train_test", "--data_root", j(root, "test")])) == {"test": j(root, "test")}
    assert learner.split_roots(_args(["--mode", "train", "--data_root", j(root, "test")])) == {}
    assert learner.split_roots(_args(["--data_root", j(root, "test")], multistep=True)) == {"test": j(root, "test")}


def test_verify_args_names_the_missing_split(root, tmp_path):
    learner.verify_args(_args(["--mode", "train_test", "--data_path", root, "--num_val_tasks", "1"]))
    learner.verify_args(_args(["--mode", "test", "--data_path", root, "--test_set", "validation"]))
    partial = str(tmp_path / "partial")
    os.makedirs(os.path.join(partial, "test"))
    learner.verify_args(_args(["--mode", "test", "--data_path", partial]))
    for extra, missing in ((["--mode", "train"], "train"), (["--mode", "train_test"], "train"),
                           (["--mode", "test", "--test_set", "validation"], "validation")):
        with pytest.raises(SystemExit) as e:
            learner.verify_args(_args(extra + ["--data_path", partial]))
        assert os.path.join(partial, missing) in str(e.value)
    os.makedirs(os.path.join(partial, "train"))
    learner.verify_args(_args(["--mode", "train", "--data_path", partial]))  # no validation asked for: none needed
    with pytest.raises(SystemExit) as e:
        learner.verify_args(_args(["--mode", "train", "--data_path", partial, "--num_val_tasks", "1"]))
    assert os.path.join(partial, "validation") in str(e.value)
    for multistep in (False, True):
        with pytest.raises(SystemExit) as e:
            learner.verify_args(_args(["--mode", "test", "--data_path", root, "--data_root", os.path.join(root, "test")], multistep))
        assert "--data_path" in str(e.value) and "--data_root" in str(e.value)


def test_train_flags_have_the_reference_defaults():
    a = _args([])
    assert (a.train_way_method, a.train_object_cap, a.train_context_shot_method, a.train_target_shot_method) == \
        ("random", 15, "random", "random")
    assert (a.with_train_shot_caps, a.train_context_clip_method, a.train_target_clip_method, a.train_task_type) == \
        (False, "uniform", "random", "user_centric")
    assert a.test_set == "test" and a.data_path is None and a.decode == "host"


def _users_of(paths):
    return {p.split(os.sep)[-5] for p in paths.reshape(-1)}  # <user>/<object>/<clean|clutter>/<video>/<frame>.jpg


def test_build_dataset_train_yields_train_layout_tasks(root):
    # (clips of 2 frames: the sampler, like the reference's, forms them for the 'max' clip methods only - the others draw clip
    # numbers and use them as frame ids, data/datasets.py clip_frame_indices)
    args = _args(["--mode", "train", "--data_path", root, "--clip_length", "2", "--seed", "9", "--train_context_clip_method", "max",
                  "--train_target_clip_method", "max"])
    ds = _bare_learner(args).build_dataset("train", frames="paths")
    assert ds.root == os.path.join(root, "train") and not ds.test_mode and len(ds) == 2
    ways = set()
    for i in (0, 1, 0, 1, 0, 1):
        t = ds[i]
        # train layout: clips (not videos) with one label each, both sets shuffled
        n, m = len(t["context_labels"]), len(t["target_labels"])
        assert t["context_paths"].shape == (n, 2) and t["target_paths"].shape == (m, 2) and n > 0 and m > 0
        assert t["context_labels"].dtype == torch.int64 and t["target_labels"].dim() == 1
        assert t["context_clips"] is None and t["target_clips"] is None  # frames="paths": nothing decoded
        way = len(t["object_list"])
        ways.add(way)
        assert 2 <= way <= 3 and set(t["context_labels"].tolist()) == set(range(way))
        assert _users_of(t["context_paths"]) == _users_of(t["target_paths"]) == {t["task_id"]} == {ds.users[i]}
        assert all("clean" in p for p in t["context_paths"].reshape(-1)) and all("clutter" in p for p in t["target_paths"].reshape(-1))
    assert ways == {2, 3}  # --train_way_method random
    # the same seed and rank sample the same tasks; another rank has its own stream
    again = _bare_learner(args).build_dataset("train", frames="paths")
    other = _bare_learner(args, rank=1, world=2).build_dataset("train", frames="paths")
    a, b, c = ([list(d[i]["target_paths"].reshape(-1)) for i in (0, 1, 0, 1)] for d in (
        _bare_learner(args).build_dataset("train", frames="paths"), again, other))
    assert a == b and a != c


def test_object_centric_tasks_mix_users(root):
    args = _args(["--mode", "train", "--data_path", root, "--train_task_type", "object_centric", "--train_way_method", "max"])
    ds = _bare_learner(args).build_dataset("train", frames="paths")
    assert learner.num_items(ds) == 6 and ds.num_users == 2
    t = ds[0]
    assert len(t["object_list"]) == 6 and t["task_id"] is None
    assert _users_of(t["context_paths"]) == _users_of(t["target_paths"]) == {"P000", "P001"}


def test_validation_and_test_datasets_are_test_mode_with_their_own_streams(root):
    args = _args(["--mode", "train_test", "--data_path", root, "--num_val_tasks", "1"])
    L = _bare_learner(args)
    val, tst = L.build_dataset("validation", frames="paths"), L.build_dataset("test", frames="paths")
    assert val.root == os.path.join(root, "validation") and tst.root == os.path.join(root, "test") and val.test_mode and tst.test_mode
    t = tst[0]
    assert isinstance(t["target_paths"], list) and len(t["target_paths"]) == 3 and len(t["target_paths"][0]) == 50  # by video
    # three streams from one seed: train and test as test_directory always seeded them, validation a third
    draws = {s: learner.split_rng(args, s).random() for s in ("train", "validation", "test")}
    assert draws["train"] == draws["test"] == random.Random(args.seed).random() and draws["validation"] != draws["train"]
    assert learner.split_rng(args, "train", rank=3).random() == random.Random(args.seed + 3).random()
    with pytest.raises(ValueError):
        _bare_learner(_args(["--mode", "test", "--data_path", root])).build_dataset("train", frames="paths")
