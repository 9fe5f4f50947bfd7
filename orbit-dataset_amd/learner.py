"""Counterpart of the reference's single-step-learner.py and multi-step-learner.py for the native path: train, validate and
test, and the finetuner's test, on synthetic tasks or on a dataset tree.

Keeps the reference CLI's flag names for everything that touches the hot path (reference utils/args.py:12-192:
--feature_extractor --learn_extractor --adapt_features --classifier --logit_scale --clip_length --frame_size
--batch_size --tasks_per_batch --with_lite --num_lite_samples --gpu --seed --mode --model_path) and the test
loop's call order (reference single-step-learner.py:298-375): per task personalise() -> per target video
{attach_frame_history -> predict -> frame accuracy} -> _reset(), with 'personalise' and per-frame 'inference' timers
(here device-synchronised; the reference's time.time() pairs do not sync). That loop is written once
(`Learner._evaluate`) for test and validation, the single-step learner and the finetuner (which swaps in its two steps,
`_personalise` / `_predict_video`), a tree's tasks and synthetic ones. Without a dataset tree the tasks come from
`synthetic.make_task` in the task_dict layout of reference data/datasets.py:584-597, their query frames grouped into videos as
a tree's test-mode tasks are (`Learner.make_task`); `--feature_extractor` additionally accepts resnet18 and `--frame_size`
any size (BASELINE.json configs).

Training (reference single-step-learner.py:128-243): per task `train_task` or `train_task_with_lite` (per query
batch {personalise_with_lite -> predict_a_batch -> N/(H*tasks_per_batch) * CE + 0.001 * l2 -> backward -> _reset}),
optimizer.step()/zero_grad() every `tasks_per_batch` tasks, optimizer groups as utils/optim.py:11-33 (extractor
parameters in their own group with `extractor_lr_scale`). All gradients come from the native backward kernels
(model/autograd.py); the optimizer is torch.optim on the device-resident parameters, or with --native_optimizer the same
update as one native launch per step (optim.NativeAdam / NativeSGD, csrc/optim.hip). The learning rate follows the
reference's epoch schedules (--scheduler none | step | multistep | cosine with its warm-up and decay flags, utils/optim.py:34-43;
optim.init_scheduler restates timm's formulas; default none = constant), stepped after every epoch before validation
(single-step-learner.py:177-181). With --checkpoint_dir DIR rank 0 writes DIR/checkpoint.pt after every epoch with the reference's
four keys (epoch, model_state_dict, optimizer_state_dict, best_stats; :377-390) and --resume continues from it at that epoch.

On a dataset tree (--data_path ROOT, the reference's flag; --data_root DIR for the test loop alone) all three loops take
their tasks from the reference-pinned sampler (data/datasets.py) in the reference's queue order (task_order) through the
input pipeline (data/pipeline.TaskPrefetcher: decode, 8-bit or compressed upload, resize and normalisation on a copy
stream): train on ROOT/train, validate on ROOT/validation, test - the finetuner too - on ROOT/<--test_set>. The reference's
five annotation flags hold there (utils/args.py:79-88): --train_filter_* on the train split, --test_filter_* on the
validation and test splits, --annotations_to_load on all three; the filters act when the tree is indexed, so a dropped
frame is never read. `--test_filter_target no_object_not_present_issue` is the benchmark's clutter-video protocol (CLU-VE).

Multi-GPU: launched under torchrun, tasks are dealt round-robin to ranks (task i -> rank i % world). Test and validation
have no data-path collective (per-task statistics are all-gathered at the end: `gather_lists`). Training all-reduces (SUM, RCCL) one
flat gradient bucket per optimizer step: every task's loss already carries 1/tasks_per_batch, so the sum over ranks
reproduces single-GPU accumulation; BatchNorm running statistics are combined at the same point as the reference's
sequential updates would have left them (dist.RunningStatSync).
"""
import argparse
import collections
import contextlib
import json
import math
import os
import random
import sys
import time
import types

import numpy as np
import torch

from . import dist as odist
from . import synthetic
from .data.datasets import ALL_FRAME_ANNOTATION_OPTIONS, BOUNDING_BOX_OPTIONS, FRAME_ANNOTATION_OPTIONS, expand_issues
from .data.utils import attach_frame_history, unpack_task
from .model.feature_extractors import EXTRACTORS
from .model.few_shot_recognisers import MultiStepFewShotRecogniser, SingleStepFewShotRecogniser
from .optim import (SCHEDULERS, apply_lr_scale, cross_entropy, get_curr_learning_rates, init_optimizer,  # noqa: F401
                    init_scheduler)  # (re-exported: bench.py, tools)
from .utils.eval_metrics import TestEvaluator


def build_parser():
    p = argparse.ArgumentParser(description="single-step learner on the MI355X-native recogniser (synthetic tasks)")
    # flags shared with the reference (utils/args.py)
    p.add_argument("--feature_extractor", default="efficientnet_b0", choices=list(EXTRACTORS))
    p.add_argument("--learn_extractor", action="store_true")
    p.add_argument("--adapt_features", action="store_true")
    p.add_argument("--classifier", default="proto", choices=["proto", "proto_cosine", "versa", "mahalanobis", "linear"])
    p.add_argument("--logit_scale", type=float, default=1.0)
    p.add_argument("--clip_length", type=int, default=1)
    p.add_argument("--frame_size", type=int, default=224)
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--tasks_per_batch", type=int, default=16)
    p.add_argument("--with_lite", action="store_true")
    p.add_argument("--vit_native_backward", action="store_true",
                   help="vit_*_32* extractors: opt in to the native FiLM gradients through the FROZEN transformer (--adapt_features "
                        "training, with or without --with_lite; the multi-step finetuner's --adapt_features). --learn_extractor "
                        "stays refused: weight gradients are not built")
    p.add_argument("--vit_native_weight_backward", action="store_true",
                   help="vit_*_32* extractors: opt in to the native gradients of every parameter of the transformer (implies what "
                        "--vit_native_backward admits, and admits --learn_extractor). Ignored for the other extractors, the "
                        "inference-only patch-16 transformers among them")
    p.add_argument("--vit16_native_backward", action="store_true",
                   help="vit_*_16* extractors (the patch-16 transformers) only, ignored elsewhere: opt in to the native FiLM "
                        "gradients through the FROZEN transformer at 197 tokens (--adapt_features training, with or without "
                        "--with_lite; the multi-step finetuner's --adapt_features). --learn_extractor stays refused under this "
                        "flag alone: --vit16_native_weight_backward opens it")
    p.add_argument("--vit16_native_weight_backward", action="store_true",
                   help="vit_*_16* extractors only, ignored elsewhere: opt in to the native gradients of every parameter of the "
                        "transformer at 197 tokens (implies what --vit16_native_backward admits, and admits --learn_extractor, "
                        "with or without --with_lite / --adapt_features)")
    p.add_argument("--vit_bf16", action="store_true",
                   help="vit_* extractors (all six), test modes only: run the qkv / proj / fc1 / fc2 GEMMs of the transformer with "
                        "bf16 operands and fp32 accumulation (VisionTransformer.bf16_inference; everything else stays fp32). A "
                        "documented precision trade, off by default; refused with a training mode and with the finetuner's "
                        "--learn_extractor / --adapt_features; ignored with a note for the other extractors")
    p.add_argument("--vit_resample_pos_embed", action="store_true",
                   help="vit_* extractors (all six), test modes only: lift the 224x224 restriction. --frame_size S (a multiple of "
                        "the model's patch size, 32..512) goes to the data pipeline as for the CNN extractors, and the transformer "
                        "adds its position table resampled to the S / patch grid (torch's bicubic, timm's resize_pos_embed; "
                        "VisionTransformer.resample_pos_embed). Off by default; at another size than 224 refused with a training "
                        "mode and with the finetuner's --learn_extractor / --adapt_features; ignored with a note for the other "
                        "extractors")
    p.add_argument("--effnetv2_native_backward", action="store_true",
                   help="efficientnet_v2_s: opt in to the native FiLM gradients through the FROZEN network (--adapt_features "
                        "training, with or without --with_lite; the multi-step finetuner's --adapt_features). --learn_extractor "
                        "stays refused under this flag alone: --effnetv2_native_weight_backward opens it. Ignored for the other "
                        "extractors")
    p.add_argument("--effnetv2_native_weight_backward", action="store_true",
                   help="efficientnet_v2_s: opt in to native training of the whole network - batch-statistics BatchNorm and the "
                        "gradients of every parameter (implies what --effnetv2_native_backward admits, and admits "
                        "--learn_extractor, with or without --with_lite). Ignored for the other extractors")
    p.add_argument("--num_lite_samples", type=int, default=16)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--seed", type=int, default=synthetic.DEFAULT_SEED)
    p.add_argument("--mode", default="test", choices=["train", "test", "train_test"])
    p.add_argument("--model_path", default=None)
    p.add_argument("--save_model_path", default=None,
                   help="where --mode train / train_test writes model.state_dict() after training (the reference saves "
                        "checkpoint_dir/final.pt, single-step-learner.py:185)")
    # synthetic-task shape (the dataset-side flags of the reference have no meaning here)
    p.add_argument("--way", type=int, default=5)
    p.add_argument("--shots", type=int, default=5)
    p.add_argument("--frames_per_shot", type=int, default=8)
    p.add_argument("--num_query_videos", type=int, default=4)
    p.add_argument("--frames_per_video", type=int, default=50)
    p.add_argument("--num_test_tasks", type=int, default=8)
    p.add_argument("--num_train_tasks", type=int, default=16,
                   help="synthetic tasks per epoch. With --data_path: train tasks per train USER (per OBJECT with "
                        "--train_task_type object_centric) and epoch, as the reference counts them (utils/args.py:91)")
    p.add_argument("--epochs", "-e", type=int, default=1)
    p.add_argument("--num_val_tasks", type=int, default=0,
                   help="validation tasks run after every epoch from --validation_on_epoch on (reference validate(), "
                        "single-step-learner.py:245-296; 0 = no validation). Synthetic tasks in all; with --data_path: tasks "
                        "per validation USER, sampled from ROOT/validation")
    p.add_argument("--validation_on_epoch", type=int, default=1, help="epoch to turn on validation (reference utils/args.py:117)")
    p.add_argument("--save_best_model_path", default=None,
                   help="where the model with the best validation frame accuracy so far is written (reference "
                        "checkpoint_dir/best.pt, single-step-learner.py:290-293)")
    p.add_argument("--learning_rate", "-lr", type=float, default=5e-6)
    p.add_argument("--extractor_lr_scale", type=float, default=1.0)
    p.add_argument("--optimizer", default="adam", choices=["adam", "sgd"])
    p.add_argument("--weight_decay", type=float, default=0.2)
    p.add_argument("--epsilon", type=float, default=1e-6)
    p.add_argument("--p2p_gradients", action="store_true",
                   help="multi-GPU: all-reduce the gradient bucket with the direct peer-to-peer reduce-scatter + all-gather "
                        "(csrc/comm.hip) instead of the backend's ring")
    p.add_argument("--fused_optimizer", action="store_true",
                   help="torch's fused multi-tensor Adam (same update, ~7 ms less host time per efficientnet_b0 step; the "
                        "native plans are re-synchronised from an optimizer step hook, optim.mark_parameters_changed)")
    p.add_argument("--native_optimizer", action="store_true",
                   help="the optimizer step as ONE native launch over all parameter tensors (csrc/optim.hip; torch.optim's "
                        "arithmetic, state_dict interchangeable with torch.optim.Adam / SGD) instead of torch's foreach ops. "
                        "Not together with --fused_optimizer")
    p.add_argument("--betas", type=float, nargs=2, default=(0.9, 0.98))
    p.add_argument("--momentum", type=float, default=0.0)
    # learning-rate schedule (reference utils/args.py, consumed by utils/optim.py:34-43 through timm's create_scheduler)
    p.add_argument("--scheduler", dest="sched", default="none", choices=list(SCHEDULERS),
                   help="epoch schedule of the learning rate (the reference's --sched; none = constant --learning_rate)")
    p.add_argument("--warmup_lr", type=float, default=1e-6, help="learning rate the linear warm-up starts from")
    p.add_argument("--warmup_epochs", type=int, default=5, help="epochs of linear warm-up to --learning_rate (0: none)")
    p.add_argument("--decay_epochs", type=int, default=15, help="step: epochs per decay; multistep: milestone spacing")
    p.add_argument("--decay_rate", type=float, default=0.5, help="factor of every decay")
    p.add_argument("--cooldown_epochs", type=int, default=0, help="accepted for the reference's command lines; has no effect")
    p.add_argument("--lr_k_decay", type=float, default=0.1, help="cosine: exponent k of (t / epochs) ** k")
    p.add_argument("--min_lr", type=float, default=1e-6, help="cosine: the floor of the learning rate")
    p.add_argument("--checkpoint_dir", default=None, metavar="DIR",
                   help="training: rank 0 writes DIR/checkpoint.pt after every epoch (epoch, model_state_dict, "
                        "optimizer_state_dict, best_stats: reference single-step-learner.py:377-390)")
    p.add_argument("--resume", action="store_true",
                   help="training: load --checkpoint_dir/checkpoint.pt and continue at its epoch under the same arguments")
    p.add_argument("--print_by_step", action="store_true")
    p.add_argument("--results_path", default=None)
    p.add_argument("--save_predictions", default=None, metavar="DIR",
                   help="with --data_root: write DIR/results.json, one predicted class per frame id of every target video in "
                        "the ORBIT challenge's layout (reference TestEvaluator.save(), utils/eval_metrics.py:112-153)")
    p.add_argument("--data_path", default=None, metavar="ROOT",
                   help="the reference's flag (utils/args.py:18): a dataset root with train/, validation/ and test/ below it, each "
                        "laid out as --data_root describes. Train tasks are sampled from ROOT/train (--train_* flags), validation "
                        "tasks from ROOT/validation and test tasks from ROOT/<--test_set> (--test_* flags), through the same input "
                        "pipeline as --data_root: --frame_size, --resample, --decode and --num_workers hold in every loop. "
                        "Not together with --data_root. Without either flag every loop runs on synthetic tasks")
    p.add_argument("--test_set", default="test", choices=["validation", "test"],
                   help="with --data_path: the split the test tasks are sampled from (reference utils/args.py:19)")
    p.add_argument("--data_root", default=None,
                   help="--mode test only (training and validation stay on synthetic tasks; use --data_path for them): one "
                        "split directory, a frame directory laid out like ORBIT (root/<user>/<object>/<clean|clutter>/<video>/*.jpg, "
                        "reference data/datasets.py:139-200). Tasks are the users' (context = clean videos, target = clutter "
                        "videos); frames are decoded with PIL by --num_workers threads, uploaded as 8-bit on a copy stream and "
                        "normalised on the GPU (data/pipeline.TaskPrefetcher) while the previous task runs. Frames stored at "
                        "another size than --frame_size are resized to it on the GPU in the same launch (--resample)")
    p.add_argument("--decode", default="host", choices=["host", "device"],
                   help="with --data_root: where the JPEG frames are decoded. host (default): PIL on --num_workers threads. "
                        "device: the threads only read the files and parse their headers, the compressed bytes are uploaded and "
                        "decoded on the GPU (baseline JPEG; Pillow's pixels bit for bit). Files the GPU path does not cover "
                        "(progressive, CMYK ..) or reports damaged are decoded by PIL; the results record how many")
    p.add_argument("--resample", default="lanczos", choices=["lanczos", "bicubic", "bilinear"],
                   help="with --data_root: the filter of that resize, PIL's 8-bit Image.resize bit for bit (default: the "
                        "reference's offline pass, scripts/resize_videos.py:46 Image.LANCZOS)")
    # dataset-side flags of the reference (utils/args.py:41-73), used with --data_root
    p.add_argument("--test_way_method", default="max", choices=["random", "max"])
    p.add_argument("--test_object_cap", type=int, default=15)
    p.add_argument("--test_context_shot_method", default="max", choices=["specific", "fixed", "random", "max"])
    p.add_argument("--test_target_shot_method", default="max", choices=["specific", "fixed", "random", "max"])
    p.add_argument("--context_shot", type=int, default=5)
    p.add_argument("--target_shot", type=int, default=2)
    p.add_argument("--context_video_type", default="clean", choices=["clean"])
    p.add_argument("--target_video_type", default="clutter", choices=["clutter", "clean"])
    p.add_argument("--subsample_factor", type=int, default=30)
    p.add_argument("--test_context_clip_method", default="uniform", choices=["random", "random_200", "max", "uniform"])
    p.add_argument("--test_target_clip_method", default="random_200", choices=["random", "random_200", "max"])
    # ... and their train-side counterparts (utils/args.py:39-91), used with --data_path
    p.add_argument("--train_way_method", default="random", choices=["random", "max"])
    p.add_argument("--train_object_cap", type=int, default=15)
    p.add_argument("--train_context_shot_method", default="random", choices=["specific", "fixed", "random", "max"])
    p.add_argument("--train_target_shot_method", default="random", choices=["specific", "fixed", "random", "max"])
    p.add_argument("--with_train_shot_caps", action="store_true", help="caps the videos per object sampled in train tasks")
    p.add_argument("--train_context_clip_method", default="uniform", choices=["random", "random_200", "max", "uniform"])
    p.add_argument("--train_target_clip_method", default="random", choices=["random", "random_200", "max"])
    p.add_argument("--train_task_type", default="user_centric", choices=["user_centric", "object_centric"],
                   help="with --data_path: train tasks from one user's objects, or from the objects of all users")
    p.add_argument("--max_test_tasks", type=int, default=None,
                   help="with --data_root: evaluate only the first N tasks of the user-major order (default: all users)")
    p.add_argument("--num_test_tasks_per_user", type=int, default=1,
                   help="with --data_root / --data_path: tasks sampled per test user (reference --num_test_tasks, utils/args.py)")
    p.add_argument("--num_workers", type=int, default=4, help="decode threads (reference data/queues.py:34: 4 in test mode)")
    p.add_argument("--frame_norm_method", default="imagenet", choices=["imagenet", "imagenet_inception", "openai_clip"])
    # frame annotations (reference utils/args.py:79-88), with --data_path / --data_root: ROOT/annotations/<split>/<video>.json
    p.add_argument("--annotations_to_load", nargs="+", default=[], choices=FRAME_ANNOTATION_OPTIONS + BOUNDING_BOX_OPTIONS,
                   help="annotations to load per frame: every task carries them as host tensors (context_annotations / "
                        "target_annotations; object_bounding_box is not built)")
    for split, role in (("train", "train"), ("test", "validation / test")):
        for which in ("context", "target"):
            p.add_argument("--%s_filter_%s" % (split, which), nargs="+", default=[], choices=ALL_FRAME_ANNOTATION_OPTIONS,
                           help="keep only the %s frames of %s tasks that carry one of these annotations (no_<issue>: the issue "
                                "is annotated false; no_issues / mixed_issues: all seven no_<issue> / <issue> names). "
                                "--test_filter_target no_object_not_present_issue is the benchmark's CLU-VE rule" % (which, role))
    return p


ANNOTATION_FLAGS = ("annotations_to_load", "train_filter_context", "train_filter_target", "test_filter_context", "test_filter_target")


def expand_annotation_args(args):
    """reference utils/args.py:181-184, after parsing: no_issues / mixed_issues in the four filter flags become the seven
    names they stand for (data/datasets.expand_issues). Idempotent; flags an args object lacks are set to []. Returns args."""
    args.annotations_to_load = list(getattr(args, "annotations_to_load", None) or [])
    for flag in ANNOTATION_FLAGS[1:]:
        setattr(args, flag, expand_issues(getattr(args, flag, None) or []))
    return args


def split_annotation_args(args, split):
    """-> (annotations_to_load, (filter_context, filter_target)) of a split's dataset, as reference data/dataloaders.py:29-30,
    48-49,66-67 passes them: the train pair to the train split, the test pair to the validation and test splits"""
    expand_annotation_args(args)
    side = "train" if split == "train" else "test"
    return args.annotations_to_load, (getattr(args, side + "_filter_context"), getattr(args, side + "_filter_target"))


# The extractors whose network is frozen unless a flag opts in: the frame normalisation the reference sets for them
# (utils/args.py:185-190; the other extractors keep --frame_norm_method), the one frame size they run on (None: any), the flag
# that opens the FiLM gradients through the frozen network and the one that opens the weight gradients (None: not built), the
# words their refusals differ in, and - the patch-16 transformers, whose refusals under the two patch-32 flags are pinned - a
# FiLM-gradient flag and a weight-gradient flag of their own.
FrozenExtractor = collections.namedtuple("FrozenExtractor",
                                         "frame_norm frame_size film_flag weight_flag no_weights no_backward film16_flag "
                                         "weight16_flag", defaults=(None, None))
_VIT = ("vit_native_backward", "vit_native_weight_backward", "weight gradients through a ViT", "a ViT")
_VIT16 = (None, None) + _VIT[2:] + ("vit16_native_backward", "vit16_native_weight_backward")
FROZEN_EXTRACTORS = {
    "vit_s_32": FrozenExtractor("imagenet_inception", 224, *_VIT),
    "vit_b_32": FrozenExtractor("imagenet_inception", 224, *_VIT),
    "vit_b_32_clip": FrozenExtractor("openai_clip", 224, *_VIT),
    # the patch-16 models: inference + FiLM only under the patch-32 flags; --vit16_native_backward opens the FiLM gradients
    # through the frozen network (csrc/vit.hip vit_attention197_bwd_kernel), --vit16_native_weight_backward the weight
    # gradients (vit_wgrad_kernel<WX_PATCH16> and the Linear weight gradients at 197 tokens)
    "vit_s_16": FrozenExtractor("imagenet_inception", 224, *_VIT16),
    "vit_b_16": FrozenExtractor("imagenet_inception", 224, *_VIT16),
    "vit_b_16_clip": FrozenExtractor("openai_clip", 224, *_VIT16),
    # any frame size, as efficientnet_b0. By default the native plan has no backward (its ConvBnAct blocks add the skip after
    # the activation, csrc/extractor_train.hip plan_trainable); the first flag opens the frozen form, the second all of it
    "efficientnet_v2_s": FrozenExtractor("imagenet_inception", None, "effnetv2_native_backward", "effnetv2_native_weight_backward",
                                         "weight gradients and batch-statistics BatchNorm", "its post-activation skips"),
}


# ---- tasks from a dataset tree (--data_path / --data_root) ------------------------------------------------------------------
def split_roots(args):
    """{split: directory} of the splits the run's mode reads from a tree (reference data/dataloaders.py:15-70): --data_path
    ROOT gives ROOT/train (and ROOT/validation when validation is on) to the training modes and ROOT/<--test_set> to the test
    modes; --data_root DIR is one split directory for the test loop alone. {} on synthetic tasks. Both flags: an error."""
    root, single = getattr(args, "data_path", None), getattr(args, "data_root", None)
    if root and single:
        sys.exit("error: --data_path (a root with train/, validation/ and test/ below it) and --data_root (one split directory, "
                 "test loop only) cannot be given together")
    roots = {}
    if root:
        if "train" in args.mode:
            roots["train"] = os.path.join(root, "train")
            if getattr(args, "num_val_tasks", 0) > 0:
                roots["validation"] = os.path.join(root, "validation")
        if "test" in args.mode:
            roots["test"] = os.path.join(root, getattr(args, "test_set", "test"))
    elif single and "test" in args.mode:
        roots["test"] = single
    return roots


def task_order(num_items, num_tasks, seed=None, epoch=0):
    """The reference's task queue (data/samplers.py:24-30): every item - a user, or an object for object-centric training -
    listed `num_tasks` times. seed None: left in that order (validation and test queues). Otherwise shuffled as the train
    queue is, once per epoch, by ONE random.Random(seed) that advances epoch by epoch - a stream of its own, so neither the
    datasets' sampling nor how far a prefetcher runs ahead moves it, and identical on every rank."""
    order = [item for item in range(num_items) for _ in range(num_tasks)]
    if seed is None:
        return order
    rng = random.Random(seed)
    for _ in range(epoch + 1):
        shuffled = list(order)
        rng.shuffle(shuffled)
    return shuffled


def split_rng(args, split, rank=0):
    """The sampling stream of a split's dataset: separate per split and rank, so tasks staged ahead for one loop never
    interleave their draws with another's. train and test: random.Random(seed + rank); validation: a third stream."""
    return random.Random(args.seed + rank + (7919 * 104729 if split == "validation" else 0))


def build_split_dataset(args, split, root, frames="uint8", rank=0, decode_pool=None):
    """The reference's queue datasets (data/dataloaders.py:15-70 -> data/queues.py) on `root`: "train" samples with the
    --train_* flags in train mode (clips and labels shuffled), user- or object-centric; "validation" and "test" with the
    --test_* flags in test mode (target frames grouped by video), user-centric. --annotations_to_load goes to every split,
    the --train_filter_* pair to "train" and the --test_filter_* pair to "validation" and "test"."""
    from .data.datasets import ObjectEpisodicORBITDataset, UserEpisodicORBITDataset
    a = args
    if split not in ("train", "validation", "test"):
        raise ValueError("split must be 'train', 'validation' or 'test', got %r" % (split,))
    train = split == "train"
    cls = ObjectEpisodicORBITDataset if train and a.train_task_type == "object_centric" else UserEpisodicORBITDataset
    way, cap, shot_methods, clip_methods = (
        (a.train_way_method, a.train_object_cap, (a.train_context_shot_method, a.train_target_shot_method),
         (a.train_context_clip_method, a.train_target_clip_method)) if train else
        (a.test_way_method, a.test_object_cap, (a.test_context_shot_method, a.test_target_shot_method),
         (a.test_context_clip_method, a.test_target_clip_method)))
    to_load, filters = split_annotation_args(a, split)
    return cls(root, way, cap, shot_methods, (a.context_shot, a.target_shot), (a.context_video_type, a.target_video_type),
               a.subsample_factor, clip_methods, a.clip_length, a.frame_size, a.frame_norm_method, to_load, filters, not train, False,
               bool(train and a.with_train_shot_caps), None, frames=frames, rng=split_rng(a, split, rank), decode_pool=decode_pool)


def num_items(dataset):
    """what a queue lists: the objects of an object-centric dataset, else the users (data/queues.py:54,74)"""
    from .data.datasets import ObjectEpisodicORBITDataset
    return dataset.num_objects if isinstance(dataset, ObjectEpisodicORBITDataset) else dataset.num_users


def opted_in(args, spec):
    """The one map from a frozen-scope extractor's opt-in flags to the gradient scope they open and the extractor attributes
    they set -> (scope "all" | "film" | "none", the flag that opened it, the attributes of every flag given)."""
    table = ((spec.weight_flag, "all", "native_weight_backward"), (spec.film_flag, "film", "native_backward"),
             (spec.weight16_flag, "all", "native_weight_backward_patch16"), (spec.film16_flag, "film", "native_backward_patch16"))
    on = [(flag, scope, attr) for flag, scope, attr in table if flag and getattr(args, flag, False)]
    if not on:
        return "none", None, []
    return on[0][1], on[0][0], [attr for _, _, attr in on]


def verify_args(args):
    """reference utils/args.py:203-217. For the frozen-scope extractors (FROZEN_EXTRACTORS) also the frame normalisation the
    reference sets for them and the inference-only scope: everything that would send a gradient or batch statistics through the
    extractor is refused here rather than at the first forward. The FiLM-gradient flag widens the scope to everything but
    --learn_extractor, and the weight-gradient flag to that as well."""
    if "train" in args.mode and not args.learn_extractor and not args.adapt_features:
        sys.exit("error: at least one of --learn_extractor and --adapt_features must be used when training")
    if args.frame_size % 1 or args.frame_size < 32:
        sys.exit("error: --frame_size must be >= 32")
    if getattr(args, "resume", False):
        if not getattr(args, "checkpoint_dir", None):
            sys.exit("error: --resume needs --checkpoint_dir (the directory that holds checkpoint.pt)")
        if not os.path.isfile(os.path.join(args.checkpoint_dir, "checkpoint.pt")):
            sys.exit("error: --resume: %s does not exist" % os.path.join(args.checkpoint_dir, "checkpoint.pt"))
    if getattr(args, "native_optimizer", False) and getattr(args, "fused_optimizer", False):
        sys.exit("error: --native_optimizer and --fused_optimizer are two optimizer steps: choose one")
    expand_annotation_args(args)
    given = ["--" + f for f in ANNOTATION_FLAGS if getattr(args, f)]
    if given and not (getattr(args, "data_path", None) or getattr(args, "data_root", None)):
        sys.exit("error: %s need a dataset tree (--data_path / --data_root): synthetic tasks have no frame annotations "
                 "(DESIGN.md §1)" % ", ".join(given))
    if "object_bounding_box" in args.annotations_to_load:
        sys.exit("error: --annotations_to_load object_bounding_box is not built (DESIGN.md §8)")
    for split, path in split_roots(args).items():  # (exits when both --data_path and --data_root are given)
        if getattr(args, "data_path", None) and not os.path.isdir(path):
            sys.exit("error: --data_path %s: --mode %s needs the %s split, and %s is not a directory"
                     % (args.data_path, args.mode, split, path))
    fe = args.feature_extractor
    multistep = getattr(args, "personalize_num_grad_steps", None) is not None
    if getattr(args, "vit_bf16", False):
        if not fe.startswith("vit_"):
            print("note: --vit_bf16 is ignored for --feature_extractor %s (bf16 token GEMMs exist for the vit_* extractors only)" % fe)
            args.vit_bf16 = False
        elif "train" in args.mode:
            sys.exit("error: --vit_bf16 is an inference mode (bf16 token GEMMs have no backward): use --mode test, got --mode %s"
                     % args.mode)
        elif multistep and (args.learn_extractor or args.adapt_features):
            sys.exit("error: --vit_bf16 is an inference mode: the finetuner's --learn_extractor / --adapt_features send gradients "
                     "through the extractor, which a bf16 plan refuses")
    resample = getattr(args, "vit_resample_pos_embed", False)
    if resample:
        S = args.frame_size
        if not fe.startswith("vit_"):
            print("note: --vit_resample_pos_embed is ignored for --feature_extractor %s (it runs at any --frame_size already; the "
                  "position table belongs to the vit_* extractors)" % fe)
            resample = args.vit_resample_pos_embed = False
        elif S != 224:
            patch = 16 if fe.split("_")[2] == "16" else 32
            if S > 512:
                sys.exit("error: --vit_resample_pos_embed covers --frame_size 32..512 (got %d)" % S)
            if S % patch:
                sys.exit("error: --vit_resample_pos_embed: --frame_size %d is not a multiple of %s's patch size %d; the nearest "
                         "valid sizes are %d and %d" % (S, fe, patch, max(S // patch * patch, patch), (S // patch + 1) * patch))
            if "train" in args.mode:
                sys.exit("error: --vit_resample_pos_embed at --frame_size %d is an inference mode (the native backward runs on "
                         "224x224 frames only): use --mode test, got --mode %s" % (S, args.mode))
            if multistep and (args.learn_extractor or args.adapt_features):
                sys.exit("error: --vit_resample_pos_embed at --frame_size %d is an inference mode: the finetuner's "
                         "--learn_extractor / --adapt_features send gradients through the extractor, which runs its backward on "
                         "224x224 frames only" % S)
    spec = FROZEN_EXTRACTORS.get(fe)
    if spec is None:
        return
    args.frame_norm_method = spec.frame_norm
    if spec.frame_size is not None and args.frame_size != spec.frame_size and not resample:
        sys.exit("error: --feature_extractor %s needs --frame_size %d (got %d)" % (fe, spec.frame_size, args.frame_size))
    scope, flag, _ = opted_in(args, spec)
    if scope == "all":
        pass  # native gradients of every parameter: everything the other extractors train is admitted
    elif scope == "film":
        if args.learn_extractor:
            sys.exit("error: --%s gives FiLM gradients through a frozen %s only: --learn_extractor (%s) is not built"
                     % (flag, fe, spec.no_weights))
    elif "train" in args.mode or args.learn_extractor or args.with_lite or (multistep and args.adapt_features):
        sys.exit("error: --feature_extractor %s is inference-only here (no backward through %s): use --mode test "
                 "without --learn_extractor / --with_lite%s" % (fe, spec.no_backward, " / --adapt_features" if multistep else ""))


def frame_accuracy(logits, label):
    """reference utils/eval_metrics.py:27-36"""
    return (logits.argmax(dim=-1) == label).float().mean().item()


def mean_ci(values):
    """mean and 95 % confidence half-width, as the reference's evaluators report (utils/eval_metrics.py:24-25)."""
    v = np.asarray(values, dtype=np.float64)
    if len(v) == 0:  # a rank (or a run) that saw no task: no statistic (None: json.dump would write a bare NaN, invalid JSON)
        return None, 0.0
    return float(v.mean()), float(1.96 * v.std() / math.sqrt(len(v))) if len(v) > 1 else 0.0


ORBIT_METRICS = ["frame_acc", "frames_to_recognition"]


class OrbitMetrics:
    """The ORBIT benchmark's evaluation beside a test loop's own figures: a TestEvaluator (utils/eval_metrics.py) fed with
    every target video's device logits - one orbit_video_metrics launch per task - that reports frame accuracy and
    frames-to-recognition averaged per user, object, task and video, and video accuracy per object and video."""

    def __init__(self, save_dir=None):
        self.save_dir = save_dir
        self.evaluator = TestEvaluator(ORBIT_METRICS, save_dir=save_dir)
        self.tasks = []  # (global task index, user key, object list) of the tasks fed, in order

    def begin_task(self, index, user, object_list=None):
        if self.tasks:  # a new user where the key changes, as the reference's loop (single-step-learner.py:348-357)
            if user != self.tasks[-1][1]:
                self.evaluator.set_current_user(self.tasks[-1][1])
                self.evaluator.next_user()
            else:
                self.evaluator.next_task()
        self.tasks.append((index, user, object_list))
        if object_list is not None:
            self.evaluator.set_task_object_list(object_list)

    def append_video(self, logits, label, paths=None):
        self.evaluator.append_video(logits, label, paths)

    def gather(self, world, with_predictions):
        """world > 1: every rank's per-video INTEGERS (not its scores) through all_gather_object, re-assembled in global task
        order, so every rank reports what a single-GPU run over the same tasks reports."""
        if world == 1:
            return self
        import torch.distributed as dist
        self.evaluator._flush()
        mine = [t for user in self.evaluator.all_video_results for t in user if t]
        assert len(mine) == len(self.tasks)
        payload = [(tag, [([s.as_tuple() for s in v.segments], v.preds.tolist() if with_predictions else None,
                           v.paths if with_predictions else None) for v in videos]) for tag, videos in zip(self.tasks, mine)]
        gathered = [None] * world
        dist.all_gather_object(gathered, payload)
        merged = OrbitMetrics(self.save_dir)
        for (index, user, object_list), videos in sorted((x for g in gathered for x in g), key=lambda x: x[0][0]):
            merged.begin_task(index, user, object_list)
            for video in videos:
                merged.evaluator.append_video_segments(*video)
        return merged

    def report(self):
        """{"user" | "object" | "task" | "video": {stat: [mean, ci]}} or None when no video was fed"""
        ev = self.evaluator
        if not self.tasks:
            return None
        if len(ev.all_users) == ev.current_user:
            ev.set_current_user(self.tasks[-1][1])
        levels = dict(zip(("user", "object", "task", "video"), ev.get_mean_stats()))
        video, obj = ev.get_video_and_object_stats()
        levels["video"].update(video)
        levels["object"].update(obj)
        return {level: {k: [float(x) for x in v] for k, v in stats.items()} for level, stats in levels.items()}

    @staticmethod
    def line(report):
        if report is None:
            return "orbit metrics: no target video"
        return "orbit metrics, % (95 % ci): " + " | ".join(
            "per %s %s" % (level, ", ".join("%s %.2f (%.2f)" % (k, 100 * m, 100 * c) for k, (m, c) in report[level].items()))
            for level in ("user", "object", "task", "video"))


def _shown(stat):
    """(mean, ci) for a print statement: NaN where mean_ci had no data"""
    return (float("nan") if stat[0] is None else stat[0]), stat[1]


def timed_ms(fn, *args):
    """fn(*args) between two device synchronisations -> (its result, milliseconds)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def gather_lists(world, *lists):
    """this rank's lists -> those of all ranks, each flattened in rank order: every rank holds the statistics of the whole run"""
    if world == 1:
        return lists
    import torch.distributed as dist
    gathered = [None] * world
    dist.all_gather_object(gathered, lists)
    return tuple([x for g in gathered for x in g[i]] for i in range(len(lists)))


def host_state(model):
    """model.state_dict() on the host: what every file the learner saves holds"""
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


class Learner:
    strict_load = True  # load_state_dict(strict=) of --model_path
    # state that appears during a run (None: not there yet)
    best_validation = None  # (mean, ci) of the best validation so far; None: no validation has beaten 0 yet
    validation_history = None  # [(epoch, mean, better)], one entry per validate()
    gradless_parameters = None  # diagnostic: the parameters without a gradient at the first optimizer step
    grad_bucket = stat_sync = None  # multi-GPU training (dist.GradientBucket, dist.RunningStatSync)
    _pool = _split_index = _train_items = _validation_dataset = None  # dataset trees: see decode_pool, build_dataset, validate

    def __init__(self, args):
        self.args = args
        verify_args(args)
        self.rank, self.world, self.local_rank = odist.init_from_env()
        np.random.seed(args.seed)  # the reference leaves numpy unseeded; LITE's permutation needs it
        torch.manual_seed(args.seed)
        index = args.gpu if self.world == 1 else self.local_rank
        torch.cuda.set_device(index)
        self.device = torch.device("cuda", index)
        self.init_model()
        import gc
        gc.collect()
        gc.freeze()  # keep torch + the model out of the cyclic collector's working set (full collections cost ms)

    def new_recogniser(self):
        a = self.args
        return SingleStepFewShotRecogniser(a.feature_extractor, a.adapt_features, a.classifier, a.clip_length, a.batch_size,
                                           a.learn_extractor, a.num_lite_samples, a.logit_scale)

    def init_model(self):
        a = self.args
        self.model = self.new_recogniser()
        if a.model_path:
            # reference single-step-learner.py:300-302. The FiLM generator's gamma0/beta0 snapshot is not part of the file
            # (feature_adapters.py:55-58); the recogniser re-takes it from the loaded extractor (load_state_dict hook)
            self.model.load_state_dict(torch.load(a.model_path, map_location="cpu"), strict=self.strict_load)
        else:
            synthetic.init_parameters_(self.model, seed=a.seed,
                                       film_strength=0.02 if a.feature_extractor == "efficientnet_b0" else 0.1)
        spec = FROZEN_EXTRACTORS.get(a.feature_extractor)
        for attr in opted_in(a, spec)[2] if spec else ():
            setattr(self.model.feature_extractor, attr, True)
        if getattr(a, "vit_bf16", False):  # (verify_args cleared it for the other extractors)
            self.model.feature_extractor.bf16_inference = True
        if getattr(a, "vit_resample_pos_embed", False):  # (the same)
            self.model.feature_extractor.resample_pos_embed = True
        self.model._set_device(self.device)
        self.model._send_to_device()

    def synthetic_task(self, index):
        a = self.args
        per_class = a.shots * a.frames_per_shot
        per_class -= per_class % a.clip_length
        return synthetic.make_task(index, a.way, 1, per_class, a.num_query_videos * a.frames_per_video, a.frame_size,
                                   clip_length=a.clip_length, seed=a.seed)

    def make_task(self, index):
        """synthetic test / validation task `index` in the layout a tree's test-mode tasks have (data/pipeline.py), frames on
        the host: the query frames grouped into videos (reference: target_frames_by_video) by their row ranges, one label per
        frame - a synthetic "video" mixes objects. One user is one task."""
        a = self.args
        task = self.synthetic_task(index)
        task["target_clips"] = task["target_clips"][:, -1:]  # [M,1,3,H,W]: a video's frames are the LAST frame of its query clips
        task["target_videos"] = [(v * a.frames_per_video, (v + 1) * a.frames_per_video) for v in range(a.num_query_videos)]
        task["user"] = index
        return task

    def run(self):
        """train / test / train_test as the reference's run() (single-step-learner.py:136-193): after training, train_test
        tests the FINAL model and then the best-validation checkpoint (`test(self.checkpoint_path_validation)`, :186-188), so
        the model `best_validation` selected is the one a second test block reports (`test_best_validation`)."""
        stats = {}
        if "train" in self.args.mode:
            stats["train"] = self.train()
        if "test" in self.args.mode:
            stats["test"] = self.test()
            best_path = self.args.save_best_model_path
            if "train" in self.args.mode and self.best_validation is not None and best_path:
                if self.world > 1:  # rank 0 wrote the file (validate()): every rank loads it after the write is complete
                    import torch.distributed as dist
                    dist.barrier()
                self.model.load_state_dict(torch.load(best_path, map_location="cpu"))
                self.model._send_to_device()
                if self.rank == 0:
                    print("testing the best-validation checkpoint %s" % best_path)
                stats["test_best_validation"] = self.test()
        return stats

    # ---- meta-training (reference single-step-learner.py:128-243) ----------------------------------------------------
    def make_train_task(self, index):
        return self.synthetic_task(10_000 + index)

    def train_task(self, task):
        a = self.args
        self.model.personalise(task["context_clips"], self._labels_to_device(task["context_labels"]))
        target_logits = self.model.predict(task["target_clips"])
        task_loss = cross_entropy(target_logits, task["target_labels"].to(self.device)) / a.tasks_per_batch
        task_loss = task_loss + 0.001 * self.model.film_generator.regularization_term()
        task_loss.backward()
        self.model._reset()
        return task_loss.detach(), target_logits.detach()

    def train_task_with_lite(self, task):
        a = self.args
        context_clips, context_labels = task["context_clips"], self._labels_to_device(task["context_labels"])
        target_clips, target_labels = task["target_clips"], task["target_labels"]
        self.model._clear_caches()
        task_loss, target_logits = 0, []
        num_clips = len(target_clips)
        num_batches = int(np.ceil(float(num_clips) / float(a.batch_size)))
        for batch in range(num_batches):
            self.model.personalise_with_lite(context_clips, context_labels)
            lo, hi = batch * a.batch_size, min((batch + 1) * a.batch_size, num_clips)
            batch_target_logits = self.model.predict_a_batch(target_clips[lo:hi])
            target_logits.append(batch_target_logits.detach())
            loss_scaling = len(context_labels) / (a.num_lite_samples * a.tasks_per_batch)
            batch_loss = loss_scaling * cross_entropy(batch_target_logits, target_labels[lo:hi].to(self.device))
            batch_loss = batch_loss + 0.001 * self.model.film_generator.regularization_term()
            batch_loss.backward()
            task_loss += batch_loss.detach()
            self.model._reset()
        return task_loss, torch.cat(target_logits)

    def _sync_gradients(self):
        """X3 of SURVEY.md §8e: one all-reduce(SUM) of the persistent flat gradient bucket per optimizer step (+ the
        running statistics, averaged). Parameters that receive no gradient on any rank keep grad None, so the optimizer
        skips them as the single-GPU run and the reference do (dist.GradientBucket)."""
        if self.world == 1:
            return
        self.grad_bucket.sync()
        if self.model.learn_extractor:
            # train-mode BatchNorm: the window's running-statistic updates of all ranks, combined as the reference's
            # sequential updates would have been (dist.RunningStatSync; round 2 averaged the ranks' values)
            self.stat_sync.sync()  # (in-place copies: the plans see the new buffer versions and re-upload them)

    # ---- tasks from a dataset tree (--data_path / --data_root) -----------------------------------------------------------
    def decode_pool(self):
        """the threads that decode (or, with --decode device, read and parse) the frames of every tree loop: --num_workers of
        them, never the CPU count"""
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=max(1, int(self.args.num_workers)))
        return self._pool

    def _close_decode_pool(self):
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def build_dataset(self, split, frames=None):
        """The dataset the `split` loop ("train", "validation" or "test") samples its tasks from, on this rank's sampling
        stream. frames: what the clips hold (data/datasets.py); default "jpeg" for --decode device, else "uint8" - the two
        forms TaskPrefetcher uploads."""
        a = self.args
        root = split_roots(a).get(split)
        if root is None:
            raise ValueError("--mode %s%s reads no %s split from a tree"
                             % (a.mode, "" if a.data_path or a.data_root else " without --data_path", split))
        if frames is None:
            frames = "jpeg" if a.decode == "device" else "uint8"
        dataset = build_split_dataset(a, split, root, frames, self.rank, None if frames == "paths" else self.decode_pool())
        if self._split_index is None:
            self._split_index = {}
        self._split_index[split] = dataset.index_summary()
        return dataset

    def annotation_stats(self, split):
        """the annotation side of a split's results: the flags as expanded, and what the index kept and the filters dropped
        (data/datasets.index_summary; None on synthetic tasks)"""
        to_load, (context, target) = split_annotation_args(self.args, split)
        return {"filter_context": list(context), "filter_target": list(target), "annotations_to_load": list(to_load),
                "index": (self._split_index or {}).get(split)}

    def ingest_stats(self, prefetch, tree):
        """the input pipeline's side of a tree loop's results (`prefetch` None: tasks that did not come through it): the sizes
        the frames were stored at and run at, the resize filter if one ran, and where the frames were decoded"""
        a = self.args
        stored = sorted(prefetch.stored_sizes) if prefetch is not None else []  # (this rank's tasks)
        return {"stored_frame_size": [list(hw) for hw in stored], "frame_size": [a.frame_size, a.frame_size],
                "resample": a.resample if any(hw != (a.frame_size, a.frame_size) for hw in stored) else None,
                "decode": a.decode if tree else None,
                "decode_fallback_frames": prefetch.fallback_frames if prefetch is not None and a.decode == "device" else None}

    def train_order(self, epoch):
        """this rank's item indices (users; objects when object-centric) of train epoch `epoch`, in the order it trains on them:
        the queue's shuffled order (task_order: the same on every rank), dealt round-robin"""
        a = self.args
        return task_order(self._num_train_items(), a.num_train_tasks, a.seed, epoch)[self.rank::self.world]

    def _num_train_items(self):
        if self._train_items is None:
            self._train_items = num_items(self.build_dataset("train", frames="paths"))
        return self._train_items

    def _prefetch(self, dataset, indices, depth):
        """dataset[i] for i in indices, staged on the device: decode / file reads on the pool, 8-bit or compressed upload,
        decode, resize and normalisation on the copy stream (data/pipeline.TaskPrefetcher), `depth` tasks in flight"""
        from .data.pipeline import DatasetTaskSource, TaskPrefetcher
        a = self.args
        self.model.frame_norm_method = a.frame_norm_method
        return TaskPrefetcher(DatasetTaskSource(dataset, indices), self.device, depth=depth, frame_norm_method=a.frame_norm_method,
                              frame_size=a.frame_size, resample=a.resample)

    def _init_training(self):
        """optimizer, schedule, --resume and, multi-GPU, the gradient and running-statistics exchange -> the epoch to start at"""
        a = self.args
        self.optimizer = init_optimizer(self.model, a.learning_rate, a.optimizer, a, a.extractor_lr_scale)
        self.scheduler = init_scheduler(self.optimizer, a)  # applies f(0) * lr_scale (default: the constant --learning_rate)
        start_epoch = self.load_checkpoint() if a.resume else 0
        self.grad_bucket = None
        if self.world > 1:
            p2p = None
            if a.p2p_gradients:
                cap = sum(-(-q.numel() // 64) * 64 for q in self.model.parameters() if q.requires_grad)
                p2p = odist.P2PAllReduce(self.rank, self.world, odist.P2PAllReduce.floats_for_bucket(cap, self.world))
            self.grad_bucket = odist.GradientBucket(self.model.parameters(), p2p=p2p)
            if self.model.learn_extractor:
                self.stat_sync = odist.RunningStatSync(self.model.feature_extractor, self.model.feature_extractor.bn_momentum)
        return start_epoch

    @contextlib.contextmanager
    def _train_tasks(self, task_source, start_epoch):
        """-> (tasks, prefetch): ONE iterator of (task, ms waited for it) over this rank's train tasks of all epochs from
        `start_epoch` - handed in, from the tree, or synthetic (waited None) - and the tree's prefetcher (else None), which is
        closed with its pool, and the recogniser's lite_query_overlap put back, on leaving."""
        a = self.args
        prefetch, lite_query_overlap = None, self.model.lite_query_overlap
        if task_source is None and split_roots(a).get("train"):
            # ONE prefetcher over all epochs (the first tasks of epoch e+1 are staged under the validation of epoch e), two
            # slots: the step is longer than the staging of a task, a third slot would only hold memory.
            # A slot must not be refilled while any stream of the recogniser still reads it (LITE's subset pass and its
            # query pass run on side streams): the loop SYNCHRONISES THE DEVICE after every task's step - the step's timer needs
            # that anyway - before it asks for the next task, so no consumer_streams are passed to the prefetcher.
            dataset = self.build_dataset("train")
            self._train_items = num_items(dataset)
            prefetch = self._prefetch(dataset, [i for epoch in range(start_epoch, a.epochs) for i in self.train_order(epoch)],
                                      depth=2)
            # The yielded clips are complete on the caller's stream when next() returns (it waits for the slot's event), so the
            # query batch's taped pass may start from LITE's fork point as it does for clips on the host: the same kernels,
            # and the same deferred running-statistics update, whether a task comes from the tree or from host tensors
            self.model.lite_query_overlap = bool(self.model.lite_overlap)
        try:
            if task_source is None and prefetch is None:
                yield self._synthetic_train_tasks(start_epoch), None
            else:
                yield self._waited_for(prefetch if task_source is None else task_source), prefetch
        finally:
            self.model.lite_query_overlap = lite_query_overlap
            if prefetch is not None:
                prefetch.close()
                self._close_decode_pool()

    @staticmethod
    def _waited_for(tasks):
        t0 = time.perf_counter()
        for task in tasks:  # (a prefetcher hands the previous task's slot back: the device is idle, see _train_tasks)
            yield task, 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()

    def _synthetic_train_tasks(self, start_epoch):
        a = self.args
        for epoch in range(start_epoch, a.epochs):
            # this rank's tasks of the epoch are generated up front (the reference prefetches with DataLoader
            # workers): generating them between steps leaves the intra-op CPU threads spinning against the thread
            # that enqueues kernels, which showed up as random 50-80 ms stalls per task
            mine = [s_ for s_ in range(a.num_train_tasks) if s_ % self.world == self.rank]
            task_bytes = 4.0 * 3 * a.frame_size ** 2 * a.way * (a.shots * a.frames_per_shot
                                                               + a.num_query_videos * a.frames_per_video)
            pregen = {s_: self.make_train_task(epoch * a.num_train_tasks + s_) for s_ in mine} \
                if task_bytes * len(mine) < 16e9 else {}
            for step in mine:
                yield pregen.pop(step, None) or self.make_train_task(epoch * a.num_train_tasks + step), None

    def train(self, task_source=None):
        """task_source: an iterable of this rank's train tasks (task dicts as data/datasets.py returns them, all epochs in
        train_order order - with --resume those from the checkpoint's epoch on) that stands in for the tree and the prefetcher;
        loop, seeds and step boundaries are the same."""
        a = self.args
        if not split_roots(a).get("train") and a.data_root and self.rank == 0:
            print("train: --data_root names a test split only: training runs on synthetic tasks (use --data_path ROOT)")
        start_epoch = self._init_training()
        # per task, in this rank's order: the losses are what a run on the same tasks must reproduce
        log = types.SimpleNamespace(losses=[], accs=[], ms=[], wait_ms=[], frames=[], lr_history=[], num_updates=0)
        self.task_losses, self.task_ms, self.task_wait_ms = log.losses, log.ms, log.wait_ms
        t_all = time.perf_counter()
        prev = torch.is_grad_enabled()
        torch.set_grad_enabled(True)
        try:
            with self._train_tasks(task_source, start_epoch) as (tasks, prefetch):
                self.model.set_test_mode(False)
                for epoch in range(start_epoch, a.epochs):
                    self._train_epoch(epoch, tasks, log)
        finally:
            torch.set_grad_enabled(prev)
        wall = time.perf_counter() - t_all
        if self.grad_bucket is not None and self.grad_bucket.p2p is not None:
            # every optimizer step checked the exchange before it (GradientBucket.sync); this covers the last one: a peer
            # that stalled makes this rank raise instead of saving parameters updated from NaN-poisoned gradients
            torch.cuda.synchronize()
            self.grad_bucket.p2p.raise_on_error()
        if a.save_model_path and self.rank == 0:  # every rank holds the same parameters after the last step
            torch.save(host_state(self.model), a.save_model_path)
        return self._train_report(log, prefetch, start_epoch, wall)

    def _train_epoch(self, epoch, tasks, log):
        """one epoch of the reference's loop (single-step-learner.py:143-182): this rank's share of the epoch's steps, an
        optimizer step every --tasks_per_batch steps and after the last one, the schedule, validation, the checkpoint"""
        a = self.args
        first_loss = len(log.losses)
        # with --data_path: --num_train_tasks per user (or object), in the queue's order (task_order)
        total_steps = a.num_train_tasks * (self._num_train_items() if split_roots(a).get("train") else 1)
        for step in range(total_steps):
            if step % self.world == self.rank:
                self._train_step(epoch, step, total_steps, *next(tasks), log)
            if (step + 1) % a.tasks_per_batch == 0 or step == total_steps - 1:
                self._optimizer_step(log)
        lr, fe_lr = get_curr_learning_rates(self.optimizer)[:2]  # reference :170-174
        log.lr_history.append((lr, fe_lr))
        if self.rank == 0:
            losses = log.losses[first_loss:]
            print("epoch [%d/%d] train loss: %.7f lr: %.3e fe-lr: %.3e"
                  % (epoch + 1, a.epochs, float(np.mean(losses)) if losses else float("nan"), lr, fe_lr))
        self.scheduler.step(epoch + 1)  # before validation, the reference's order (:177-181)
        if a.num_val_tasks > 0 and (epoch + 1) >= a.validation_on_epoch:
            self.validate(epoch + 1)
            torch.set_grad_enabled(True)
            self.model.set_test_mode(False)
        self.save_checkpoint(epoch + 1)

    def _train_step(self, epoch, step, total_steps, task, wait_ms, log):
        """the timed step of one task: the device is synchronised before and after it"""
        a = self.args
        if wait_ms is not None:
            log.wait_ms.append(wait_ms)
            log.frames.append(sum(int(np.prod(task[k].shape[:2])) for k in ("context_clips", "target_clips")))
        # LITE draws its subsets from np.random (few_shot_recognisers.py:330); seeding per TASK (the
        # reference leaves numpy unseeded) makes a run independent of how tasks are dealt to ranks
        np.random.seed((a.seed + 7919 * (epoch * total_steps + step + 1)) % (2 ** 32))
        (task_loss, logits), ms = timed_ms(self.train_task_with_lite if a.with_lite else self.train_task, task)
        log.ms.append(ms)
        log.losses.append(float(task_loss))
        log.accs.append(frame_accuracy(logits.cpu(), task["target_labels"].cpu()))
        if a.print_by_step:
            print("epoch [%d/%d][%d/%d] rank %d train loss %.7f frame_acc %.3f  %.1f ms/task"
                  % (epoch + 1, a.epochs, step + 1, total_steps, self.rank, log.losses[-1], log.accs[-1], ms))

    def _optimizer_step(self, log):
        self._sync_gradients()
        if self.gradless_parameters is None:  # diagnostic, first optimizer step only
            self.gradless_parameters = sorted(n for n, p in self.model.named_parameters() if p.requires_grad and p.grad is None)
        self.optimizer.step()
        if self.grad_bucket is not None:
            if self.model.learn_extractor:
                self.stat_sync.begin()  # the next window's running statistics start from here
            self.grad_bucket.zero_()  # one memset; gradients keep living inside the flat bucket
        else:
            self.optimizer.zero_grad()
        log.num_updates += 1
        self.scheduler.step_update(log.num_updates)  # (a no-op for epoch schedules, where the reference calls it: :166)

    def _train_report(self, log, prefetch, start_epoch, wall):
        """-> train()'s result dict, summarised in one or two lines by rank 0"""
        a = self.args
        tree = split_roots(a).get("train")
        lr, fe_lr = log.lr_history[-1] if log.lr_history else (None, None)
        loss, acc, ms = (mean_ci(values) if values else (0.0, 0.0) for values in (log.losses, log.accs, log.ms))
        stats = {"loss": loss, "frame_acc": acc, "ms_per_task": ms, "num_tasks": len(log.losses), "world_size": self.world,
                 "validation": self.validation_history, "best_validation": self.best_validation,
                 "lr": lr, "fe_lr": fe_lr, "lr_history": log.lr_history, "start_epoch": start_epoch}
        # the tree's side of the run (None / empty on synthetic tasks). ms_per_task is the step alone; data_wait_ms is the time
        # the loop was blocked in next() on the prefetcher, per task; wall_s covers both, validation and the optimizer steps
        stats.update(self.ingest_stats(prefetch, tree))
        stats.update({"data_path": a.data_path if tree else None, "train_task_type": a.train_task_type if tree else None,
                      "data_wait_ms": mean_ci(log.wait_ms) if log.wait_ms else None,
                      "frames_per_task": mean_ci(log.frames) if log.frames else None, "wall_s": wall})
        stats.update(self.annotation_stats("train"))
        stats["validation_annotations"] = self.annotation_stats("validation") if split_roots(a).get("validation") else None
        if self.rank == 0:
            print("train: loss %.5f | frame_acc %.2f %% | %.1f ms/task | %d tasks on this rank, %d GPU(s)"
                  % (stats["loss"][0], 100 * stats["frame_acc"][0], stats["ms_per_task"][0], stats["num_tasks"], self.world))
            if log.frames:
                print("train (%s): %.0f frames per task | waited %.1f (%.1f) ms per task for data (decode: %s, %d threads) | "
                      "%.2f tasks/s of wall time"
                      % ("%s, %s" % (a.data_path, a.train_task_type) if prefetch is not None else "tasks handed in",
                         stats["frames_per_task"][0], *stats["data_wait_ms"], a.decode, a.num_workers,
                         stats["num_tasks"] / max(wall, 1e-9)))
        return stats

    def save_checkpoint(self, epoch):
        """reference single-step-learner.py:377-383: DIR/checkpoint.pt with its four keys, written by rank 0 (every rank holds
        the same parameters and optimizer state after a step). Written AFTER the epoch's validation - the reference writes it
        before - so that best_stats covers the epoch the file names and a resumed run takes the decisions of a straight one.
        The file is replaced atomically: an interruption during the write leaves the previous epoch's checkpoint."""
        directory = self.args.checkpoint_dir
        if not directory or self.rank != 0:
            return
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, "checkpoint.pt")
        torch.save({"epoch": epoch, "model_state_dict": host_state(self.model), "optimizer_state_dict": self.optimizer.state_dict(),
                    "best_stats": {"best_validation": self.best_validation, "validation_history": self.validation_history}},
                   path + ".tmp")
        os.replace(path + ".tmp", path)

    def load_checkpoint(self):
        """reference single-step-learner.py:385-390: model, optimizer state and best validation stats from
        --checkpoint_dir/checkpoint.pt. -> the epoch to continue at; the schedule is set to f(epoch)."""
        path = os.path.join(self.args.checkpoint_dir, "checkpoint.pt")
        checkpoint = torch.load(path, map_location="cpu")
        self.model.load_state_dict(checkpoint["model_state_dict"])
        self.optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
        best = checkpoint.get("best_stats") or {}
        if best.get("best_validation") is not None:
            self.best_validation = tuple(best["best_validation"])
        if best.get("validation_history") is not None:
            self.validation_history = list(best["validation_history"])
        epoch = int(checkpoint["epoch"])
        self.scheduler.step(epoch)
        if self.rank == 0:
            print("resumed from %s: continuing at epoch %d of %d" % (path, epoch + 1, self.args.epochs))
        return epoch

    # ---- the evaluation loop of test and validation (reference single-step-learner.py:245-375) ----------------------------
    def _labels_to_device(self, labels):
        """the reference's unpack_task (data/utils.py:42-43) for the context labels; the label set rides along from the host copy"""
        return unpack_task({"context_labels": labels, "target_labels": None, "context_clips": None, "target_clips": None},
                           self.device)[2]

    def _personalise(self, context_clips, context_labels):
        self.model.personalise(context_clips, context_labels)

    def _predict_video(self, frames):
        # = predict(attach_frame_history(frames, clip_length)) of the reference loop, frames not duplicated
        return self.model.predict_video(frames)

    def _evaluate(self, tasks, indices=None, metrics=None):
        """The reference's test and validation loops (single-step-learner.py:262-281, 316-341) over an iterable of test-mode
        tasks - a TaskPrefetcher's on the device or make_task's on the host, the loop does not ask: per task personalise on the
        context clips, then per target VIDEO (task["target_videos"]: row ranges of target_clips [M,1,3,H,W]) predict on its frame
        history, frame accuracy, _reset. metrics (OrbitMetrics) is fed every video; indices[k] is the k-th task's global index.
        -> per task {"accs": per-video frame accuracies, "personalise_ms", "inference_ms": per video and frame, "frames"}"""
        self.model.set_test_mode(True)
        records = []
        with torch.no_grad():
            for k, task in enumerate(tasks):
                if metrics is not None:
                    metrics.begin_task(indices[k], task["user"], task.get("object_list"))
                # the labels' copies - the context set's to the device, the frames' to the host - stay outside the timers
                context_labels, labels = self._labels_to_device(task["context_labels"]), task["target_labels"].cpu()
                _, personalise_ms = timed_ms(self._personalise, task["context_clips"], context_labels)
                accs, inference_ms = [], []
                target = task["target_clips"][:, 0]  # [M,3,H,W]: the videos' frames, in video order
                for v, (lo, hi) in enumerate(task["target_videos"]):
                    logits, ms = timed_ms(self._predict_video, target[lo:hi])
                    inference_ms.append(ms / float((hi - lo) * self.model.clip_length))
                    accs.append(frame_accuracy(logits.cpu(), labels[lo:hi]))
                    if metrics is not None:
                        # one label per frame: a tree's video repeats its object's label - one run of labels, which is what
                        # its single label gives (TestEvaluator.append_video) - and a synthetic "video" mixes objects
                        paths = task["target_paths"][v] if task.get("target_paths") is not None else None
                        metrics.append_video(logits, labels[lo:hi], paths)
                self.model._reset()
                records.append({"accs": accs, "personalise_ms": personalise_ms, "inference_ms": inference_ms,
                                "frames": sum(hi - lo for lo, hi in task["target_videos"])})
        return records

    def validate(self, epoch=0):
        """The reference's validate() (single-step-learner.py:245-296) on held-out tasks - synthetic ones, or with
        --data_path the validation split's - through the evaluation loop; the
        model whose mean per-video accuracy beats the best so far (ValidationEvaluator.is_better, utils/eval_metrics.py:351-357:
        strictly greater, starting from 0) is written to --save_best_model_path. Tasks are dealt to the ranks and the
        per-video accuracies gathered, so every rank takes the same decision."""
        a = self.args
        prefetch = None
        if split_roots(a).get("validation"):
            # --data_path: --num_val_tasks tasks per user of ROOT/validation in the queue's unshuffled order, each run as the
            # test loop runs a task. The sampling stream restarts with every call, so every epoch's model is scored on the
            # same tasks and "strictly greater" compares like with like.
            if self._validation_dataset is None:
                self._validation_dataset = self.build_dataset("validation")
            dataset = self._validation_dataset
            dataset.rng = split_rng(a, "validation", self.rank)
            order = task_order(num_items(dataset), a.num_val_tasks)
            tasks = prefetch = self._prefetch(dataset, order[self.rank::self.world], depth=3)
        else:
            tasks = (self.make_task(20_000 + t) for t in odist.tasks_for_rank(a.num_val_tasks, self.rank, self.world))
        accs, = gather_lists(self.world, [x for record in self._evaluate(tasks) for x in record["accs"]])
        if prefetch is not None:
            prefetch.close()
        stat = mean_ci(accs)
        better = stat[0] is not None and stat[0] > (self.best_validation or (0.0, 0.0))[0]
        if better:
            self.best_validation = stat
            if a.save_best_model_path and self.rank == 0:
                torch.save(host_state(self.model), a.save_best_model_path)
        self.validation_history = (self.validation_history or []) + [(epoch, stat[0], better)]
        if self.rank == 0:
            print("validation (epoch %d): per-video frame_acc %.2f (%.2f) %% over %d videos%s"
                  % (epoch, 100 * _shown(stat)[0], 100 * stat[1], len(accs), " - best so far, model saved" if better else ""))
        return stat

    def _test_prefetcher(self, root):
        """-> (the global indices of this rank's test tasks on the tree, the prefetcher that yields them). The reference's test
        queue (data/queues.py:44-46 -> data/datasets.py; pinned by fixture G14): every user's objects, all their videos, context
        clips sampled uniformly, 200 random clips per target video. Decode, 8-bit upload and normalisation of task i+1 overlap
        the extractor work of task i; a tree stored at another size than --frame_size is resized to it in the normalisation
        launch (--resample)."""
        a = self.args
        dataset = self.build_dataset("test")
        # TaskSampler order (data/samplers.py:24-30, no shuffle): user 0 x num_tasks, user 1 x num_tasks, ...; dealt to ranks
        # - EVERY user x num_test_tasks_per_user, as the reference's loop visits them (single-step-learner.py:313-314). An
        # optional total cap (--max_test_tasks; default none) is applied BEFORE the tasks are dealt, so the evaluated set does
        # not depend on the world size, and is announced when it truncates the user list
        order = [u for u in range(len(dataset)) for _ in range(a.num_test_tasks_per_user)]
        if a.max_test_tasks is not None and a.max_test_tasks < len(order):
            if self.rank == 0:
                print("test (%s): --max_test_tasks %d truncates %d tasks (%d users x %d) - NOT the full test set"
                      % (root, a.max_test_tasks, len(order), len(dataset), a.num_test_tasks_per_user))
            order = order[:a.max_test_tasks]
        return range(len(order))[self.rank::self.world], self._prefetch(dataset, order[self.rank::self.world], depth=3)

    def test(self):
        """The reference's test loop (single-step-learner.py:298-375) through the evaluation loop, on --num_test_tasks synthetic
        tasks or on a tree (--data_root, or --data_path's <--test_set> split: one task per user and --num_test_tasks_per_user):
        frame accuracy per video averaged per task, the two timers and the ORBIT metrics, gathered from all ranks."""
        a = self.args
        root = split_roots(a).get("test")
        save_dir = a.save_predictions if root else None
        metrics, prefetch, t_all = OrbitMetrics(save_dir), None, time.perf_counter()
        if root:
            indices, prefetch = self._test_prefetcher(root)
            tasks = prefetch
        else:
            # (synthetic tasks live on the host and are uploaded per mini-batch: in its default mode, overlap_query = "auto", the
            # recogniser runs the query pass of predict() on its own stream for such clips)
            indices = odist.tasks_for_rank(a.num_test_tasks, self.rank, self.world)
            tasks = (self.make_task(t) for t in indices)
        records = self._evaluate(tasks, indices, metrics)
        if prefetch is not None:
            prefetch.close()
            self._close_decode_pool()
        wall = time.perf_counter() - t_all
        records, = gather_lists(self.world, records)  # per-task results of every rank
        metrics = metrics.gather(self.world, with_predictions=bool(save_dir))
        stats = {"frame_acc": mean_ci([float(np.mean(r["accs"])) for r in records]),
                 "personalise_ms": mean_ci([r["personalise_ms"] for r in records]),
                 "inference_ms_per_frame": mean_ci([ms for r in records for ms in r["inference_ms"]]),
                 "num_tasks": len(records), "world_size": self.world, "orbit_metrics": metrics.report()}
        if a.feature_extractor.startswith("vit_"):  # the precision of the transformer's token GEMMs (--vit_bf16)
            stats["vit_precision"] = "bf16" if getattr(a, "vit_bf16", False) else "fp32"
            stats["vit_frame_size"] = [a.frame_size, a.frame_size]  # the frames the plan ran at (--vit_resample_pos_embed)
        if prefetch is not None:
            stats.update({"target_frames": sum(r["frames"] for r in records), "wall_s": wall, "data_root": root})
            stats.update(self.ingest_stats(prefetch, root))
            stats.update(self.annotation_stats("test"))
        if self.rank == 0:
            self._report_test(stats, prefetch)
            if save_dir and stats["orbit_metrics"] is not None:
                metrics.evaluator.save()
                print("predictions written to %s" % metrics.evaluator.json_results_path)
            if a.results_path:
                with open(a.results_path, "w") as f:
                    json.dump(stats, f)
        return stats

    def _report_words(self):
        """what the report line calls the loop, and a note on its personalise timer"""
        return "test", ""

    def _report_test(self, stats, prefetch):
        a = self.args
        name, note = self._report_words()
        if prefetch is not None:
            name = "%s (%s)" % (name, stats["data_root"])
            print("%s: frames stored at %s, extractor ran at %dx%d%s"
                  % (name, ", ".join("%dx%d" % tuple(hw) for hw in stats["stored_frame_size"]) or "-", a.frame_size, a.frame_size,
                     " (resized on the GPU, %s)" % a.resample if stats["resample"] else ""))
            if stats["index"]["dropped"] is not None:
                kept, dropped = stats["index"]["kept"], stats["index"]["dropped"]
                print("%s: context frames filtered by %s, target frames by %s: kept %d users, %d objects, %d + %d videos, "
                      "%d + %d frames; dropped %d users, %d objects, %d + %d videos, %d + %d frames"
                      % (name, stats["filter_context"] or "-", stats["filter_target"] or "-",
                         *(d[k] for d in (kept, dropped) for k in ("users", "objects", "context_videos", "target_videos",
                                                                   "context_frames", "target_frames"))))
            if a.decode == "device":
                print("%s: JPEG decode on the GPU, %d frames; %d decoded by PIL instead (out of scope or damaged)"
                      % (name, prefetch.device_frames, prefetch.fallback_frames))
        print("%s: frame_acc %.2f (%.2f) %% | time to personalise %.2f (%.2f) ms%s | inference %.4f (%.4f) ms/frame | %d tasks%s"
              % (name, 100 * _shown(stats["frame_acc"])[0], 100 * stats["frame_acc"][1], *_shown(stats["personalise_ms"]),
                 note, *_shown(stats["inference_ms_per_frame"]), stats["num_tasks"],
                 " on %d GPU(s)" % self.world if prefetch is None else ", %d target frames in %.1f s incl. JPEG decode (%d threads)"
                 % (stats["target_frames"], stats["wall_s"], a.num_workers)))
        print(OrbitMetrics.line(stats["orbit_metrics"]))


class MultiStepLearner(Learner):
    """Counterpart of the reference's multi-step-learner.py (FineTuner, test only): per task a fresh copy of the model is
    personalised by `personalize_num_grad_steps` optimizer steps on the context set, then evaluated per target video
    (multi-step-learner.py:132-196). The evaluation loop is the learner's, with the finetuner's two steps swapped in."""
    strict_load = False

    def new_recogniser(self):
        a = self.args
        return MultiStepFewShotRecogniser(a.feature_extractor, a.adapt_features, a.classifier, a.clip_length, a.batch_size,
                                          a.learn_extractor, a.logit_scale)

    def init_model(self):
        super().init_model()
        self.base_state = {k: v.clone() for k, v in self.model.state_dict().items()}

    def run(self):
        return {"test": self.test()}

    def learning_args(self):
        a = self.args
        return {"num_grad_steps": a.personalize_num_grad_steps, "learning_rate": a.personalize_learning_rate,
                "extractor_lr_scale": a.personalize_extractor_lr_scale, "loss_fn": cross_entropy,
                "optimizer": a.personalize_optimizer, "momentum": a.personalize_momentum,
                "weight_decay": a.personalize_weight_decay, "betas": tuple(a.personalize_betas),
                "epsilon": a.personalize_epsilon, "native_optimizer": bool(a.native_optimizer)}

    def _personalise(self, context_clips, context_labels):
        # every task starts from the initial parameters (multi-step-learner.py:153-154); the gradient steps need autograd
        # inside the loop's no_grad
        self.model.load_state_dict(self.base_state, strict=False)
        with torch.enable_grad():
            self.model.personalise(context_clips, context_labels, self.learning_args())

    def _predict_video(self, frames):
        return self.model.predict(attach_frame_history(frames, self.args.clip_length))

    def _report_words(self):
        return "finetuner test", " (%d steps)" % self.args.personalize_num_grad_steps

def build_multistep_parser():
    p = build_parser()
    p.set_defaults(classifier="linear", mode="test")
    p.add_argument("--personalize_num_grad_steps", type=int, default=50)
    p.add_argument("--personalize_learning_rate", type=float, default=0.001)
    p.add_argument("--personalize_optimizer", default="adam", choices=["sgd", "adam"])
    p.add_argument("--personalize_weight_decay", type=float, default=0.0)
    p.add_argument("--personalize_extractor_lr_scale", type=float, default=1.0)
    p.add_argument("--personalize_epsilon", type=float, default=1e-8)
    p.add_argument("--personalize_betas", type=float, nargs=2, default=(0.9, 0.999))
    p.add_argument("--personalize_momentum", type=float, default=0.0)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    return Learner(args).run()


def main_multistep(argv=None):
    args = build_multistep_parser().parse_args(argv)
    return MultiStepLearner(args).run()


if __name__ == "__main__":
    main()
