"""Counterpart of the reference's utils/eval_metrics.py: Evaluator, TrainEvaluator, TestEvaluator, ValidationEvaluator with
the reference's constructor arguments, method names and return shapes, so its learners bind by import swap.

All three ORBIT metrics (frame accuracy, frames-to-recognition, video accuracy; utils/eval_metrics.py:27-69) are functions
of the per-frame argmax alone. The reference copies every video's softmax to the host and re-derives the argmax for each
averaging level; here the logits stay on the device, ONE `orbit_video_metrics` launch per task (csrc/eval.hip) reduces them
to four integers-or-rows per video (frames correct, first correct frame, histogram of predictions, and the predictions
themselves for `save()`), one device-to-host copy brings those over, and every statistic of every averaging level is
computed from the stored integers.

Deviations:
  * `with_ops_counter=True` raises NotImplementedError: the MACs counter (thop) is not built. `get_mean_ops_counter_stats`
    returns the reference's no-counter strings.
  * `video_acc` at task and user level: the reference compares a scalar with a per-frame label ARRAY there
    (`1.0 if most_freq_prediction == label`, :46, called from :190 and :200) and raises for more than one frame. No
    definition is invented: `get_mean_stats` raises ValueError when `video_acc` is among the requested statistics, and
    `get_video_and_object_stats()` reports it at the two levels where the reference defines it.
  * `append_video` also takes one label PER FRAME (the synthetic tasks of learner.py cut their query frames into "videos" that
    mix objects): see its docstring. ORBIT videos, with their one label, are unaffected.
  * a task without videos (a `next_task()` that nothing followed) is skipped by the statistics; the reference fails on it.
"""
import json
from pathlib import Path

import numpy as np
import torch

from .. import _lib

STATS = ("frame_acc", "frames_to_recognition", "video_acc")
_VIDEO_ACC_ERROR = ("video_acc is defined per video and per object only: at task and user level the reference compares the "
                    "most frequent prediction with a per-frame label array (utils/eval_metrics.py:46 called from :190, :200) and "
                    "raises for more than one frame. Use get_video_and_object_stats()")


def video_metrics(logits, video_offsets, video_labels, want_preds=True):
    """One `orbit_video_metrics` launch on the current stream. logits [M, C] float32 on the device, video_offsets [V+1] and
    video_labels [V] host sequences. Returns (out, V, C): `out` is ONE int32 device tensor laid out as
    [correct V | first_correct V | hist V*C | preds M], so that a single copy brings every result to the host."""
    _lib.require_gpu()
    M, C = int(logits.shape[0]), int(logits.shape[1])
    V = len(video_labels)
    dev = logits.device
    offsets = torch.tensor(list(video_offsets), dtype=torch.int32).to(dev, non_blocking=True)
    labels = torch.tensor(list(video_labels), dtype=torch.int64).to(dev, non_blocking=True)
    out = torch.empty(2 * V + V * C + (M if want_preds else 0), dtype=torch.int32, device=dev)
    base = out.data_ptr()
    ptr = lambda first: _lib.c_void_p(base + 4 * first)  # noqa: E731
    _lib.check(_lib.load().orbit_video_metrics(
        _lib.dptr(logits, torch.float32), M, C, _lib.dptr(offsets), _lib.dptr(labels), V,
        ptr(2 * V + V * C) if want_preds else _lib.c_void_p(0), ptr(0), ptr(V), ptr(2 * V), _lib.stream_handle()),
        "orbit_video_metrics")
    return out, V, C


def split_video_metrics(host, V, C, M=None):
    """(correct [V], first_correct [V], hist [V, C], preds [M] or None) views of video_metrics' buffer after its copy to the host"""
    host = np.asarray(host)
    preds = host[2 * V + V * C:] if M is not None else None
    return host[:V], host[V:2 * V], host[2 * V:2 * V + V * C].reshape(V, C), preds


class Segment:
    """The integers a run of frames with ONE label contributes to every statistic: a whole ORBIT video, or one label run of a
    video that was appended with per-frame labels."""
    __slots__ = ("label", "n", "correct", "first_correct", "hist")

    def __init__(self, label, n, correct, first_correct, hist):
        self.label, self.n, self.correct, self.first_correct = int(label), int(n), int(correct), int(first_correct)
        self.hist = np.asarray(hist, dtype=np.int64)
        if self.n < 1:
            raise ValueError("a video needs at least one frame")

    def as_tuple(self):
        return self.label, self.n, self.correct, self.first_correct, self.hist.tolist()


class VideoResult:
    """One appended video: its segments in frame order (one, for a video with a video label), predictions and frame paths."""
    __slots__ = ("segments", "preds", "paths")

    def __init__(self, segments, preds=None, paths=None):
        self.segments = [s if isinstance(s, Segment) else Segment(*s) for s in segments]
        self.preds = None if preds is None else np.asarray(preds, dtype=np.int64)
        self.paths = None if paths is None else [str(p) for p in paths]
        if not self.segments:
            raise ValueError("a video needs at least one frame")

    @property
    def label(self):
        """the video's label; None for a video appended with per-frame labels of more than one value"""
        return self.segments[0].label if len(self.segments) == 1 else None

    @property
    def n(self):
        return sum(s.n for s in self.segments)

    @property
    def hist(self):
        return _sum_hist(self.segments)


def _sum_hist(videos):
    width = max(len(v.hist) for v in videos)
    total = np.zeros(width, dtype=np.int64)
    for v in videos:
        total[:len(v.hist)] += v.hist
    return total


def _score(stat, videos, label=None):
    """`stat` of the concatenation of `videos` in order (one video, a task, a user, or - with `label` - an object)."""
    n = sum(v.n for v in videos)
    if stat == "frame_acc":
        return np.float64(sum(v.correct for v in videos)) / n
    if stat == "frames_to_recognition":
        seen = 0
        for v in videos:
            if v.first_correct < v.n:
                return np.int64(seen + v.first_correct) / n
            seen += v.n
        return 1.0
    if stat == "video_acc":  # np.bincount(predictions).argmax(): the lowest-index maximum of the histogram
        return 1.0 if int(np.argmax(_sum_hist(videos))) == label else 0.0
    raise KeyError(stat)


class Evaluator:
    def __init__(self, stats_to_compute):
        self.stats_to_compute = stats_to_compute
        self.stat_fns = {"frame_acc": self.get_frame_accuracy, "frames_to_recognition": self.get_frames_to_recognition,
                         "video_acc": self.get_video_accuracy}

    def get_confidence_interval(self, scores):
        return (1.96 * np.std(scores)) / np.sqrt(len(scores))

    # The four per-clip functions of the reference on host arrays (label, scores [n, C]); the evaluators below do not go
    # through them - they read the kernel's integers - but callers of the reference's public names keep working.
    def get_frame_accuracy(self, label, probs):
        return np.mean(np.equal(label, np.argmax(probs, axis=-1)).astype(int))

    def get_video_accuracy(self, label, probs):
        return 1.0 if self.get_video_prediction(probs) == label else 0.0

    def get_frames_to_recognition(self, label, probs):
        predictions = np.argmax(probs, axis=-1)
        hits = np.where(label == predictions)[0]
        return hits[0] / len(predictions) if len(hits) > 0 else 1.0

    def get_video_prediction(self, probs):
        return np.bincount(np.argmax(probs, axis=-1)).argmax()


class TrainEvaluator(Evaluator):
    """`update_stats(logits, labels)` takes one label PER FRAME. Device logits only (the native path has no CPU fallback): the
    frames are cut into the runs of equal consecutive labels, each run is one "video" of ONE `orbit_video_metrics` launch, and
    the statistics of the whole clip set are the task-level rule over those runs. `video_acc` follows the reference: defined
    for a single frame only."""

    def __init__(self, stats_to_compute):
        super().__init__(stats_to_compute)
        self.reset()

    def reset(self):
        self.current_stats = {stat: 0.0 for stat in self.stats_to_compute}
        self.running_stats = {stat: [] for stat in self.stats_to_compute}

    def update_stats(self, logits, labels):
        labels = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        logits = logits.detach()
        if logits.shape[0] != len(labels) or len(labels) == 0:
            raise ValueError("update_stats: %d rows of logits for %d labels" % (logits.shape[0], len(labels)))
        cuts = [0] + [i for i in range(1, len(labels)) if labels[i] != labels[i - 1]] + [len(labels)]
        out, V, C = video_metrics(logits.float().contiguous(), cuts, labels[cuts[:-1]], want_preds=False)
        correct, first, hist, _ = split_video_metrics(out.cpu().numpy(), V, C)
        runs = [Segment(labels[cuts[v]], cuts[v + 1] - cuts[v], correct[v], first[v], hist[v]) for v in range(V)]
        for stat in self.stats_to_compute:
            if stat == "video_acc":
                if len(labels) > 1:
                    raise ValueError(_VIDEO_ACC_ERROR)
                score = _score(stat, runs, int(labels[0]))
            else:
                score = _score(stat, runs)
            self.current_stats[stat] = score
            self.running_stats[stat].append(score)

    def get_current_stats(self):
        return self.current_stats

    def get_mean_stats(self):
        return {stat: [np.mean(scores), self.get_confidence_interval(scores)] for stat, scores in self.running_stats.items()}


class TestEvaluator(Evaluator):
    __test__ = False  # (not a pytest class)

    def __init__(self, stats_to_compute, save_dir=None, with_ops_counter=False, count_backwards=False):
        super().__init__(stats_to_compute)
        unknown = [s for s in stats_to_compute if s not in STATS]
        if unknown:
            raise KeyError("unknown statistics %s (known: %s)" % (unknown, list(STATS)))
        if save_dir:
            self.save_dir = save_dir
        if with_ops_counter:
            raise NotImplementedError("with_ops_counter=True: the MACs counter of the reference (thop) is not built, see DESIGN.md "
                                      "section 8; construct the evaluator with with_ops_counter=False")
        self.ops_counter = None
        self.reset()

    def reset(self):
        self.current_user = 0
        self.current_task = 0
        self.all_video_results = [[[]]]  # [user][task] -> [VideoResult]
        self.all_users = []
        self.all_object_lists = [[[]]]
        self.all_personalise_times = [[[]]]
        self.all_inference_times = [[[]]]
        self._pending = []  # the current task's videos, logits still on the device: (logits [n, C], label, paths)

    # ---- collecting -------------------------------------------------------------------------------------------------
    def append_video(self, frame_logits, video_label, frame_paths=None):
        """frame_logits [n, C] on the device (kept there until the task is flushed), video_label the video's logit column.
        Beyond the reference: video_label may hold one label PER FRAME (the synthetic tasks' "videos" mix objects; the
        reference's frame statistics take label arrays too, :35, :56). Such a video is cut into its runs of equal labels; its
        frame statistics are those of the runs' concatenation, every run joins its own object, and the video has no video
        accuracy (it has no video label)."""
        if frame_logits.dim() != 2 or frame_logits.shape[0] == 0:
            raise ValueError("append_video: an empty video (logits of shape %s)" % (tuple(frame_logits.shape),))
        if not frame_logits.is_cuda:
            raise _lib.OrbitHipError("append_video: expected device logits, got a %s tensor (no CPU fallback; integers computed "
                                     "elsewhere go through append_video_integers)" % frame_logits.device)
        frame_logits = frame_logits.detach()
        raw_frames, keep = frame_logits.shape[0], None
        if frame_paths is not None:
            # duplicate frames added by padding to a multiple of clip_length are dropped, keeping the FIRST occurrence in frame
            # order. The reference takes np.unique(frame_paths, return_index=True) (:263-264), which keeps first occurrences too
            # but returns them in SORTED path order: the same frames in the same order wherever the paths arrive sorted, as the
            # dataset yields them.
            frame_paths = [str(p) for p in np.asarray(frame_paths, dtype=object).reshape(-1)]
            if len(frame_paths) != frame_logits.shape[0]:
                raise ValueError("append_video: %d paths for %d frames" % (len(frame_paths), frame_logits.shape[0]))
            seen, keep = set(), []
            for i, p in enumerate(frame_paths):
                if p not in seen:
                    seen.add(p)
                    keep.append(i)
            if len(keep) < len(frame_paths):
                frame_logits = frame_logits[torch.tensor(keep, device=frame_logits.device)]
                frame_paths = [frame_paths[i] for i in keep]
        labels = np.asarray(video_label.detach().cpu() if isinstance(video_label, torch.Tensor) else video_label).reshape(-1)
        if len(labels) == 1:
            runs = [(int(labels[0]), frame_logits.shape[0])]
        elif len(labels) == raw_frames:
            labels = labels if keep is None else labels[keep]
            cuts = [0] + [i for i in range(1, len(labels)) if labels[i] != labels[i - 1]] + [len(labels)]
            runs = [(int(labels[lo]), hi - lo) for lo, hi in zip(cuts, cuts[1:])]
        else:
            raise ValueError("append_video: %d labels for %d frames (one label, or one per frame)" % (len(labels), raw_frames))
        self._pending.append((frame_logits, runs, frame_paths))

    def append_video_integers(self, video_label, n, correct, first_correct, hist, preds=None, frame_paths=None):
        """A video whose integers were computed elsewhere (a recorded run): what a flush stores."""
        self.append_video_segments([(video_label, n, correct, first_correct, hist)], preds, frame_paths)

    def append_video_segments(self, segments, preds=None, frame_paths=None):
        """... a video as its label runs [(label, n, correct, first_correct, hist)] (another rank's evaluator)"""
        self._flush()
        self.all_video_results[self.current_user][self.current_task].append(VideoResult(segments, preds, frame_paths))

    def _flush(self):
        """The current task's pending videos: one launch, one device-to-host copy of the integer outputs."""
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        C = pending[0][0].shape[1]
        if any(lg.shape[1] != C for lg, _, _ in pending):
            raise ValueError("the videos of one task must share the number of classes")
        logits = torch.cat([lg for lg, _, _ in pending]).float().contiguous()
        runs = [run for _, video_runs, _ in pending for run in video_runs]  # the launch's "videos": every label run
        offsets = np.concatenate([[0], np.cumsum([n for _, n in runs])])
        out, V, C = video_metrics(logits, offsets, [label for label, _ in runs], want_preds=True)
        correct, first, hist, preds = split_video_metrics(out.cpu().numpy(), V, C, M=int(offsets[-1]))
        store = self.all_video_results[self.current_user][self.current_task]
        v = 0
        for _, video_runs, paths in pending:
            lo, k = int(offsets[v]), len(video_runs)
            segments = [Segment(label, n, correct[v + i], first[v + i], hist[v + i]) for i, (label, n) in enumerate(video_runs)]
            store.append(VideoResult(segments, preds[lo:int(offsets[v + k])], paths))
            v += k

    def set_current_user(self, user_id):
        self.all_users.append(user_id)
        assert len(self.all_users) == self.current_user + 1

    def set_task_object_list(self, task_object_list):
        self.all_object_lists[self.current_user][self.current_task] = task_object_list

    def next_user(self):
        self._flush()
        for per_user in (self.all_video_results, self.all_object_lists, self.all_personalise_times, self.all_inference_times):
            per_user.append([[]])
        self.current_task = 0
        self.current_user += 1

    def next_task(self):
        self._flush()
        for per_user in (self.all_video_results, self.all_object_lists, self.all_personalise_times, self.all_inference_times):
            per_user[self.current_user].append([])
        self.current_task += 1

    def set_base_params(self, params):
        pass  # (ops counter only)

    def task_complete(self):
        pass  # (ops counter only)

    def log_time(self, time, time_type="personalise"):
        if time_type == "personalise":
            self.all_personalise_times[self.current_user][self.current_task] = time
        elif time_type == "inference":
            self.all_inference_times[self.current_user][self.current_task] = time
        else:
            raise ValueError("time_type must be 'personalise' or 'inference' but got %s" % time_type)

    # ---- statistics -------------------------------------------------------------------------------------------------
    def _users(self, current_user):
        self._flush()
        return [self.current_user] if current_user else range(self.current_user + 1)

    def _level_scores(self, stat, current_user):
        """lists of `stat` per user, object, task and video, in the reference's order (:163-201)"""
        user_scores, object_scores, task_scores, video_scores = [], [], [], []
        for user in self._users(current_user):
            by_object, user_videos = {}, []
            for task_videos in self.all_video_results[user]:
                if not task_videos:
                    continue
                task_segments = [s for v in task_videos for s in v.segments]
                for v in task_videos:
                    if stat != "video_acc" or v.label is not None:  # (no video accuracy without a video label)
                        video_scores.append(_score(stat, v.segments, v.label))
                for s in task_segments:
                    by_object.setdefault(s.label, []).append(s)
                if stat != "video_acc":
                    task_scores.append(_score(stat, task_segments))
                user_videos.extend(task_segments)
            for label, videos in by_object.items():
                object_scores.append(_score(stat, videos, label))
            if stat != "video_acc" and user_videos:
                user_scores.append(_score(stat, user_videos))
        return user_scores, object_scores, task_scores, video_scores

    def get_mean_stats(self, current_user=False):
        """(user, object, task, video) dictionaries {stat: [mean, 1.96 std / sqrt(len)]}"""
        if "video_acc" in self.stats_to_compute:
            raise ValueError(_VIDEO_ACC_ERROR)
        levels = [{stat: [] for stat in self.stats_to_compute} for _ in range(4)]
        for stat in self.stats_to_compute:
            for level, scores in zip(levels, self._level_scores(stat, current_user)):
                level[stat] = scores
        return tuple(self.average_over_scores(level) for level in levels)

    def get_video_and_object_stats(self, current_user=False):
        """(video, object) dictionaries {"video_acc": [mean, ci]}: video accuracy at the two levels where the reference defines
        it (not part of the reference's interface; see the module docstring)."""
        _, object_scores, _, video_scores = self._level_scores("video_acc", current_user)
        return tuple({"video_acc": [np.mean(s), self.get_confidence_interval(s)]} if s else {} for s in (video_scores, object_scores))

    def average_over_scores(self, user_stats):
        return {stat: [np.mean(user_stats[stat]), self.get_confidence_interval(user_stats[stat])]
                for stat in self.stats_to_compute}

    def get_mean_ops_counter_stats(self, current_user=False):
        return "0.00B", "0.00B", "0.00B", ""

    def get_mean_times(self, current_user=False):
        users = self._users(current_user)
        personalise = [np.mean(self.all_personalise_times[u]) for u in users]
        inference = [np.mean(self.all_inference_times[u]) for u in users]
        return (_minutes(np.mean(personalise)), _minutes(np.std(personalise)),
                _microseconds(np.mean(inference)), _microseconds(np.std(inference)))

    def check_for_uncounted_modules(self, model):
        return "TestEvaluator has no ops_counter: MACs are not counted (DESIGN.md section 8)."

    # ---- results.json -----------------------------------------------------------------------------------------------
    def results_dict(self):
        """user -> [ {task_object_list, task_videos: {video_id: {frame_id: prediction}}} ], the structure the reference writes
        (:112-148): video_id is the frame's directory name, frame_id the integer after the last '-' of the file stem."""
        self._flush()
        assert len(self.all_users) == self.current_user + 1
        output = {}
        for user in range(self.current_user + 1):
            output[self.all_users[user]] = []
            for task, task_videos in enumerate(self.all_video_results[user]):
                task_output = {"task_object_list": self.all_object_lists[user][task], "task_videos": {}}
                for v in task_videos:
                    if v.paths is None or v.preds is None:
                        raise ValueError("save() needs the frame paths and predictions of every video")
                    assert len(v.paths) == len(v.preds)
                    frames = task_output["task_videos"][Path(v.paths[0]).parts[-2]] = {}
                    for path, pred in zip(v.paths, v.preds):
                        frames[int(Path(path).stem.split("-")[-1])] = int(pred)
                output[self.all_users[user]].append(task_output)
        return output

    def save(self):
        output = self.results_dict()
        self.json_results_path = Path(self.save_dir, "results.json")
        self.json_results_path.parent.mkdir(exist_ok=True, parents=True)
        with open(self.json_results_path, "w") as json_file:
            json.dump(output, json_file)


class ValidationEvaluator(TestEvaluator):
    def __init__(self, stats_to_compute):
        super().__init__(stats_to_compute)
        self.comparison_stat = self.stats_to_compute[0]  # the first statistic validates the model
        self.current_best_stats = {stat: [0.0, 0.0] for stat in self.stats_to_compute}

    def is_better(self, stats):
        return bool(stats[self.comparison_stat][0] > self.current_best_stats[self.comparison_stat][0])

    def replace(self, stats):
        self.current_best_stats = stats

    def get_current_best_stats(self):
        return self.current_best_stats


def _minutes(seconds):
    mins, secs = (round(x) for x in divmod(seconds, 60))
    return "%.2fs" % seconds if mins == 0 and secs == 0 else "%dm%ds" % (mins, secs)


def _microseconds(seconds):
    return "%dμs" % round(seconds * 1e6)
