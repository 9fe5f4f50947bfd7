"""Dataset-side input pipeline of the episodic path: JPEG directory -> decoded 8-bit frames -> pinned ring buffer ->
8-bit upload on a copy stream -> to_tensor + normalize on the GPU, double-buffered against the extractor.

What the reference does per task: `data/datasets.py:139-200` walks `root/<user>/<object>/<clean|clutter>/
<video>/*.jpg`, `:376-431` opens every frame with PIL, applies `to_tensor` + `normalize` on the host and returns fp32 clips
(602 KB per 224x224 frame); `data/queues.py:44,52-53` wraps that in a `DataLoader(pin_memory=False, num_workers=4/8)`, and
the recogniser moves each mini-batch to the device on the compute stream (`model/few_shot_recognisers.py:112,142`). Here:

  ORBITDirectory      the same directory walk (users -> objects -> clean / clutter -> videos -> sorted frames) and a test-task
                      sampler in the reference's layout (context = the clean videos of each object, target = its clutter
                      videos - or the clean ones left over, `datasets.py:153-161`), returning frame PATHS;
  decode_frames       PIL decode (as `datasets.py:422-431`) of a list of paths into one uint8 [n, H, W, 3] buffer, by a pool
                      of threads (Pillow releases the GIL while it decodes);
  TaskPrefetcher      a staging thread turns host tasks (8-bit frames, from the decoder or any other source) into device tasks:
                      pinned slot <- frames, uint8 H2D on a COPY stream (150 KB per frame instead of 602 KB), then
                      orbit_frames_from_uint8 (the reference transform, bit-identical, csrc/ingest.hip) on that stream into
                      the slot's fp32 clips, and an event the compute stream waits on. `depth` slots rotate, so the upload
                      and the normalisation of task i+1 run while the extractor works on task i. With `frame_size` the
                      frames stored at another size are resized in that launch (orbit_frames_resize_from_uint8: Pillow's
                      8-bit Image.resize, bit-identical - the reference's offline scripts/resize_videos.py pass): the upload
                      stays 8-bit at the stored size, the fp32 clips take the size the extractor runs at.

  JpegFrames          with decode="device" the sources hand over the FILES instead of pixels: the threads read them and parse
                      their headers (orbit_jpeg_parse, host only); the prefetcher uploads the compressed bytes in one copy and
                      orbit_frames_from_jpeg (csrc/jpeg.hip) decodes them on the copy stream into the same 8-bit buffer the
                      launches above read - Pillow's pixels, bit for bit. Files outside the device path's scope (progressive,
                      CMYK ..) and files the device reports damaged are decoded by PIL as before; the count is reported.

`write_synthetic_orbit_directory` builds a small JPEG tree in that layout (the ORBIT dataset itself is not available
offline) and `write_synthetic_orbit_annotations` its frame annotations from explicit per-video rules; they are test / benchmark
scaffolding, not part of the path.
"""
import ctypes
import io
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .utils import NORMALIZE_STATS, output_size, resample_filter


# ---- directory layout (reference data/datasets.py:139-200) -----------------------------------------------------------------
def write_synthetic_orbit_directory(root, users=2, objects_per_user=3, clean_videos=3, clutter_videos=2, frames_per_video=12,
                                    frame_size=224, seed=1991, quality=90):
    """root/<user>/<object>/<clean|clutter>/<video>/<video>-00001.jpg ...: every object has a colour / texture template
    (class signal), every video a smooth drift of it plus noise. Returns the number of frames written."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    n = 0
    for u in range(users):
        for o in range(objects_per_user):
            base = rng.randint(0, 256, size=(8, 8, 3)).astype(np.float32)
            for kind, count in (("clean", clean_videos), ("clutter", clutter_videos)):
                for v in range(count):
                    name = "P%03d--obj%02d--%s--%02d" % (u, o, kind, v)
                    d = os.path.join(root, "P%03d" % u, "obj%02d" % o, kind, name)
                    os.makedirs(d, exist_ok=True)
                    for f in range(frames_per_video):
                        small = np.clip(base + rng.normal(0, 20 if kind == "clean" else 45, base.shape) + 2.0 * f, 0, 255)
                        img = Image.fromarray(small.astype(np.uint8)).resize((frame_size, frame_size), Image.BILINEAR)
                        img.save(os.path.join(d, "%s-%05d.jpg" % (name, f + 1)), quality=quality)
                        n += 1
    return n


def write_synthetic_orbit_annotations(split_root, absent=None, issues=None):
    """The frame annotations of a written split, where the datasets look for them: dirname(split_root)/annotations/<split>/
    <video>.json, one per video, keyed by frame file name, in the two formats of the ORBIT release - a clean video's frames
    carry the seven quality issues (all but object_not_present_issue null where the object is absent), a clutter video's
    frames a bounding box (null where the object is absent) and object_not_present_issue.

    Explicit rules, no random draws: absent = {video name: frame positions (0-based, in sorted frame order) without the
    object}, issues = {clean video name: {issue: frame positions that have it}}; every other value is false. Returns the
    annotation directory."""
    import json
    from .datasets import FRAME_ANNOTATION_OPTIONS
    absent = {k: set(v) for k, v in (absent or {}).items()}
    issues = {k: {i: set(f) for i, f in v.items()} for k, v in (issues or {}).items()}
    split_root = split_root.rstrip(os.sep) or split_root
    out = os.path.join(os.path.dirname(split_root), "annotations", os.path.basename(split_root))
    os.makedirs(out, exist_ok=True)
    seen = set()
    for user in sorted(os.listdir(split_root)):
        for obj in sorted(os.listdir(os.path.join(split_root, user))):
            for kind in ("clean", "clutter"):
                kind_dir = os.path.join(split_root, user, obj, kind)
                for video in sorted(os.listdir(kind_dir)) if os.path.isdir(kind_dir) else ():
                    seen.add(video)
                    if kind == "clutter" and video in issues:
                        raise ValueError("quality issues are annotated on clean videos only, %s is a clutter video" % video)
                    unknown = set(issues.get(video, {})) - set(FRAME_ANNOTATION_OPTIONS[1:])
                    if unknown:
                        raise ValueError("unknown quality issues %s for %s" % (sorted(unknown), video))
                    frames = sorted(f for f in os.listdir(os.path.join(kind_dir, video)) if f.endswith(".jpg"))
                    anns = {}
                    for k, frame in enumerate(frames):
                        gone = k in absent.get(video, ())
                        if kind == "clean":
                            anns[frame] = {"object_not_present_issue": gone}
                            for issue in FRAME_ANNOTATION_OPTIONS[1:]:
                                anns[frame][issue] = None if gone else k in issues.get(video, {}).get(issue, ())
                        else:
                            box = None if gone else {"x": 270 + k % 7, "y": 300 + k % 5, "w": 400, "h": 360}
                            anns[frame] = {"object_bounding_box": box, "object_not_present_issue": gone}
                    with open(os.path.join(out, video + ".json"), "w") as f:
                        json.dump(anns, f)
    unknown = (set(absent) | set(issues)) - seen
    if unknown:
        raise ValueError("rules for videos that are not under %s: %s" % (split_root, sorted(unknown)))
    return out


class ORBITDirectory:
    """The directory walk of reference data/datasets.py:139-200 (no annotation filters): users, their objects, the clean /
    clutter videos of every object and the sorted frame paths of every video."""

    def __init__(self, root, context_type="clean", target_type="clutter", min_context_frames=1, min_target_frames=1):
        self.root = root
        self.users, self.user2objs, self.obj2name, self.obj2vids, self.vid2frames = [], {}, {}, {}, {}
        obj_id = 0
        for user in sorted(os.listdir(root)):
            user_path = os.path.join(root, user)
            if not os.path.isdir(user_path):
                continue
            objs = []
            for obj_name in sorted(os.listdir(user_path)):
                obj_path = os.path.join(user_path, obj_name)
                clean_dir = os.path.join(obj_path, "clean")
                if not os.path.isdir(clean_dir):
                    continue
                clean = sorted(os.listdir(clean_dir))
                if context_type == "clean" and target_type == "clean":
                    split = min(5, len(clean) - 1)  # aim for 5 context videos, leaving at least 1 target video (:157-160)
                    sets = {"context": [("clean", v) for v in clean[:split]], "target": [("clean", v) for v in clean[split:]]}
                else:
                    clutter_dir = os.path.join(obj_path, "clutter")
                    clutter = sorted(os.listdir(clutter_dir)) if os.path.isdir(clutter_dir) else []
                    sets = {"context": [("clean", v) for v in clean], "target": [("clutter", v) for v in clutter]}
                kept = {"context": [], "target": []}
                for set_type, vids in sets.items():
                    need = min_context_frames if set_type == "context" else min_target_frames
                    for kind, v in vids:
                        vp = os.path.join(obj_path, kind, v)
                        frames = sorted(os.path.join(vp, f) for f in os.listdir(vp) if f.endswith(".jpg"))
                        if len(frames) >= need:
                            kept[set_type].append(vp)
                            self.vid2frames[vp] = frames
                if kept["context"] and kept["target"]:  # object is valid (:184-186)
                    objs.append(obj_id)
                    self.obj2name[obj_id] = obj_name
                    self.obj2vids[obj_id] = kept
                    obj_id += 1
            if objs:
                self.users.append(user)
                self.user2objs[user] = objs

    def user_task(self, user, clip_length=1, context_frames_per_video=None, target_frames_per_video=None):
        """One user-episodic task in the reference's task_dict layout (datasets.py:584-597) with PATHS instead of pixels:
        context_paths [N, T] / target_paths [M, T] (clips of T contiguous frames, non-overlapping for the context set, one
        clip ending at every frame - `attach_frame_history` - is the test loop's job for the target set), labels = the
        object's index within the user."""
        ctx, ctx_lab, tgt, tgt_lab, tgt_videos = [], [], [], [], []
        T = int(clip_length)
        for label, obj in enumerate(self.user2objs[user]):
            for vp in self.obj2vids[obj]["context"]:
                frames = self.vid2frames[vp][:context_frames_per_video]
                for i in range(0, len(frames) - T + 1, T):
                    ctx.append(frames[i:i + T])
                    ctx_lab.append(label)
            for vp in self.obj2vids[obj]["target"]:
                frames = self.vid2frames[vp][:target_frames_per_video]
                tgt_videos.append((len(tgt), len(tgt) + len(frames)))
                for f in frames:
                    tgt.append([f])
                    tgt_lab.append(label)
        return {"context_paths": np.array(ctx, dtype=object).reshape(len(ctx), T), "context_labels": torch.tensor(ctx_lab),
                "target_paths": np.array(tgt, dtype=object).reshape(len(tgt), 1), "target_labels": torch.tensor(tgt_lab),
                "target_videos": tgt_videos, "object_list": [self.obj2name[o] for o in self.user2objs[user]]}


def decode_frames(paths, out=None, pool=None):
    """JPEG files -> uint8 [n, H, W, 3] (RGB, as PIL decodes them: the input of to_tensor in datasets.py:428-429)."""
    from PIL import Image
    paths = list(paths)
    if not paths:  # a user without context / target frames: an empty batch, not an IndexError
        return out if out is not None else np.empty((0, 0, 0, 3), dtype=np.uint8)

    def one(i):
        with Image.open(paths[i]) as im:
            a = np.asarray(im.convert("RGB"))
        if out is not None:
            out[i].copy_(torch.from_numpy(a)) if isinstance(out, torch.Tensor) else out.__setitem__(i, a)
        return a

    if out is None:
        first = one(0)
        out = np.empty((len(paths),) + first.shape, dtype=np.uint8)
        out[0] = first
        rest = range(1, len(paths))
    else:
        rest = range(len(paths))
    if pool is None:
        for i in rest:
            one(i)
    else:
        list(pool.map(one, rest))
    return out


# ---- compressed frames for the device decoder -------------------------------------------------------------------------------
JPEG_WORKSPACE_CAP = 1 << 30  # bytes of coefficient + plane workspace per launch; more frames go through it in chunks (a chunk
#                               runs one wave per frame: at 1080 x 1080, 10.6 MB per frame, this is 100 frames at a time)


def _pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))  # (a copy: torch wants a writable array)


class JpegFrames:
    """The frames of a clips tensor [*lead, H, W, 3] as FILES: `files` (one bytes object per frame, row-major over `lead`),
    `descs` (uint8 [n, sizeof(orbit_jpeg_desc_t)], the parsed headers), `codes` (orbit_jpeg_parse's result per frame: 0 =
    the device decodes it) and `pixels` {frame: uint8 [H, W, 3]}: the frames PIL has already decoded because the device
    path does not cover them. All frames are `size` = (H, W)."""

    def __init__(self, files, descs, codes, pixels, lead, size):
        self.files, self.descs, self.codes, self.pixels = files, descs, codes, pixels
        self.lead, self.size = tuple(int(v) for v in lead), (int(size[0]), int(size[1]))
        assert int(np.prod(self.lead)) == len(files) == len(descs) == len(codes)

    @property
    def shape(self):
        return (*self.lead, *self.size, 3)

    def __len__(self):
        return self.lead[0]

    def with_lead(self, *lead):
        return JpegFrames(self.files, self.descs, self.codes, self.pixels, lead, self.size)

    def flatten(self, end_dim=1):
        """as Tensor.flatten(end_dim=k) over the leading dimensions"""
        k = end_dim + 1
        return self.with_lead(int(np.prod(self.lead[:k])), *self.lead[k:])

    def unsqueeze(self, dim):
        lead = list(self.lead)
        lead.insert(dim, 1)
        return self.with_lead(*lead)

    @staticmethod
    def cat(parts):
        """as torch.cat along the first dimension"""
        parts = list(parts)
        sizes = {p.size for p in parts if len(p.files)}
        if len(sizes) > 1:
            raise ValueError("JpegFrames.cat: frames of different sizes %s" % sorted(sizes))
        files, codes, pixels, base = [], [], {}, 0
        for p in parts:
            files += p.files
            codes += list(p.codes)
            pixels.update({base + i: px for i, px in p.pixels.items()})
            base += len(p.files)
        return JpegFrames(files, np.concatenate([p.descs for p in parts]), codes, pixels,
                          (sum(p.lead[0] for p in parts), *parts[0].lead[1:]), sizes.pop() if sizes else parts[0].size)


def read_jpeg_frames(paths, pool=None, lead=None, empty_size=(0, 0)):
    """Files -> JpegFrames: every file is read and its headers parsed (orbit_jpeg_parse releases the GIL: `pool` threads work
    side by side); PIL decodes the files the device path does not cover, and only those."""
    from .. import _lib
    lib = _lib.load()
    paths = list(paths)
    n, size = len(paths), ctypes.sizeof(_lib.JpegDesc)
    descs = np.zeros((n, size), dtype=np.uint8)
    files, codes, pixels = [None] * n, [0] * n, {}

    def one(i):
        with open(paths[i], "rb") as f:
            files[i] = f.read()
        codes[i] = lib.orbit_jpeg_parse(files[i], len(files[i]), descs[i].ctypes.data, size)
        if codes[i] != 0:
            pixels[i] = _pil_rgb(files[i])  # (what PIL raises for a broken file surfaces here, as in decode_frames)

    if pool is None:
        for i in range(n):
            one(i)
    else:
        list(pool.map(one, range(n)))
    hw = empty_size
    if n:
        d = descs.view(np.int32)
        sizes = {(int(d[i, 6]), int(d[i, 5])) if codes[i] == 0 else pixels[i].shape[:2] for i in range(n)}  # (height, width)
        if len(sizes) > 1:
            raise ValueError("read_jpeg_frames: frames of different sizes in one batch: %s" % sorted(sizes))
        hw = sizes.pop()
    return JpegFrames(files, descs, codes, pixels, (n,) if lead is None else lead, hw)


def _jpeg_launch(jf, u8, pinned, dev, device):
    """Upload jf's files and descriptors in one copy and decode them into u8 [n, H, W, 3] on the current stream; the frames PIL
    already decoded are copied into their rows. `pinned` / `dev`: dicts that keep the buffers between calls. Returns the
    pinned status vector (int32 [n]) and the event after which it is valid."""
    from .. import _lib
    lib = _lib.load()
    n, (H, W) = len(jf.files), jf.size
    dsize = ctypes.sizeof(_lib.JpegDesc)
    offsets, at = np.empty(n, dtype=np.uint64), 0
    for i, f in enumerate(jf.files):
        offsets[i] = at
        at += (len(f) + 15) // 16 * 16
    head, total = n * dsize, n * dsize + max(at, 16)

    def grow(store, key, count, make):
        t = store.get(key)
        if t is None or t.numel() < count:
            t = store[key] = make(count)
        return t[:count]

    arena = grow(pinned, "arena", total, lambda c: torch.empty(c, dtype=torch.uint8).pin_memory())
    host = arena.numpy()
    rows = host[:head].reshape(n, dsize)
    rows[:] = jf.descs
    rows.view(np.uint64)[:, 0] = offsets  # file_offset, the descriptor's first field
    for i, f in enumerate(jf.files):
        o = head + int(offsets[i])
        host[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        if jf.codes[i] < 0:
            rows.view(np.int32)[i, 4] = 127  # not a JPEG at all: skipped like any other host-decoded frame
    d_arena = grow(dev, "arena", total, lambda c: torch.empty(c, dtype=torch.uint8, device=device))
    d_arena.copy_(arena, non_blocking=True)
    ws_bytes = min(lib.orbit_jpeg_workspace_bytes(n, H, W), max(JPEG_WORKSPACE_CAP, lib.orbit_jpeg_workspace_bytes(1, H, W)))
    ws = grow(dev, "workspace", ws_bytes, lambda c: torch.empty(c, dtype=torch.uint8, device=device))
    status = grow(dev, "status", n, lambda c: torch.empty(c, dtype=torch.int32, device=device))
    _lib.check(lib.orbit_frames_from_jpeg(ctypes.c_void_p(d_arena.data_ptr() + head), total - head, _lib.dptr(d_arena), n, H, W,
                                          _lib.dptr(u8, torch.uint8), _lib.dptr(status), _lib.dptr(ws), ws_bytes,
                                          _lib.stream_handle()), "orbit_frames_from_jpeg")
    if jf.pixels:
        frames = u8.view(n, H, W, 3)
        px = grow(pinned, "pixels", len(jf.pixels) * H * W * 3, lambda c: torch.empty(c, dtype=torch.uint8).pin_memory())
        px = px.view(len(jf.pixels), H, W, 3)
        for k, (i, a) in enumerate(sorted(jf.pixels.items())):
            px[k].copy_(torch.from_numpy(a))
            frames[i].copy_(px[k], non_blocking=True)
    status_host = grow(pinned, "status", n, lambda c: torch.empty(c, dtype=torch.int32).pin_memory())
    status_host.copy_(status, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    return status_host, done


def decode_frames_device(paths, device, pool=None, stats=None):
    """JPEG files -> uint8 [n, H, W, 3] on `device`, equal to decode_frames(paths): decoded by orbit_frames_from_jpeg, by PIL
    where the device path does not cover a file or reports it damaged. `stats`, a dict, receives the counts."""
    from .. import _lib
    _lib.require_gpu()
    device = torch.device(device)
    jf = read_jpeg_frames(paths, pool)
    n, (H, W) = len(jf.files), jf.size
    with torch.cuda.device(device):
        u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=device)
        bad = []
        if n:
            status, done = _jpeg_launch(jf, u8, {}, {}, device)
            done.synchronize()
            bad = [i for i in range(n) if status[i] > 0]
            for i in bad:
                u8[i].copy_(torch.from_numpy(_pil_rgb(jf.files[i])))
            torch.cuda.current_stream().synchronize()  # the pinned buffers of this call are dropped on return
    if stats is not None:
        stats.update({"frames": n, "fallback_frames": len(jf.pixels) + len(bad), "out_of_scope": len(jf.pixels), "damaged": len(bad),
                      "status": [int(v) for v in status] if n else []})
    return u8


class DirectoryTaskSource:
    """Iterator of host tasks decoded from an ORBITDirectory: {context_clips u8 [N,T,H,W,3], context_labels, target_clips u8
    [M,1,H,W,3], target_labels, target_videos}. `workers` decode threads (the reference: DataLoader workers, queues.py:34).
    decode="device": the clips are JpegFrames (the files, read and parsed by the threads) for the prefetcher to decode."""

    def __init__(self, directory, clip_length=1, workers=8, context_frames_per_video=None, target_frames_per_video=None,
                 users=None, decode="host"):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' or 'device', got %r" % (decode,))
        self.decode = decode
        self.dir, self.T = directory, int(clip_length)
        self.users = list(users if users is not None else directory.users)
        self.cpv, self.tpv = context_frames_per_video, target_frames_per_video
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))

    def __len__(self):
        return len(self.users)

    def __iter__(self):
        for user in self.users:
            t = self.dir.user_task(user, self.T, self.cpv, self.tpv)
            if self.decode == "device":
                yield {"context_clips": read_jpeg_frames(t["context_paths"].reshape(-1), self.pool, (len(t["context_paths"]), self.T)),
                       "context_labels": t["context_labels"],
                       "target_clips": read_jpeg_frames(t["target_paths"].reshape(-1), self.pool, (len(t["target_paths"]), 1)),
                       "target_labels": t["target_labels"], "target_videos": t["target_videos"], "user": user}
                continue
            ctx = decode_frames(t["context_paths"].reshape(-1), pool=self.pool)
            tgt = decode_frames(t["target_paths"].reshape(-1), pool=self.pool)
            yield {"context_clips": torch.from_numpy(ctx).reshape(len(t["context_paths"]), self.T, *ctx.shape[1:]),
                   "context_labels": t["context_labels"],
                   "target_clips": torch.from_numpy(tgt).reshape(len(t["target_paths"]), 1, *tgt.shape[1:]),
                   "target_labels": t["target_labels"], "target_videos": t["target_videos"], "user": user}


class DatasetTaskSource:
    """Host tasks from a data/datasets.py dataset built with frames="uint8" - or frames="jpeg": JpegFrames for the device decoder - (the reference-pinned sampler: way, video and clip
    sampling of reference data/datasets.py:289-336,433-469,540-598), in the layout TaskPrefetcher uploads:
    context_clips u8 [N,T,H,W,3]; a test-mode target set (a list of videos) is concatenated into target_clips u8 [M,1,H,W,3]
    with `target_videos` = [(lo, hi)] row ranges and one label per frame; a train-mode target set passes through as clips.
    Frame annotations ride along as host tensors: `context_annotations` as sampled, `target_annotations` of a test-mode target
    set as ONE dict of [M, 1] tensors in the row order of target_clips ({} when nothing is loaded)."""

    def __init__(self, dataset, indices=None):
        if dataset.frames not in ("uint8", "jpeg"):
            raise ValueError("DatasetTaskSource needs a dataset built with frames='uint8' or frames='jpeg'")
        self.dataset = dataset
        self.indices = list(range(len(dataset)) if indices is None else indices)

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        for i in self.indices:
            t = self.dataset[i]
            out = {"context_clips": t["context_clips"], "context_labels": t["context_labels"], "context_paths": t["context_paths"],
                   "object_list": t["object_list"], "task_id": t["task_id"], "user": t["task_id"],
                   "context_annotations": t["context_annotations"]}
            if isinstance(t["target_clips"], list):
                ranges, lo = [], 0
                for frames in t["target_clips"]:
                    ranges.append((lo, lo + len(frames)))
                    lo += len(frames)
                cat = JpegFrames.cat if self.dataset.frames == "jpeg" else torch.cat
                out["target_clips"] = cat(t["target_clips"]).unsqueeze(1)
                out["target_labels"] = torch.cat([lab.reshape(1).expand(hi - lo) for lab, (lo, hi) in
                                                  zip(t["target_labels"], ranges)]) if ranges else torch.empty(0, dtype=torch.int64)
                out["target_videos"], out["target_paths"] = ranges, t["target_paths"]
                per_video = [a for a in t["target_annotations"] if a is not None]
                out["target_annotations"] = {k: torch.cat([a[k] for a in per_video]) for k in (per_video[0] if per_video else ())}
            else:
                out["target_clips"], out["target_labels"], out["target_paths"] = t["target_clips"], t["target_labels"], t["target_paths"]
                out["target_annotations"] = t["target_annotations"]
            yield out


# ---- pinned ring + copy stream ---------------------------------------------------------------------------------------------
class _Slot:
    def __init__(self):
        self.pinned, self.dev_u8, self.dev_f32, self.dev_lab = {}, {}, {}, {}
        self.ready = None      # recorded on the copy stream when the slot's fp32 clips are complete
        self.released = None   # recorded on the consumer's stream when it is done with the slot
        self.task = None


class TaskPrefetcher:
    """Iterate over `source` (host tasks whose `*_clips` are uint8, channels last [..., H, W, 3] or channels first
    [..., 3, H, W] - or already-normalised float32 [..., 3, H, W], the reference's layout); yields the same dicts with the
    clips replaced by normalised fp32 [..., 3, H, W] tensors RESIDENT on `device`. Every other entry passes through (label
    tensors are moved to the device; the `*_annotations` dicts stay on the host, as the reference's unpack_task leaves them).

    A staging thread fills pinned slot buffers and issues, on a copy stream, the 8-bit upload and the normalisation kernel of
    task i+1 (and i+2 with depth 3) while the caller's stream runs the extractor on task i. The yielded tensors belong to the
    slot: they stay valid until the NEXT task is requested (then the slot is handed back: an event on the caller's stream
    makes the copy stream wait for the kernels that still read it).

    frame_size (an int or (H, W)): uint8 clips stored at another size leave at this one, resized on the device as PIL's
    Image.resize((W, H), resample) would ("lanczos", "bicubic" or "bilinear"); clips already at it, and float32 clips,
    take the path without a resize. Context and target clips may be stored at different sizes.

    Clips may also be JpegFrames (a source with decode="device"): their files are uploaded and decoded on the copy stream
    into the 8-bit buffer, then normalised / resized like uploaded pixels. The staging thread alone waits for the decode's
    status; a frame the device reports damaged is decoded by PIL, uploaded and normalised again - or raises what PIL
    raises. Every yielded task then carries "decode_fallbacks", the number of its frames PIL decoded; `fallback_frames`
    and `device_frames` count over all tasks."""

    def __init__(self, source, device, depth=3, frame_norm_method="imagenet", consumer_streams=(), frame_size=None,
                 resample="lanczos"):
        from .. import _lib
        _lib.require_gpu()
        self._lib = _lib
        self.source, self.device = source, torch.device(device)
        self.mean, self.std = NORMALIZE_STATS[frame_norm_method]
        self.frame_size, self.filter = frame_size, resample_filter(resample)
        self.stored_sizes = set()  # (H, W) of the 8-bit clips staged so far
        self.fallback_frames = self.device_frames = 0  # JpegFrames: frames PIL decoded / frames the device decoded
        self.depth = max(2, int(depth))
        self.slots = [_Slot() for _ in range(self.depth)]
        self.copy_stream = torch.cuda.Stream(device=self.device)
        # further streams on which the consumer reads a slot's tensors (a recogniser in pipelined mode, overlap_query = 2, runs
        # the query pass on its own second stream and does not join it): a slot is only refilled once EVERY such stream has
        # passed the point at which the next task was requested. A callable is evaluated at release time.
        self.consumer_streams = consumer_streams
        self.free, self.full = queue.Queue(), queue.Queue()
        for s in self.slots:
            self.free.put(s)
        self.current = None
        self.error = None
        self.thread = threading.Thread(target=self._stage, name="orbit-task-prefetch", daemon=True)
        self.thread.start()

    @staticmethod
    def _buffer(store, key, shape, make):
        t = store.get(key)
        n = int(np.prod(shape))
        if t is None or t.numel() < n:
            t = store[key] = make(n)
        return t[:n].view(*shape)

    def _normalise(self, u8, f32, hwc, B, H, W, Ho, Wo, first=0, count=None):
        """frames [first, first + count) of u8 [B, H, W, 3] (or [B, 3, H, W]) -> f32 [B, 3, Ho, Wo] on the current stream"""
        lib, f3 = self._lib.load(), ctypes.c_float * 3
        mean, std = f3(*self.mean), f3(*self.std)
        count = B - first if count is None else count
        src = ctypes.c_void_p(self._lib.dptr(u8, torch.uint8).value + first * 3 * H * W)
        dst = ctypes.c_void_p(self._lib.dptr(f32, torch.float32).value + 4 * first * 3 * Ho * Wo)
        if (Ho, Wo) != (H, W):
            self._lib.check(lib.orbit_frames_resize_from_uint8(src, 1 if hwc else 0, count, H, W, Ho, Wo, self.filter, mean, std, dst,
                                                               self._lib.stream_handle()), "orbit_frames_resize_from_uint8")
        else:
            self._lib.check(lib.orbit_frames_from_uint8(src, 1 if hwc else 0, count, H, W, mean, std, dst,
                                                        self._lib.stream_handle()), "orbit_frames_from_uint8")

    def _stage(self):
        try:
            torch.cuda.set_device(self.device)
            lib = self._lib.load()
            f3 = ctypes.c_float * 3
            mean, std = f3(*self.mean), f3(*self.std)
            for task in self.source:
                slot = self.free.get()
                if slot is None:
                    return
                for ev in slot.released or ():
                    self.copy_stream.wait_event(ev)  # the consumer's kernels that read the slot's last task
                out = dict(task)
                pending = []  # device decodes whose status is still to be read
                with torch.cuda.stream(self.copy_stream):
                    for key, val in task.items():
                        if isinstance(val, JpegFrames) and key.endswith("clips"):
                            (H, W), B = val.size, len(val.files)
                            Ho, Wo = output_size(self.frame_size, H, W)
                            u8 = self._buffer(slot.dev_u8, key, val.shape,
                                              lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
                            f32 = self._buffer(slot.dev_f32, key, (*val.lead, 3, Ho, Wo),
                                               lambda n: torch.empty(n, dtype=torch.float32, device=self.device))
                            if B > 0:
                                self.stored_sizes.add((H, W))
                                for ev in slot.released or ():
                                    ev.synchronize()  # (the slot's pinned arena: see the 8-bit path below)
                                status, done = _jpeg_launch(val, u8, slot.pinned.setdefault((key, "jpeg"), {}),
                                                            slot.dev_u8.setdefault((key, "jpeg"), {}), self.device)
                                self._normalise(u8, f32, True, B, H, W, Ho, Wo)
                                pending.append((val, u8, f32, status, done, (B, H, W, Ho, Wo)))
                            out[key] = f32
                            continue
                        if not (isinstance(val, torch.Tensor) and key.endswith("clips")):
                            if isinstance(val, torch.Tensor) and key.endswith("labels"):
                                # labels live in the slot like the clips: the slot's `released` event orders their reuse
                                # after the consumer's kernels (a fresh allocation here would return to the COPY stream's
                                # pool when the consumer drops the task, while compute-stream kernels may still read it)
                                lab = self._buffer(slot.dev_lab, (key, val.dtype), val.shape,
                                                   lambda n, dt=val.dtype: torch.empty(n, dtype=dt, device=self.device))
                                lab.copy_(val, non_blocking=True)
                                out[key] = lab
                            continue
                        if val.dtype == torch.float32:
                            # already-normalised fp32 clips (the reference's own task_dict layout, data/datasets.py:584-597:
                            # 602 KB per 224x224 frame): no transform, but the upload of task i+1 still runs on the copy stream
                            # under the extractor's work on task i instead of in front of it
                            host = val
                            if not val.is_pinned():
                                host = self._buffer(slot.pinned, (key, "f32"), val.shape,
                                                    lambda n: torch.empty(n, dtype=torch.float32).pin_memory())
                                for ev in slot.released or ():
                                    ev.synchronize()
                                host.copy_(val)
                            f32 = self._buffer(slot.dev_f32, key, val.shape,
                                               lambda n: torch.empty(n, dtype=torch.float32, device=self.device))
                            f32.copy_(host, non_blocking=True)
                            out[key] = f32
                            continue
                        if val.dtype != torch.uint8:
                            raise ValueError("TaskPrefetcher: %s must be uint8 or float32 frames, got %s" % (key, val.dtype))
                        hwc = val.shape[-1] == 3 and val.shape[-3] != 3
                        *lead, a, b, c = val.shape
                        H, W = (a, b) if hwc else (b, c)
                        B = int(np.prod(lead)) if lead else 1
                        host = val
                        if not val.is_pinned():
                            host = self._buffer(slot.pinned, key, val.shape,
                                                lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
                            for ev in slot.released or ():
                                ev.synchronize()             # the previous upload from this pinned buffer has long finished;
                            host.copy_(val)                  # (host-side wait only matters if the consumer never advanced)
                        u8 = self._buffer(slot.dev_u8, key, val.shape,
                                          lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
                        Ho, Wo = output_size(self.frame_size, H, W)
                        if B > 0:
                            self.stored_sizes.add((H, W))
                        f32 = self._buffer(slot.dev_f32, key, (*lead, 3, Ho, Wo),
                                           lambda n: torch.empty(n, dtype=torch.float32, device=self.device))
                        u8.copy_(host, non_blocking=True)
                        if B > 0 and (Ho, Wo) != (H, W):
                            self._lib.check(lib.orbit_frames_resize_from_uint8(
                                self._lib.dptr(u8, torch.uint8), 1 if hwc else 0, B, H, W, Ho, Wo, self.filter, mean, std,
                                self._lib.dptr(f32), self._lib.stream_handle()), "orbit_frames_resize_from_uint8")
                        else:
                            self._lib.check(lib.orbit_frames_from_uint8(self._lib.dptr(u8, torch.uint8), 1 if hwc else 0, B, H, W,
                                                                        mean, std, self._lib.dptr(f32), self._lib.stream_handle()),
                                            "orbit_frames_from_uint8")
                        out[key] = f32
                    # The decodes' statuses, read by this thread once everything of the task is queued (the compute stream never
                    # waits for this): a frame the device gave up on is decoded by PIL and takes the same two steps again.
                    fallbacks = 0
                    for val, u8, f32, status, done, (B, H, W, Ho, Wo) in pending:
                        done.synchronize()
                        bad = [i for i in np.nonzero(status.numpy() > 0)[0]]
                        frames = u8.view(B, H, W, 3)
                        for i in bad:
                            a = _pil_rgb(val.files[i])  # raises for a file PIL cannot decode either: surfaces from __next__
                            if a.shape != (H, W, 3):
                                raise ValueError("TaskPrefetcher: a frame of %s among frames of %s" % (a.shape[:2], (H, W)))
                            frames[i].copy_(torch.from_numpy(a))
                            self._normalise(u8, f32, True, B, H, W, Ho, Wo, first=int(i), count=1)
                        fallbacks += len(val.pixels) + len(bad)
                        self.device_frames += B - len(val.pixels) - len(bad)
                    if pending:
                        out["decode_fallbacks"] = fallbacks
                        self.fallback_frames += fallbacks
                    slot.ready = torch.cuda.Event()
                    slot.ready.record(self.copy_stream)
                slot.task = out
                self.full.put(slot)
        except BaseException as e:  # surfaced by the consumer
            self.error = e
        finally:
            self.full.put(None)

    def _release_current(self):
        if self.current is not None:
            extra = self.consumer_streams() if callable(self.consumer_streams) else self.consumer_streams
            events = []
            for st in [torch.cuda.current_stream(self.device)] + [s for s in (extra or ()) if s is not None]:
                ev = torch.cuda.Event()
                ev.record(st)
                events.append(ev)
            self.current.released = events
            self.current.task = None
            self.free.put(self.current)
            self.current = None

    def __iter__(self):
        return self

    def __next__(self):
        self._release_current()
        slot = self.full.get()
        if slot is None:
            if self.error is not None:
                raise self.error
            raise StopIteration
        torch.cuda.current_stream(self.device).wait_event(slot.ready)
        # the clips were produced on the copy stream, complete at `slot.ready`: a recogniser in its default mode may start its
        # query pass from that event instead of behind the support pass (data.utils.mark_ready)
        from .utils import mark_ready
        for key, val in slot.task.items():
            if isinstance(val, torch.Tensor) and key.endswith("clips"):
                mark_ready(val, slot.ready)
        self.current = slot
        return slot.task

    def close(self):
        self._release_current()
        self.free.put(None)
