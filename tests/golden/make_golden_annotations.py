"""Generate fixture G16: what the REFERENCE's data/datasets.py returns with frame annotations loaded and annotation filters on.

Run once where the reference is mounted (it never travels):

    python tests/golden/make_golden_annotations.py [/root/reference]

The reference's `data.datasets` is imported as it is, exactly as make_golden.py:g14_datasets does it - torchvision is absent
offline, so the two transforms data/datasets.py:429-430 calls are stubbed with their documented arithmetic - and its
`utils.args.expand_issues` expands no_issues / mixed_issues. The tree and the cases are tests/annotation_cases.py's. Stored:
the JPEG tree (blob + offsets), the annotation JSONs as strings, the expanded filters, and per case the reference's index
(users, object count, videos in id order with the file numbers they keep) and two passes of `__getitem__` over all users under
one `random.seed` - paths, labels and annotation tensors. Only data is stored - no reference source.
"""
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import orbit_dataset_amd  # noqa: E402,F401
import annotation_cases as ac  # noqa: E402


def stub_torchvision():
    tvf = types.ModuleType("torchvision.transforms.functional")

    def to_tensor(pic):
        a = torch.from_numpy(np.asarray(pic.convert("RGB") if pic.mode != "RGB" else pic).copy())
        return a.permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def normalize(t, mean, std):
        mean = torch.as_tensor(mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(std, dtype=t.dtype).view(-1, 1, 1)
        return t.clone().sub_(mean).div_(std)

    tvf.to_tensor, tvf.normalize = to_tensor, normalize
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})


def main():
    stub_torchvision()
    from data.datasets import UserEpisodicORBITDataset  # the REFERENCE's modules
    from utils.args import expand_issues

    tmp = tempfile.mkdtemp(prefix="g16_")
    root = os.path.join(tmp, "test")
    files = ac.write_tree(root)
    blob, offsets = [], [0]
    for rel in files:
        with open(os.path.join(root, rel), "rb") as f:
            b = f.read()
        blob.append(np.frombuffer(b, dtype=np.uint8))
        offsets.append(offsets[-1] + len(b))
    ann_dir = os.path.join(tmp, "annotations", "test")
    videos = sorted(n[:-5] for n in os.listdir(ann_dir))
    out = {"tree_files": np.array(files), "tree_blob": np.concatenate(blob), "tree_offsets": np.array(offsets, dtype=np.int64),
           "annotation_videos": np.array(videos),
           "annotation_json": np.array([open(os.path.join(ann_dir, v + ".json")).read() for v in videos])}
    file_no = {f: i for i, f in enumerate(files)}

    def rel(paths):  # frame paths -> row numbers of tree_files
        a = np.asarray(paths)
        return np.array([file_no[os.path.relpath(p, root)] for p in a.reshape(-1)], dtype=np.int32).reshape(a.shape)

    for name, kw in ac.CASES.items():
        filters = (expand_issues(kw["filter_context"]), expand_issues(kw["filter_target"]))
        ds = UserEpisodicORBITDataset(root, kw["way_method"], kw["object_cap"], kw["shot_methods"], kw["shots"], kw["video_types"],
                                      kw["subsample_factor"], kw["clip_methods"], kw["clip_length"], 16, "imagenet", kw["load"],
                                      filters, kw["test_mode"], False, kw["with_caps"], None)
        out[name + "_filter_context"], out[name + "_filter_target"] = np.array(filters[0], dtype=str), np.array(filters[1], dtype=str)
        out[name + "_annotations_to_load"] = np.array(ds.annotations_to_load, dtype=str)
        by_id = sorted(ds.video2id.items(), key=lambda kv: kv[1])
        out[name + "_users"] = np.array(ds.users)
        out[name + "_num_objects"] = np.array(ds.num_objects)
        out[name + "_video_ids"] = np.array([os.path.relpath(p, root) for p, _ in by_id])
        kept = [rel(ds.vid2frames[p]) for p, _ in by_id]
        out[name + "_video_files"] = np.concatenate(kept)
        out[name + "_video_file_offsets"] = np.cumsum([0] + [len(k) for k in kept]).astype(np.int64)
        random.seed(ac.SEED + len(name))
        for rep in range(2):  # two passes: the module-level random stream runs on (with_caps state persists)
            for idx in range(len(ds)):
                t = ds[idx]
                key = "%s_r%d_i%d" % (name, rep, idx)
                out[key + "_objects"] = np.array(t["object_list"])
                out[key + "_context_paths"] = rel(t["context_paths"])
                out[key + "_context_labels"] = t["context_labels"]
                assert sorted(t["context_annotations"]) == ds.annotations_to_load
                for a, v in t["context_annotations"].items():
                    out[key + "_context_ann_" + a] = v
                if kw["test_mode"]:
                    out[key + "_target_videos"] = np.array(len(t["target_paths"]))
                    for v, (pa, la, an) in enumerate(zip(t["target_paths"], t["target_labels"], t["target_annotations"])):
                        out[key + "_target%d_paths" % v] = rel(pa)
                        out[key + "_target%d_label" % v] = la
                        assert (an is None) == (not kw["load"])
                        for a, x in (an or {}).items():
                            out[key + "_target%d_ann_%s" % (v, a)] = x
                else:
                    out[key + "_target_paths"] = rel(t["target_paths"])
                    out[key + "_target_labels"] = t["target_labels"]
                    for a, v in t["target_annotations"].items():
                        out[key + "_target_ann_" + a] = v
    out["case_names"] = np.array(list(ac.CASES))
    shutil.rmtree(tmp)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "G16_annotations.npz")
    np.savez_compressed(path, **out)
    g = np.load(path)
    ac.fixture_conditions(g)
    limit = os.path.getsize(os.path.join(HERE, "G14_datasets.npz"))
    assert os.path.getsize(path) <= limit, (os.path.getsize(path), limit)
    print("G16_annotations %.1f KB (limit %.1f KB), %d arrays" % (os.path.getsize(path) / 1024, limit / 1024, len(out)))


if __name__ == "__main__":
    main()
