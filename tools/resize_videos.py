"""The reference's data-preparation pass (scripts/resize_videos.py: every frame of the ORBIT tree opened with PIL, resized to
--size with LANCZOS and saved at quality 95, on --nthreads host threads) with decode, resize and encode on the device: the
threads only read, parse and write files. The tree under --data_path is mirrored under --save_path, file names kept; with the
default flags every output file equals, byte for byte, what the reference's script writes with the installed Pillow (a
source's COM segment is carried over as Pillow does; a frame already at --size is re-encoded as the reference does).
Only .jpg / .jpeg files are taken. --restart_rows N writes a restart marker every N MCU rows (Pillow's restart_marker_rows).
Usage (GPU box): python tools/resize_videos.py --data_path RAW --save_path OUT [--size 224] [--nthreads 12] [--quality 95]
                 [--resample lanczos] [--restart_rows 0] [--batch 200]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_path", required=True, type=str, help="Path to ORBIT benchmark dataset root saved by modes")
    p.add_argument("--save_path", required=True, type=str, help="Path to save resized dataset")
    p.add_argument("--size", type=int, default=224, help="Target image size.")
    p.add_argument("--nthreads", type=int, default=12, help="Number of threads that read, parse and write files.")
    p.add_argument("--quality", type=int, default=95)
    p.add_argument("--resample", default="lanczos", choices=("lanczos", "bicubic", "bilinear"))
    p.add_argument("--restart_rows", type=int, default=0, help="MCU rows per restart interval, 0 = no restart markers")
    p.add_argument("--batch", type=int, default=200, help="frames per launch")
    a = p.parse_args(argv)
    import orbit_dataset_amd  # noqa: F401
    from orbit_dataset_amd.data.encode import resize_tree
    r = resize_tree(a.data_path, a.save_path, size=a.size, nthreads=a.nthreads, quality=a.quality, resample=a.resample,
                    restart_rows=a.restart_rows, batch=a.batch)
    print("resized videos saved to %s" % a.save_path)
    print("frames %d  seconds %.2f  frames/s %.1f  host-decoded %d" % (r["frames"], r["seconds"], r["frames_per_s"], r["host_decoded"]))
    print(json.dumps(r))
    return r


if __name__ == "__main__":
    main()
