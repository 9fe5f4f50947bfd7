#!/usr/bin/env python3
"""Standing check for a "no kernel changed" claim: compare the gfx950 device assembly of two checkouts, file by file.

Usage: python tools/device_asm_diff.py PARENT_TREE THIS_TREE

The file list, the compiler and the flags come from THIS_TREE's orbit-dataset_amd/build.py (SOURCES, HIPCC, FLAGS). Every
source is compiled in both trees with `--cuda-device-only -S`, from the tree's own csrc directory and by its relative name,
so that file names inside the assembly are the same on both sides (`-fuse-cuid=none` drops the compilation-unit id symbol, a
hash of the source's absolute path that is no device code). One line per file: `same`, `reordered`, `DIFFERENT` or `new`
(absent from PARENT_TREE; a new file must define no kernel to count as unchanged device code).
A file whose assembly differs as a whole is compared function by function: the text is split at the function symbols (body,
resource `.set`s and kernel descriptor of each mangled name, local label numbers dropped). `reordered` means every function is
there with an identical body, only their order in the file changed; otherwise the added, removed and changed functions are
listed. Exit status 1 on any added, removed or changed function, on a new file that holds an .amdhsa_kernel, or on a parent
source the list no longer names. No GPU needed.
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    spec = importlib.util.spec_from_file_location("orbit_build_asm", os.path.join(tree, "orbit-dataset_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(build, tree, name, out):
    csrc = os.path.join(tree, "orbit-dataset_amd", "csrc")
    flags = list(build.FLAGS)
    flags[flags.index(build.INCLUDE)] = os.path.join(tree, "include")
    r = subprocess.run([build.HIPCC] + flags + ["--cuda-device-only", "-S", "-fuse-cuid=none", name, "-o", out], cwd=csrc,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s in %s:\n%s" % (name, tree, r.stderr))
    with open(out) as f:
        return f.read().splitlines()


def functions(lines):
    """{mangled name: its lines}: from `Begin function` to `End function`, the name's `.set` lines and its .amdhsa_kernel block.
    The <n> of .LBB<n>_, BB<n>_ (loop comments) and .Lfunc_end<n> is the function's position in the file and is dropped."""
    out, cur = {}, None
    for line in lines:
        m = re.search(r"; -- Begin function (\S+)", line) or re.match(r"\t\.amdhsa_kernel (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is None:
            m = re.match(r"\t\.set (\S+)\.\w+, ", line)
            if m and m.group(1) in out:
                out[m.group(1)].append(line)
        if cur is not None:
            # (the padding before a label's `;` comment depends on how many digits <n> had: dropped with it)
            cur.append(re.sub(r"\s+;", " ;", re.sub(r"\b(BB|LBB|Lfunc_begin|Lfunc_end)\d+", r"\1", line)))
            if "; -- End function" in line or ".end_amdhsa_kernel" in line:
                cur = None
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    parent, this = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    build = load_build(this)
    tmp = tempfile.mkdtemp(prefix="device_asm_diff_")

    def one(name):
        new = device_asm(build, this, name, os.path.join(tmp, name + ".this.s"))
        if not os.path.exists(os.path.join(parent, "orbit-dataset_amd", "csrc", name)):
            kernels = sum(1 for line in new if ".amdhsa_kernel" in line)
            return name, "new, %d kernels" % kernels, kernels != 0, []
        old = device_asm(build, parent, name, os.path.join(tmp, name + ".parent.s"))
        if old == new:
            return name, "same (%d lines)" % len(new), False, []
        fo, fn = functions(old), functions(new)
        detail = ["removed " + k for k in fo if k not in fn] + ["added   " + k for k in fn if k not in fo]
        detail += ["changed " + k for k in fo if k in fn and fo[k] != fn[k]]
        if not detail:
            return name, "reordered (%d functions, every body identical)" % len(fn), False, []
        return name, "DIFFERENT (%d of %d functions identical)" % (sum(1 for k in fo if fn.get(k) == fo[k]), len(fo)), True, detail

    bad = False
    with ThreadPoolExecutor(max_workers=8) as ex:
        for name, verdict, failed, detail in ex.map(one, build.SOURCES):
            print("%-22s %s" % (name, verdict))
            for line in detail:
                print("    " + line)
            bad |= failed
    for name in load_build(parent).SOURCES:
        if name not in build.SOURCES:
            print("%-22s MISSING from this tree's SOURCES" % name)
            bad = True
    print("device code %s" % ("DIFFERS" if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
