"""Static instruction counts of the conv_igemm_kernel instantiations, from the compiler's assembly (no GPU needed).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only -o conv_igemm.s orbit-dataset_amd/csrc/conv_igemm.hip
  python tools/conv_isa_counts.py conv_igemm.s [substring of the demangled template arguments ...]

Per kernel: VALU (v_* without MFMA and transcendentals), transcendentals (v_exp / v_rcp / v_log / v_rsq / v_sqrt / v_sin / v_cos),
MFMA, SALU (s_* without waits, nops, barriers, branches, scalar loads and s_endpgm), branches (s_branch / s_cbranch_*), the VALU
and SALU before the first and after the last MFMA, total VGPRs (arch + acc) and the occupancy the compiler reports.
profiles/r08_conv_epilogue_static.txt is this script's output for the parent commit and for the epilogue forms."""
import re
import sys

TRANS = ("v_exp_", "v_rcp_", "v_log_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_branch", "s_cbranch", "s_load_", "s_buffer_load_", "s_setprio", "s_sleep",
            "s_code_end")


def template_args(mangled):
    """The template arguments of a mangled conv_igemm_kernel name: Li<int>E, Lb<0|1>E and L<enum type><int>E literals."""
    out = []
    for kind_, val in re.findall(r"L(i|b|NS_7ConvEpiE)(n?\d+)E", mangled.split("conv_igemm_kernelI", 1)[1]):
        out.append(("true" if val == "1" else "false") if kind_ == "b" else val.replace("n", "-"))
    return ",".join(out)


def kind(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if op.startswith("s_") and not op.startswith(NOT_SALU):
        return "salu"
    return None


def main():
    path, filters = sys.argv[1], sys.argv[2:]
    kernels, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_ZN5orbit17conv_igemm_kernel\w+):", line)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".end_amdhsa_kernel") or t.startswith(".section"):
            if cur in kernels:
                cur = None
            continue
        op = t.split()[0] if t and not t.startswith((";", ".")) else None
        if op and not op.endswith(":"):
            body.append(op)
        for key, pat in (("vgpr", r"; TotalNumVgprs: (\d+)"), ("arch", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"),
                         ("occ", r"; Occupancy: (\d+)")):
            mm = re.match(pat, t)
            if mm:
                kernels.setdefault(cur, {"body": body})[key] = int(mm.group(1))
    names = list(kernels)
    rows = []
    for mangled in names:
        args = template_args(mangled)
        if filters and not any(f in args for f in filters):
            continue
        k = kernels[mangled]
        kinds = [kind(op) for op in k["body"]]
        mf = [i for i, x in enumerate(kinds) if x == "mfma"]
        first, last = (mf[0], mf[-1]) if mf else (len(kinds), len(kinds))
        c = lambda what, lo=0, hi=None: sum(1 for x in kinds[lo:hi] if x == what)  # noqa: E731
        rows.append((args, c("valu"), c("trans"), len(mf), c("salu"), c("branch"), c("valu", 0, first), c("salu", 0, first),
                     c("valu", last), c("salu", last), k.get("vgpr", k.get("arch", 0) + k.get("agpr", 0)), k.get("occ", 0)))
    print("%-52s %5s %5s %5s %5s %6s | %9s %9s | %9s %9s | %5s %3s" % (
        "conv_igemm_kernel<...>", "VALU", "trans", "MFMA", "SALU", "branch", "VALU<mfma", "SALU<mfma", "VALU>mfma", "SALU>mfma", "VGPRs", "occ"))
    for r in sorted(rows):
        print("%-52s %5d %5d %5d %5d %6d | %9d %9d | %9d %9d | %5d %3d" % r)


if __name__ == "__main__":
    main()
