"""Per-launch timing of EfficientNet-B0's five narrow gated projections (224x224, 200 frames): the streaming kernel with the
gate in its prologue (csrc/pw_stream.hip, conv_rgemm = 1) against se_gate2 + the LDS-tiled conv (conv_rgemm = 0); a layer the
streaming kernel does not serve (240 -> 40) shows the pair in both settings.
Usage (GPU box): python tools/pw_stream_bench.py [--reps 10] [--timeout 300]
Prints, per shape and setting, the µs of every kernel of the pair per pass and the algorithmic TB/s of the projection
(bytes = A + output + residual + pooling partials, the conv_pw_stream profiling record); a watchdog ends the run at --timeout s."""
import argparse
import ctypes
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import orbit_dataset_amd  # noqa: E402,F401
from orbit_dataset_amd import _lib  # noqa: E402

# (name, H, Cin, Cout, R, se chunks of the producing front, residual)
SHAPES = [("1.0  32->16 @112", 112, 32, 16, 8, 98, False), ("2.0  96->24 @56", 56, 96, 24, 4, 49, False),
          ("2.1 144->24 @56 +res", 56, 144, 24, 6, 49, True), ("3.0 144->40 @28", 28, 144, 40, 6, 14, False),
          ("3.1 240->40 @28 +res", 28, 240, 40, 10, 14, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: (print("pw_stream_bench: timeout", flush=True), os._exit(124)))
    signal.alarm(a.timeout)
    lib = _lib.load()
    _lib.require_gpu()
    prev = lib.orbit_get_option(b"conv_rgemm")
    B, d = a.frames, _lib.dptr
    g = torch.Generator(device="cuda").manual_seed(0)
    total = {0: 0.0, 1: 0.0}
    print("%-22s %-8s %-44s %9s %9s" % ("projection", "setting", "kernels (us per pass each)", "us/pass", "proj TB/s"))
    for name, H, Cin, Cout, R, chunks, res in SHAPES:
        r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
        x, w = r(B, H, H, Cin), r(Cout, Cin, 1, 1) * Cin ** -0.5
        sc, sh = 1.0 + 0.1 * r(Cout), 0.1 * r(Cout)
        rs = r(B, H, H, Cout) if res else None
        part = (0.3 + 0.5 * r(B, chunks, Cin)) * (H * H / chunks)
        w1, b1, w2t, b2 = r(R, Cin) * Cin ** -0.5, 0.1 * r(R), r(R, Cin) * R ** -0.5, 0.1 * r(Cin)
        y = torch.empty(B, H, H, Cout, device="cuda")

        def run():
            _lib.check(lib.orbit_op_pw_stream(d(x), d(w), d(sc), d(sh), d(rs), d(part), chunks, d(w1), d(b1), d(w2t), d(b2), R,
                                              d(y), None, B, H, H, Cin, Cout, _lib.stream_handle()), "orbit_op_pw_stream")

        for rnd, opt in enumerate((0, 1, 0, 1)):  # interleaved; both rounds printed, the second one summed
            lib.orbit_set_option(b"conv_rgemm", opt)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            lib.orbit_prof_enable(1)
            for _ in range(a.reps):
                run()
            torch.cuda.synchronize()
            lib.orbit_prof_enable(0)
            ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
            lib.orbit_prof_collect(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n))
            parts, us_sum, tbs = [], 0.0, 0.0
            for i in range(lib.orbit_prof_num_variants()):
                nm = ctypes.create_string_buffer(48)
                ln, vms, vfl, vby = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
                lib.orbit_prof_variant(i, nm, ctypes.byref(ln), ctypes.byref(vms), ctypes.byref(vfl), ctypes.byref(vby))
                if not ln.value:
                    continue
                us = 1e3 * vms.value / a.reps
                us_sum += us
                parts.append("%s %.1f" % (nm.value.decode().split("<")[0], us))
                if nm.value.startswith(b"conv"):  # the projection's own algorithmic bytes over its time
                    tbs = vby.value / (vms.value * 1e-3) / 1e12
            if rnd >= 2:
                total[opt] += us_sum
            print("%-22s %-8s %-44s %9.1f %9.2f" % (name, "rgemm=%d" % opt, ", ".join(parts), us_sum, tbs), flush=True)
    lib.orbit_set_option(b"conv_rgemm", prev)
    print("sum of the five (us per pass, second round): conv_rgemm=0 %.1f  conv_rgemm=1 %.1f" % (total[0], total[1]))
    signal.alarm(0)


if __name__ == "__main__":
    main()
