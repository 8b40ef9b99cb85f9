"""Resampler.resample at 2^20 and 2^26 output samples, device-resident, warm ("Resampler"): T 8, 16, 32 at L = 128, both interp,
steps 1.0001, 4/5 and 5/4, complex64 and sc16 in, each beside a device-to-device copy that moves the bytes the call reads and writes.
Event pairs around `reps` back-to-back calls, `rounds` rounds with call and copy alternating; median and [min, max].
    python3 scratch/resampler_timing.py [out_file [reps [rounds]]]               -> profiles/r19/resampler_kernel_durations.txt"""
import sys, os
from fractions import Fraction
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
out_file = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds))
g = torch.Generator(device=dev).manual_seed(1)
n_max = int((1 << 26) * 1.26) + 64
x64 = torch.view_as_complex(torch.randn(n_max, 2, device=dev, generator=g))
x16 = torch.randint(-2048, 2048, (n_max, 2), device=dev, generator=g).to(torch.int16)
out = torch.empty(1 << 26, dtype=torch.complex64, device=dev)
for n_out in (1 << 20, 1 << 26):
    say("n_out %d" % n_out)
    for rate in (1.0001, Fraction(4, 5), Fraction(5, 4)):
        step = gfdm_amd.resampler_step(rate)
        n_in = ((n_out * step) >> 32) + 1
        for T in (8, 16, 32):
            for interp in ("nearest", "linear"):
                rs = gfdm_amd.Resampler(step, n_phases=128, n_taps=T, interp=interp)
                for fmt, x, sb in (("c64", x64, 8), ("sc16", x16, 4)):
                    moved = 8 * n_out + sb * n_in
                    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                    dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                    fns = {"resample": lambda: rs.resample(x[:n_in], n_out=n_out, out=out[:n_out]), "copy": lambda: dst.copy_(src)}
                    res = {}
                    for r in range(rounds + 1):                                  # round 0 warms up
                        for what, fn in fns.items():
                            fn()
                            torch.cuda.synchronize()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(reps): fn()
                            e1.record(); torch.cuda.synchronize()
                            if r: res.setdefault(what, []).append(e0.elapsed_time(e1) / reps * 1e3)
                    med = {w: float(np.median(v)) for w, v in res.items()}
                    say("  step %-6s T %2d %-7s %-4s resample %9.2f us [%9.2f, %9.2f]  copy %9.2f us [%9.2f, %9.2f]  bytes %11d  %6.3f TB/s  time / copy %5.2f" % (
                        str(rate), T, interp, fmt, med["resample"], min(res["resample"]), max(res["resample"]), med["copy"], min(res["copy"]), max(res["copy"]),
                        moved, moved / med["resample"] / 1e6, med["resample"] / med["copy"]))
                    del src, dst
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
