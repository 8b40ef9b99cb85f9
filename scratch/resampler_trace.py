"""Kernel durations of Resampler.resample from a kernel trace, beside a device-to-device copy of the bytes the call reads and writes in the
same run ("Resampler"): 2^20 and 2^26 outputs; T 8, 16, 32 at L = 128; both interp; steps 1.0001, 4/5, 5/4 and, at T = 16
linear, 8; complex64 and sc16 in.
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d out -o rs -- python3 scratch/resampler_trace.py run out/plan.json
    python3 scratch/resampler_trace.py summarise out/plan.json out <out_file>          -> profiles/r19/resampler_kernel_durations.txt
`run` launches, per configuration, 1 + REPS resample calls, then 1 + REPS copies, and writes the order of the configurations; `summarise`
cuts the trace's k_resample launches into groups of 1 + REPS in that order, finds each group's copies behind it, and drops the first of each."""
import sys, os, json, csv, glob
from fractions import Fraction
REPS = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def configs():
    out = []
    for n_out in (1 << 20, 1 << 26):
        for rate in ("1.0001", "4/5", "5/4"):
            for T in (8, 16, 32):
                for interp in ("nearest", "linear"):
                    for fmt in ("c64", "sc16"):
                        out.append((n_out, rate, T, interp, fmt))
        for fmt in ("c64", "sc16"):
            out.append((n_out, "8", 16, "linear", fmt))
    return out


def run(plan_file):
    sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
    import torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    n_max = 8 * (1 << 26) + 64
    x64 = torch.view_as_complex(torch.randn(n_max, 2, device=dev, generator=g))
    x16 = (torch.randn(n_max, 2, device=dev, generator=g) * 500).to(torch.int16)
    out = torch.empty(1 << 26, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    plan = []
    for n_out, rate, T, interp, fmt in configs():
        step = gfdm_amd.resampler_step(Fraction(rate))
        n_in = ((n_out * step) >> 32) + 1
        rs = gfdm_amd.Resampler(step, n_phases=128, n_taps=T, interp=interp)
        x, sb = (x64, 8) if fmt == "c64" else (x16, 4)
        moved = 8 * n_out + sb * n_in
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        for _ in range(1 + REPS):
            rs.resample(x[:n_in], n_out=n_out, out=out[:n_out])
            torch.cuda.synchronize()
        for _ in range(1 + REPS):
            dst.copy_(src)
            torch.cuda.synchronize()
        plan.append(dict(n_out=n_out, rate=rate, T=T, interp=interp, fmt=fmt, n_in=n_in, bytes=moved))
        del src, dst
    json.dump(dict(build=gfdm_amd.build_id(), device=torch.cuda.get_device_name(0), reps=REPS, plan=plan), open(plan_file, "w"))


def spans(trace_dir, keep):
    """(start, end) in ns of the kernels of the trace that `keep` takes, in order of start"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if keep(r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return sorted(rows)


def summarise(plan_file, trace_dir, out_file):
    """The runtime runs a device-to-device copy as a kernel of its own (__amd_rocclr_copyBuffer), and uploads a handle's table through one
    too: the copies of configuration i are the first 1 + REPS copy kernels between its last k_resample launch and the next
    configuration's first (a copy the runtime splits into two kernels counts as their sum)."""
    import statistics
    meta = json.load(open(plan_file))
    per = 1 + meta["reps"]
    kern = spans(trace_dir, lambda n: "k_resample" in n)
    copies = spans(trace_dir, lambda n: "copyBuffer" in n)
    lines = ["build %s  device %s  rocprofv3 --kernel-trace: %d launches per line after one warm-up, one kernel on the GPU at a time; copy = the runtime's"
             " device-to-device copy kernel on the bytes the call reads and writes, same run" % (meta["build"], meta["device"], meta["reps"]),
             "k_resample launches in the trace %d, expected %d" % (len(kern), per * len(meta["plan"]))]
    if len(kern) == per * len(meta["plan"]):
        for i, c in enumerate(meta["plan"]):
            mine = kern[per * i:per * (i + 1)]
            until = kern[per * (i + 1)][0] if per * (i + 1) < len(kern) else float("inf")
            win = [(s, e) for s, e in copies if mine[-1][1] <= s < until]
            parts = 2 if len(win) >= 2 * per else 1
            m = [sum(e - s for s, e in win[parts * a:parts * (a + 1)]) / 1e3 for a in range(per)][1:] if len(win) >= per else [float("nan")] * meta["reps"]
            k = [(e - s) / 1e3 for s, e in mine[1:]]
            km, mm = statistics.median(k), statistics.median(m)
            lines.append("n_out %8d step %-6s T %2d %-7s %-4s kernel %9.2f us [%9.2f, %9.2f]  copy %9.2f us [%9.2f, %9.2f] (%d kernel%s)  bytes %11d  %6.3f TB/s  kernel / copy %5.2f" % (
                c["n_out"], c["rate"], c["T"], c["interp"], c["fmt"], km, min(k), max(k), mm, min(m), max(m), parts, "s" if parts > 1 else "", c["bytes"],
                c["bytes"] / km / 1e6, km / mm))
    print("\n".join(lines))
    open(out_file, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summarise(*sys.argv[2:5])
