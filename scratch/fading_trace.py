"""Kernel durations of FadingModel.apply from a kernel trace, beside a device-to-device copy of the bytes the call reads and writes and
beside ChannelModel.apply at the same T (real taps, no mixer, no noise) in the same run ("Fading model"): 2^26 complex64
samples; (P, S, T) = (1, 8, 1) flat, (4, 8, 16), (8, 17, 64), and the neighbours that separate the slope over P * S from the slope over
P * T; complex64 and sc16 out.
    rocprofv3 --kernel-trace --output-format csv -d out -o fd -- python3 scratch/fading_trace.py run out/plan.json
    python3 scratch/fading_trace.py summarise out/plan.json out <out_file>          -> profiles/r20/fading_kernel_durations.txt
`run` launches, per configuration, 1 + REPS fading calls, then 1 + REPS channel-model calls, then 1 + REPS copies, and writes the order of
the configurations; `summarise` cuts the trace's k_fade and k_channel launches into groups of 1 + REPS in that order, finds each group's
copies behind it, and drops the first of each."""
import sys, os, json, csv, glob
REPS = 5
N = 1 << 26
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def configs():
    named = [(1, 8, 1), (4, 8, 16), (8, 17, 64)]
    slope = [(1, 1, 1), (1, 17, 1), (4, 1, 16), (4, 17, 16), (4, 8, 1), (4, 8, 64), (8, 8, 1), (8, 1, 64)]
    return [(s, fmt) for s in named for fmt in ("c64", "sc16")] + [(s, "c64") for s in slope]


def tables(shape):
    import numpy as np
    P, S, T = shape
    rng = np.random.default_rng([3000, P, S, T])
    c = rng.standard_normal((P, T)) * 0.5 ** (1 + np.arange(T) / 4.0)
    c[:, 0] = 1.0
    A = (0.5 + rng.random((P, S))) / np.sqrt(S * P)
    F = np.rint(0.05 * np.cos(2 * np.pi * rng.random((P, S))) * 2.0 ** 64).astype(np.int64)
    ph = rng.integers(0, 2 ** 64 - 1, (P, S), dtype=np.uint64, endpoint=True)
    return c.astype(np.float32), A.astype(np.float32), F, ph


def run(plan_file):
    sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
    import torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn(N + 64, 2, device=dev, generator=g))
    out = torch.empty(N, dtype=torch.complex64, device=dev)
    out16 = torch.empty((N, 2), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    plan = []
    for shape, fmt in configs():
        c, A, F, ph = tables(shape)
        T = shape[2]
        fm = gfdm_amd.FadingModel.from_tables(c, A, F, ph)
        ch = gfdm_amd.ChannelModel(taps=c[0])
        sc16 = fmt == "sc16"
        moved = (8 + (4 if sc16 else 8)) * N
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        for _ in range(1 + REPS):
            fm.apply(x[:N + T - 1], T - 1, 12345, out=out16 if sc16 else out, gain=100.0 if sc16 else 1.0)
            torch.cuda.synchronize()
        for _ in range(1 + REPS):
            ch.apply(x[:N + T - 1], T - 1, 12345, sc16=sc16, gain=100.0 if sc16 else 1.0, out=out16 if sc16 else out)
            torch.cuda.synchronize()
        for _ in range(1 + REPS):
            dst.copy_(src)
            torch.cuda.synchronize()
        plan.append(dict(P=shape[0], S=shape[1], T=T, fmt=fmt, bytes=moved))
        del src, dst
    json.dump(dict(build=gfdm_amd.build_id(), device=torch.cuda.get_device_name(0), reps=REPS, n=N, plan=plan), open(plan_file, "w"))


def spans(trace_dir, keep):
    """(start, end) in ns of the kernels of the trace that `keep` takes, in order of start"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if keep(r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return sorted(rows)


def summarise(plan_file, trace_dir, out_file):
    """the copies of configuration i are the first 1 + REPS copy kernels behind its last k_channel launch (the runtime runs a
    device-to-device copy as a kernel of its own, and uploads a handle's table through one too, in front of the configuration's launches)"""
    import statistics
    meta = json.load(open(plan_file))
    per = 1 + meta["reps"]
    fade = spans(trace_dir, lambda n: "k_fade" in n)
    chan = spans(trace_dir, lambda n: "k_channel" in n)
    copies = spans(trace_dir, lambda n: "copyBuffer" in n)
    want = per * len(meta["plan"])
    lines = ["build %s  device %s  rocprofv3 --kernel-trace: n = %d complex64 samples in, %d launches per line after one warm-up, one kernel on the GPU at a time;"
             " copy = the runtime's device-to-device copy kernel on the bytes the call reads and writes, channel = k_channel (ChannelModel.apply, the real taps c[0]"
             " of the same T, no mixer, no noise), same run" % (meta["build"], meta["device"], meta["n"], meta["reps"]),
             "k_fade launches in the trace %d, k_channel %d, expected %d each" % (len(fade), len(chan), want)]
    if len(fade) == want and len(chan) == want:
        for i, c in enumerate(meta["plan"]):
            mine, his = fade[per * i:per * (i + 1)], chan[per * i:per * (i + 1)]
            until = fade[per * (i + 1)][0] if per * (i + 1) < len(fade) else float("inf")
            win = [(s, e) for s, e in copies if his[-1][1] <= s < until]
            parts = 2 if len(win) >= 2 * per else 1
            m = [sum(e - s for s, e in win[parts * a:parts * (a + 1)]) / 1e3 for a in range(per)][1:] if len(win) >= per else [float("nan")] * meta["reps"]
            k = [(e - s) / 1e3 for s, e in mine[1:]]
            h = [(e - s) / 1e3 for s, e in his[1:]]
            km, hm, mm = statistics.median(k), statistics.median(h), statistics.median(m)
            lines.append("P %d S %2d T %2d %-4s fade %9.2f us [%9.2f, %9.2f]  channel %9.2f us [%9.2f, %9.2f]  copy %8.2f us [%8.2f, %8.2f]  bytes %10d  fade / copy %6.2f  fade / channel %6.2f"
                         "  ns per sample %7.3f" % (c["P"], c["S"], c["T"], c["fmt"], km, min(k), max(k), hm, min(h), max(h), mm, min(m), max(m), c["bytes"], km / mm, km / hm,
                                                   km * 1e3 / meta["n"]))
    print("\n".join(lines))
    open(out_file, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summarise(*sys.argv[2:5])
