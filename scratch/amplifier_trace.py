"""Kernel durations of AmplifierModel.apply from a kernel trace, beside a device-to-device copy of the bytes the call reads and writes in the
same run, and for POLY(T, 1) beside ChannelModel.apply at the same T (complex taps, no mixer, no noise) ("Amplifier model"):
2^26 complex64 samples; CLIP, RAPP, SALEH, POLY (1, 1), (4, 3), (16, 5), the neighbours that give the slope over Q and K, and sc16 out.
    rocprofv3 --kernel-trace --output-format csv -d out -o am -- python3 scratch/amplifier_trace.py run out/plan.json
    python3 scratch/amplifier_trace.py summarise out/plan.json out <out_file>          -> profiles/r23/amplifier_kernel_durations.txt
`run` launches, per configuration, 1 + REPS amplifier calls, then (POLY(T, 1) alone) 1 + REPS channel-model calls, then 1 + REPS copies, and
writes the order of the configurations; `summarise` cuts the trace's k_amplify and k_channel launches into groups of 1 + REPS in that
order, finds each group's copies behind it, and drops the first of each."""
import sys, os, json, csv, glob
REPS = 5
N = 1 << 26
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def configs():
    """(name, kind, params, (Q, K) or None, real coefficients, fmt, beside the channel model)"""
    out = []
    for fmt in ("c64", "sc16"):
        out += [("clip", "clip", (1.0,), None, False, fmt, False), ("rapp p 2", "rapp", (2.0, 1.5, 2.0), None, False, fmt, False),
                ("saleh", "saleh", (2.1587, 1.1517, 4.0033, 9.1040), None, False, fmt, False),
                ("poly (1,1)", "poly", (), (1, 1), False, fmt, True), ("poly (4,3)", "poly", (), (4, 3), False, fmt, False),
                ("poly (16,5)", "poly", (), (16, 5), False, fmt, False)]
    out += [("poly (4,1)", "poly", (), (4, 1), False, "c64", True), ("poly (16,1)", "poly", (), (16, 1), False, "c64", True),
            ("poly (1,5)", "poly", (), (1, 5), False, "c64", False), ("poly (4,5)", "poly", (), (4, 5), False, "c64", False),
            ("poly (16,3)", "poly", (), (16, 3), False, "c64", False), ("poly (16,5) real", "poly", (), (16, 5), True, "c64", False)]
    return out


def coefficients(Q, K, real):
    import numpy as np
    rng = np.random.default_rng([3100, Q, K])
    c = (rng.standard_normal((Q, K)) + (0 if real else 1j) * rng.standard_normal((Q, K))) * 0.5 ** (1 + np.arange(Q)[:, None] / 2.0) * 0.1 ** np.arange(K)[None, :]
    c[0, 0] = 1.0
    return c.astype(np.complex64)


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
    for name, kind, params, shape, real, fmt, beside in configs():
        c = coefficients(*shape, real) if shape else None
        Q = shape[0] if shape else 1
        am = gfdm_amd.AmplifierModel(kind, params, c)
        sc16 = fmt == "sc16"
        moved = (8 + (4 if sc16 else 8)) * N
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        for _ in range(1 + REPS):
            am.apply(x[:N + Q - 1], Q - 1, out=out16 if sc16 else out, gain=100.0 if sc16 else 1.0)
            torch.cuda.synchronize()
        if beside:
            ch = gfdm_amd.ChannelModel(taps=c[:, 0])
            for _ in range(1 + REPS):
                ch.apply(x[:N + Q - 1], Q - 1, 0, sc16=sc16, gain=100.0 if sc16 else 1.0, out=out16 if sc16 else out)
                torch.cuda.synchronize()
        for _ in range(1 + REPS):
            dst.copy_(src)
            torch.cuda.synchronize()
        plan.append(dict(name=name, fmt=fmt, bytes=moved, beside=beside))
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
    """the copies of configuration i are the first 1 + REPS copy kernels behind its last k_amplify or k_channel launch and in front of the
    next configuration's first k_amplify launch"""
    import statistics
    meta = json.load(open(plan_file))
    per = 1 + meta["reps"]
    amp = spans(trace_dir, lambda n: "k_amplify" in n)
    chan = spans(trace_dir, lambda n: "k_channel" in n)
    copies = spans(trace_dir, lambda n: "copyBuffer" in n)
    want = per * len(meta["plan"])
    want_ch = per * sum(1 for c in meta["plan"] if c["beside"])
    lines = ["build %s  device %s  rocprofv3 --kernel-trace: n = %d complex64 samples in, %d launches per line after one warm-up, one kernel on the GPU at a time;"
             " copy = the runtime's device-to-device copy kernel on the bytes the call reads and writes, channel = k_channel (ChannelModel.apply, the complex taps"
             " c[:, 0] of POLY(T, 1), no mixer, no noise), same run" % (meta["build"], meta["device"], meta["n"], meta["reps"]),
             "k_amplify launches in the trace %d, expected %d; k_channel %d, expected %d" % (len(amp), want, len(chan), want_ch)]
    if len(amp) == want and len(chan) == want_ch:
        j = 0
        for i, c in enumerate(meta["plan"]):
            mine = amp[per * i:per * (i + 1)]
            his = None
            if c["beside"]:
                his = chan[per * j:per * (j + 1)]
                j += 1
            last = (his or mine)[-1][1]
            until = amp[per * (i + 1)][0] if per * (i + 1) < len(amp) else float("inf")
            win = [(s, e) for s, e in copies if last <= s < until]
            parts = 2 if len(win) >= 2 * per else 1
            m = [sum(e - s for s, e in win[parts * a:parts * (a + 1)]) / 1e3 for a in range(per)][1:] if len(win) >= per else [float("nan")] * meta["reps"]
            k = [(e - s) / 1e3 for s, e in mine[1:]]
            km, mm = statistics.median(k), statistics.median(m)
            line = "%-17s %-4s amplify %9.2f us [%9.2f, %9.2f]  copy %8.2f us [%8.2f, %8.2f]  bytes %10d  amplify / copy %6.2f  ns per sample %7.4f" % (
                c["name"], c["fmt"], km, min(k), max(k), mm, min(m), max(m), c["bytes"], km / mm, km * 1e3 / meta["n"])
            if his:
                h = [(e - s) / 1e3 for s, e in his[1:]]
                hm = statistics.median(h)
                line += "  channel %9.2f us [%9.2f, %9.2f]  amplify / channel %6.2f" % (hm, min(h), max(h), km / hm)
            lines.append(line)
    print("\n".join(lines))
    open(out_file, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summarise(*sys.argv[2:5])
