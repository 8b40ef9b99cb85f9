"""Kernel durations of SpectrumMeter.update and .power from a kernel trace, beside a device-to-device copy of the bytes the call reads in the
same run ("Spectrum meter"): 2^26 complex64 samples; nfft 64, 1024, 4096 at hop = nfft / 2 and hop = nfft; sc16 at 1024; power.
    rocprofv3 --kernel-trace --output-format csv -d out -o sp -- python3 scratch/spectrum_trace.py run out/plan.json
    python3 scratch/spectrum_trace.py summarise out/plan.json out <out_file>          -> profiles/r22/spectrum_kernel_durations.txt
`run` launches, per configuration, 1 + REPS calls and then 1 + REPS copies, and writes the order of the configurations; `summarise` cuts
the trace's k_spectrum_psd / k_spectrum_power launches into groups of 1 + REPS in that order, with the sum pass and the copies behind
them, and drops the first of each.  The same `run` under rocprofv3 --pmc (counters only, a run of its own) and then
    python3 scratch/spectrum_trace.py counters out/plan.json out <out_file>           -> profiles/r22/spectrum_counters.txt"""
import csv
import glob
import json
import os
import sys

REPS = 5
N = 1 << 26
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def configs():
    out = [("psd", nfft, hop, "c64") for nfft in (64, 1024, 4096) for hop in (nfft // 2, nfft)]
    return out + [("psd", 1024, 512, "sc16"), ("psd", 1024, 1024, "sc16"), ("power", 64, 64, "c64"), ("power", 64, 64, "sc16")]


def run(plan_file):
    sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib")]
    import torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn(N, 2, device=dev, generator=g))
    iq = (torch.randn(N, 2, device=dev, generator=g) * 500).to(torch.int16)
    torch.cuda.synchronize()
    plan = []
    for what, nfft, hop, fmt in configs():
        sm = gfdm_amd.SpectrumMeter(nfft, hop=hop)
        src = iq if fmt == "sc16" else x
        nbytes = src.numel() * src.element_size()
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        for _ in range(1 + REPS):
            sm.update(src) if what == "psd" else sm.power(src)
            torch.cuda.synchronize()
        for _ in range(1 + REPS):
            b.copy_(a)                                     # reads and writes nbytes / 2 each: the bytes the call reads, moved once
            torch.cuda.synchronize()
        t = sm.read()
        plan.append(dict(what=what, nfft=nfft, hop=hop, fmt=fmt, bytes=nbytes, segments=t["segments"], samples=t["samples"], build=gfdm_amd.build_id()))
    with open(plan_file, "w") as f:
        json.dump(plan, f)


def summarise(plan_file, trace_dir, out_file):
    plan = json.load(open(plan_file))
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ev = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0) for r in rows]
    main = [i for i, (k, _) in enumerate(ev) if "k_spectrum_psd" in k or "k_spectrum_power" in k]
    assert len(main) == len(plan) * (1 + REPS), (len(main), len(plan))
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["SpectrumMeter.update / .power on 2^26 samples: rocprofv3 --kernel-trace, kernel durations in us, median of %d after one warm-up call; the copy is a"
             % REPS, "device-to-device copy of HALF the bytes the call reads (it reads and writes that half: the same bytes moved) in the same run.  One MI355X, build %s."
             % plan[0]["build"], "", "%-6s %5s %5s %-5s %10s %10s %10s %8s %10s" % ("what", "nfft", "hop", "fmt", "kernel", "sum pass", "copy", "x copy", "GB/s read")]
    for c, cfg in enumerate(plan):
        grp = main[c * (1 + REPS):(c + 1) * (1 + REPS)]
        nxt = main[(c + 1) * (1 + REPS)] if c + 1 < len(plan) else len(ev)
        k = med([ev[i][1] for i in grp[1:]])
        s = med([ev[i + 1][1] for i in grp[1:]])
        copies = [d for i in range(grp[-1] + 2, nxt) for (name, d) in [ev[i]] if "copyBuffer" in name and d > 20.0]      # (read() makes small copies too)
        cp = med(copies[1:]) if len(copies) > 1 else float("nan")
        lines.append("%-6s %5d %5d %-5s %10.1f %10.1f %10.1f %8.2f %10.0f" % (cfg["what"], cfg["nfft"], cfg["hop"], cfg["fmt"], k, s, cp, k / cp, cfg["bytes"] / k / 1000.0))
    open(out_file, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def counters(plan_file, pmc_dir, out_file):
    """the counters of the SECOND k_spectrum_psd / k_spectrum_power dispatch of every configuration, from a --pmc run of `run`"""
    plan = json.load(open(plan_file))
    rows = []
    for path in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    by = {}
    for r in rows:
        if "k_spectrum_psd" in r["Kernel_Name"] or "k_spectrum_power" in r["Kernel_Name"]:
            by.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = by.get(int(r["Dispatch_Id"]), {}).get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    ids = sorted(by)
    assert len(ids) == len(plan) * (1 + REPS), (len(ids), len(plan))
    lines = ["rocprofv3 --pmc, a run of its own (no tracing): the second dispatch of every configuration of profiles/r22/spectrum_kernel_durations.txt, 2^26 samples."
             "  SQ_ACTIVE_INST_*, SQ_WAVE_CYCLES and SQ_BUSY_CYCLES count quad-cycles.  One MI355X, build %s." % plan[0]["build"], ""]
    for c, cfg in enumerate(plan):
        v = by[ids[c * (1 + REPS) + 1]]
        g = lambda k: v.get(k, float("nan"))
        lines.append("%-5s nfft %4d hop %4d %-4s  " % (cfg["what"], cfg["nfft"], cfg["hop"], cfg["fmt"]) + "  ".join("%s %.4g" % (k, v[k]) for k in sorted(v)))
        lines.append("        per sample (wave-level x 64 / 2^26): VALU %.1f, LDS %.2f;  active VALU / wave cycles %.3f, active LDS / wave cycles %.3f;  "
                     "LDS bank-conflict cycles / active LDS %.3f" % (g("SQ_INSTS_VALU") * 64 / N, g("SQ_INSTS_LDS") * 64 / N, g("SQ_ACTIVE_INST_VALU") / g("SQ_WAVE_CYCLES"),
                                                                   g("SQ_ACTIVE_INST_LDS") / g("SQ_WAVE_CYCLES"), g("SQ_LDS_BANK_CONFLICT") / max(g("SQ_ACTIVE_INST_LDS"), 1.0)))
    open(out_file, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    {"run": run, "summarise": summarise, "counters": counters}[sys.argv[1]](*sys.argv[2:])
