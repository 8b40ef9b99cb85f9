"""Hardware counters of k_fade ("Fading model"): which resource the slopes over P * S and over P * T point at.  A run of its
own, counters only, no tracing:
    rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \
        --output-format csv -d out -o fd -- python3 scratch/fading_counters.py run out/plan.json
    python3 scratch/fading_counters.py summarise out/plan.json out <out_file>          -> profiles/r20/fading_counters.txt
`run` launches every configuration twice (the first is the warm-up); `summarise` takes the second k_fade dispatch of each."""
import sys, os, json, csv, glob
N = 1 << 26
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1, 1, 1), (1, 8, 1), (1, 17, 1), (4, 8, 1), (4, 8, 16), (4, 8, 64), (8, 17, 64)]


def run(plan_file):
    sys.path.insert(0, os.path.join(ROOT, "scratch"))
    import fading_trace
    sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
    import torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.view_as_complex(torch.randn(N + 64, 2, device=dev, generator=g))
    out = torch.empty(N, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    for shape in CONFIGS:
        fm = gfdm_amd.FadingModel.from_tables(*fading_trace.tables(shape))
        for _ in range(2):
            fm.apply(x[:N + shape[2] - 1], shape[2] - 1, 12345, out=out)
            torch.cuda.synchronize()
    json.dump(dict(build=gfdm_amd.build_id(), device=torch.cuda.get_device_name(0), n=N, plan=[list(s) for s in CONFIGS]), open(plan_file, "w"))


def summarise(plan_file, trace_dir, out_file):
    meta = json.load(open(plan_file))
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_fade" in r["Kernel_Name"]:
                rows.setdefault(int(r["Dispatch_Id"]), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    order = sorted(rows)
    lines = ["build %s  device %s  rocprofv3 --pmc, a run of its own: n = %d complex64 samples, complex64 out, the second of two launches per shape; SQ_ACTIVE_INST_*,"
             " SQ_WAVE_CYCLES and SQ_BUSY_CYCLES count quad-cycles summed over the chip" % (meta["build"], meta["device"], meta["n"]),
             "k_fade dispatches in the collection %d, expected %d" % (len(order), 2 * len(meta["plan"]))]
    if len(order) == 2 * len(meta["plan"]):
        for i, (P, S, T) in enumerate(meta["plan"]):
            c = rows[order[2 * i + 1]]
            get = lambda k: c.get(k, float("nan"))
            lines.append("P %d S %2d T %2d  " % (P, S, T) + "  ".join("%s %.4g" % (k, c[k]) for k in sorted(c)))
            lines.append("             VALU instructions per sample %.1f (wave-level x 64 / n), LDS %.2f;  active VALU / wave cycles %.3f, active LDS / wave cycles %.3f;"
                         "  LDS bank-conflict cycles / active LDS %.3f" % (get("SQ_INSTS_VALU") * 64 / meta["n"], get("SQ_INSTS_LDS") * 64 / meta["n"],
                                                                          get("SQ_ACTIVE_INST_VALU") / get("SQ_WAVE_CYCLES"), get("SQ_ACTIVE_INST_LDS") / get("SQ_WAVE_CYCLES"),
                                                                          get("SQ_LDS_BANK_CONFLICT") / max(get("SQ_ACTIVE_INST_LDS"), 1.0)))
    print("\n".join(lines))
    open(out_file, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summarise(*sys.argv[2:5])
