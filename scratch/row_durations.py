"""Kernel durations of the five row stages from kernel traces of two builds (profiles/README.md, r23): SymbolMapper.map and .soft on the
shapes of scratch/symbols_timing.py (2^15 rows of 512 symbols, QPSK and the 256-point grid), ConvolutionalCode.encode on those of
scratch/conv_code_timing.py, RateMatcher.match / unmatch / unmatch_hard on those of scratch/rate_matcher_timing.py; device-resident, warm.
    GFDM_HIP_LIB=<lib> rocprofv3 --kernel-trace --stats --output-format csv -d out/<tag> -o t -- python3 scratch/row_durations.py run out/<tag>/plan.json
        per process; tags parent1, new1, parent2, new2, in that order, in one call
    python3 scratch/row_durations.py summarise out <out_file>                           -> profiles/r23/row_kernel_durations.txt
`run` launches 1 + REPS calls per line, one kernel on the GPU at a time, and writes which launches of which kernel family they were;
`summarise` cuts them out of the trace, drops the first of each, pools the processes of a build and gives the verdict per line: the new
median is no higher than the parent's median plus the parent's max - min."""
import sys, os, json, csv, glob, statistics
REPS = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = {"map": "k_symbols_map", "soft": "k_symbols_soft", "encode": "k_cc_encode", "match": "k_rm_match", "unmatch": "k_rm_unmatch", "unmatch_hard": "k_rm_unmatch"}


def run(plan_file):
    sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
    import numpy as np, torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    launched, plan = {}, []

    def call(op, fn):                                    # every call of a row stage goes through here, so that the trace can be cut
        launched[FAMILY[op]] = launched.get(FAMILY[op], 0) + 1
        return fn()

    def line(label, op, fn):
        plan.append(dict(label=label, family=FAMILY[op], first=launched.get(FAMILY[op], 0)))
        for _ in range(1 + REPS):
            call(op, fn)
            torch.cuda.synchronize()

    s, lv = np.sqrt(0.5), np.arange(-15, 16, 2)
    consts = {"qpsk": np.array([-s - 1j * s, s - 1j * s, -s + 1j * s, s + 1j * s]), "grid256": (lv[None, :] + 1j * lv[:, None]).ravel() / np.sqrt(170)}
    n_rows, n_sym = 1 << 15, 512
    for cname, pts in consts.items():
        m = gfdm_amd.SymbolMapper(pts)
        k, g = m.bits_per_symbol(), torch.Generator(device=dev).manual_seed(1)
        data = torch.randint(0, 256, (n_rows, m.row_bytes(n_sym)), dtype=torch.uint8, device=dev, generator=g)
        o_sym = torch.empty(n_rows, n_sym, dtype=torch.complex64, device=dev)
        x = (call("map", lambda: m.map(data, n_sym)) + 0.1 * torch.view_as_complex(torch.randn(n_rows, n_sym, 2, device=dev, generator=g))).to(torch.complex64)
        o_soft = torch.empty(n_rows, n_sym * k, dtype=torch.float32, device=dev)
        line("symbols %-7s map  %d rows of %d" % (cname, n_rows, n_sym), "map", lambda: m.map(data, n_sym, out=o_sym))
        line("symbols %-7s soft %d rows of %d" % (cname, n_rows, n_sym), "soft", lambda: m.soft(x, out=o_soft))
        del data, o_sym, x, o_soft
        torch.cuda.empty_cache()
    m = gfdm_amd.SymbolMapper(consts["qpsk"])
    cc = gfdm_amd.ConvolutionalCode()
    for n_rows, n_info in ((4096, 456), (65536, 456), (64, 1 << 16)):
        g = torch.Generator(device=dev).manual_seed(1)
        rb = m.row_bytes(468 if n_info == 456 else cc.coded_bits(n_info) // 2)
        info = torch.randint(0, 256, (n_rows, cc.info_bytes(n_info)), dtype=torch.uint8, device=dev, generator=g)
        o_coded = torch.empty(n_rows, rb, dtype=torch.uint8, device=dev)
        line("encode %d rows of n_info %d" % (n_rows, n_info), "encode", lambda: cc.encode(info, n_info, out_row_bytes=rb, out=o_coded))
    n_info = 456
    n_coded = cc.coded_bits(n_info)
    keep = gfdm_amd.puncture_pattern("3/4")
    n_tx = gfdm_amd.RateMatcher.tx_bits_of(n_coded, keep)
    rm = gfdm_amd.RateMatcher(n_coded, keep, gfdm_amd.block_interleaver(n_tx, 18))
    for n_rows in (4096, 65536):
        g = torch.Generator(device=dev).manual_seed(1)
        info = torch.randint(0, 256, (n_rows, cc.info_bytes(n_info)), dtype=torch.uint8, device=dev, generator=g)
        coded = call("encode", lambda: cc.encode(info, n_info))
        sent = call("match", lambda: rm.match(coded))
        llr = torch.randn(n_rows, n_tx, device=dev, generator=g)
        o_sent, o_llr = torch.empty_like(sent), torch.empty(n_rows, n_coded, dtype=torch.float32, device=dev)
        line("match        %d rows of n_coded %d, rate 3/4" % (n_rows, n_coded), "match", lambda: rm.match(coded, out=o_sent))
        line("unmatch      %d rows of n_coded %d, rate 3/4" % (n_rows, n_coded), "unmatch", lambda: rm.unmatch(llr, out=o_llr))
        line("unmatch_hard %d rows of n_coded %d, rate 3/4" % (n_rows, n_coded), "unmatch_hard", lambda: rm.unmatch_hard(sent, out=o_llr))
    json.dump(dict(build=gfdm_amd.build_id(), device=torch.cuda.get_device_name(0), reps=REPS, plan=plan, launched=launched), open(plan_file, "w"))


def durations(tag_dir):
    """label -> the REPS durations in us of one process, in the plan's order"""
    meta = json.load(open(os.path.join(tag_dir, "plan.json")))
    spans = {}
    for path in glob.glob(os.path.join(tag_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            for fam in set(FAMILY.values()):
                if fam in r["Kernel_Name"]:
                    spans.setdefault(fam, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for fam, n in meta["launched"].items():
        assert len(spans.get(fam, [])) == n, "%s: %s launched %d times, %d in the trace" % (tag_dir, fam, n, len(spans.get(fam, [])))
        spans[fam].sort()
    out = {}
    for c in meta["plan"]:
        mine = spans[c["family"]][c["first"]:c["first"] + 1 + meta["reps"]]
        out[c["label"]] = [(e - s) / 1e3 for s, e in mine[1:]]
    return meta, out


def summarise(out_dir, out_file):
    runs = {b: [durations(d) for d in sorted(glob.glob(os.path.join(out_dir, b + "[0-9]")))] for b in ("parent", "new")}
    meta = {b: runs[b][0][0] for b in runs}
    lines = ["%s   rocprofv3 --kernel-trace --stats in a run of its own, %d processes alternating parent, new in one call; per process and line one warm-up, then %d launches, "
             "one kernel on the GPU at a time.  parent = build %s, new = build %s.  A line passes when the new median is no higher than the parent's median plus the parent's max - min."
             % (meta["new"]["device"], len(runs["parent"]) + len(runs["new"]), meta["new"]["reps"], meta["parent"]["build"], meta["new"]["build"])]
    worst = 0.0
    for c in meta["new"]["plan"]:
        p = [v for _, d in runs["parent"] for v in d[c["label"]]]
        n = [v for _, d in runs["new"] for v in d[c["label"]]]
        pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        worst = max(worst, nm / pm)
        lines.append("%-52s parent %9.2f us [%9.2f, %9.2f] spread %7.2f   new %9.2f us [%9.2f, %9.2f]   new / parent %.4f   %s" % (
            c["label"], pm, min(p), max(p), spread, nm, min(n), max(n), nm / pm, "pass" if nm <= pm + spread else "FAIL"))
    lines.append("worst new / parent %.4f" % worst)
    print("\n".join(lines))
    open(out_file, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        summarise(*sys.argv[2:4])
