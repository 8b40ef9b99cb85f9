"""RateMatcher match / unmatch / unmatch_hard, device-resident and warm ("Rate matcher"): 4096 and 65 536 rows of n_coded = 924
(n_info = 456), rate 3/4 (616 transmitted bits), 18-column block interleaver, and beside each a plain device-to-device copy of as many
bytes as the call reads and writes together (unmatch: 4 (616 + 924) a row) -- the copy reads and writes that many, so it moves twice the
call's traffic.  ConvolutionalCode.decode on the depunctured rows is timed as context.  One kernel on the GPU at a time: event pairs
around `reps` back-to-back calls, `rounds` rounds with the variants alternating; median and [min, max].  For kernel durations proper run
it under a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python3 scratch/rate_matcher_timing.py - 20 1 4096).
    python3 scratch/rate_matcher_timing.py [out_file | - [reps [rounds [n_rows ...]]]]      -> profiles/r17/rate_matcher_kernel_durations.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
out_file = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
sizes = [int(a) for a in sys.argv[4:]] or [4096, 65536]
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds))
n_info = 456
cc = gfdm_amd.ConvolutionalCode()
n_coded = cc.coded_bits(n_info)
keep = gfdm_amd.puncture_pattern("3/4")
n_tx = gfdm_amd.RateMatcher.tx_bits_of(n_coded, keep)
rm = gfdm_amd.RateMatcher(n_coded, keep, gfdm_amd.block_interleaver(n_tx, 18))
cb, tb = cc.coded_bytes(n_info), rm.tx_bytes()
for n_rows in sizes:
    g = torch.Generator(device=dev).manual_seed(1)
    info = torch.randint(0, 256, (n_rows, cc.info_bytes(n_info)), dtype=torch.uint8, device=dev, generator=g)
    coded = cc.encode(info, n_info)
    sent = rm.match(coded)
    src = torch.as_tensor(rm.source_index().astype(np.int64), device=dev)
    llr = 4.0 * rm.unmatch_hard(sent)[:, src].contiguous() + torch.randn(n_rows, n_tx, device=dev, generator=g)
    o_sent, o_llr, o_hard = torch.empty_like(sent), torch.empty(n_rows, n_coded, dtype=torch.float32, device=dev), torch.empty(n_rows, n_coded, dtype=torch.float32, device=dev)
    o_info, o_pm = torch.empty_like(info), torch.empty(n_rows, dtype=torch.int32, device=dev)
    depunctured = rm.unmatch(llr)
    errs = int((cc.decode(depunctured, n_info, 4.0) != info).any(dim=1).sum().item())
    moved = {"match": cb + tb, "unmatch": 4 * (n_tx + n_coded), "unmatch_hard": tb + 4 * n_coded}       # bytes a row, read + written
    bufs = {k: (torch.empty(n_rows * v, dtype=torch.uint8, device=dev), torch.empty(n_rows * v, dtype=torch.uint8, device=dev)) for k, v in moved.items()}
    variants = [("match", lambda: rm.match(coded, out=o_sent)), ("copy match", lambda: bufs["match"][0].copy_(bufs["match"][1])),
                ("unmatch", lambda: rm.unmatch(llr, out=o_llr)), ("copy unmatch", lambda: bufs["unmatch"][0].copy_(bufs["unmatch"][1])),
                ("unmatch_hard", lambda: rm.unmatch_hard(sent, out=o_hard)), ("copy unmatch_hard", lambda: bufs["unmatch_hard"][0].copy_(bufs["unmatch_hard"][1])),
                ("decode", lambda: cc.decode(depunctured, n_info, 4.0, out=o_info, path_metric=o_pm))]
    res = {}
    for r in range(rounds + 1):                                  # round 0 warms up
        for name, fn in variants:
            for _ in range(3): fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): fn()
            e1.record(); torch.cuda.synchronize()
            if r: res.setdefault(name, []).append(e0.elapsed_time(e1) / reps * 1e3)
    say("%d rows of n_coded = %d, rate 3/4: %d transmitted bits, %d coded and %d transmitted bytes a row; rows that decode wrong at this noise: %d"
        % (n_rows, n_coded, n_tx, cb, tb, errs))
    med = {name: float(np.median(v)) for name, v in res.items()}
    for name, _ in variants:
        v = res[name]
        extra = ""
        if name in moved:
            extra = "   %6.2f x its copy, %5.1f %% of decode, %7.1f GB/s read + written" % (med[name] / med["copy " + name], 100 * med[name] / med["decode"],
                                                                                            n_rows * moved[name] / med[name] * 1e-3)
        elif name.startswith("copy"):
            extra = "   copy of %d bytes a row" % moved[name[5:]]
        say("  %-18s median %10.2f us [%10.2f, %10.2f]%s" % (name, med[name], min(v), max(v), extra))
    del info, coded, sent, llr, o_sent, o_llr, o_hard, o_info, depunctured, bufs, variants
    torch.cuda.empty_cache()
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
