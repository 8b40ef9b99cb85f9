"""ConvolutionalCode encode / decode / decode_hard, device-resident and warm ("Convolutional code"): 4096 and 65 536 rows of
n_info = 456 (one K = 64, M = 9, 52-subcarrier QPSK frame at rate 1/2), 64 rows of n_info = 2^16 (decisions in the workspace), and
SymbolMapper.soft -- the decoder's producer -- on the same rows as context.  One kernel on the GPU at a time: event pairs around `reps`
back-to-back calls, `rounds` rounds with the variants alternating; median and [min, max].
    python3 scratch/conv_code_timing.py [out_file [reps [rounds]]]                 -> profiles/r16/conv_code_kernel_durations.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
out_file = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds))
s = np.sqrt(0.5)
pts = np.array([-s - 1j * s, s - 1j * s, -s + 1j * s, s + 1j * s])
m = gfdm_amd.SymbolMapper(pts)
cc = gfdm_amd.ConvolutionalCode()
for n_rows, n_info in ((4096, 456), (65536, 456), (64, 1 << 16)):
    g = torch.Generator(device=dev).manual_seed(1)
    cb, nb = cc.coded_bits(n_info), cc.info_bytes(n_info)
    n_sym = 468 if n_info == 456 else cb // 2                   # 456: the frame's 52 * 9 symbols, six of them padding
    rb = m.row_bytes(n_sym)
    info = torch.randint(0, 256, (n_rows, nb), dtype=torch.uint8, device=dev, generator=g)
    coded = cc.encode(info, n_info, out_row_bytes=rb)
    sym = (m.map(coded, n_sym) + 0.25 * (torch.randn(n_rows, n_sym, device=dev, generator=g) + 1j * torch.randn(n_rows, n_sym, device=dev, generator=g))).to(torch.complex64)
    scale = torch.full((n_rows,), 8.0, dtype=torch.float32, device=dev)
    llr = m.soft(sym, scale)
    hard = m.decode(sym)
    ws_bytes = cc.workspace_bytes(n_info, n_rows)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    o_info = torch.empty(n_rows, nb, dtype=torch.uint8, device=dev)
    o_pm = torch.empty(n_rows, dtype=torch.int32, device=dev)
    o_coded = torch.empty_like(coded)
    o_llr = torch.empty_like(llr)
    dec = cc.decode(llr, n_info, 4.0, workspace=ws)
    errs = int((dec != cc.decode_hard(coded, n_info, workspace=ws)).sum().item())
    variants = [("encode", lambda: cc.encode(info, n_info, out_row_bytes=rb, out=o_coded)),
                ("decode", lambda: cc.decode(llr, n_info, 4.0, out=o_info, path_metric=o_pm, workspace=ws)),
                ("decode_hard", lambda: cc.decode_hard(hard, n_info, out=o_info, path_metric=o_pm, workspace=ws)),
                ("mapper.soft", lambda: m.soft(sym, scale, out=o_llr))]
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
    say("%d rows of n_info = %d (%d steps, %d LLRs and %d coded bytes a row, workspace %d bytes; decoded rows that differ from the payload: %d bytes)"
        % (n_rows, n_info, cc.steps(n_info), llr.shape[1], rb, ws_bytes, errs))
    for name, _ in variants:
        v = res[name]
        med = float(np.median(v))
        say("  %-12s median %10.2f us [%10.2f, %10.2f]   %10.1f information Mbit/s" % (name, med, min(v), max(v), n_rows * n_info / med))
    del info, coded, sym, llr, hard, ws, o_info, o_coded, o_llr, variants
    torch.cuda.empty_cache()
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
