"""FrameCheck attach / verify / verify with good_row, device-resident and warm ("Frame check"): frames of 61 and 1024 bytes
(payloads of 57 and 1020), 4096 and 65 536 rows, the default whitening, and beside each call a plain device-to-device copy of as many
bytes as the call reads and writes together -- the copy reads and writes that many, so it moves twice the call's traffic.
ConvolutionalCode.decode of the 61-byte frame's rows (n_info = 488) is timed as context; profiles/r16/conv_code_kernel_durations.txt
has the decoder's own figures at n_info = 456.  One kernel on the GPU at a time: event pairs around `reps` back-to-back calls, `rounds`
rounds with the variants alternating; median and [min, max].  Every seventh row carries a flipped bit, so verify's good_row has gaps.
At the small sizes a call's host side is longer than its kernels, so for kernel durations proper run one case under a kernel trace of
its own (rocprofv3 --kernel-trace --stats -- python3 scratch/frame_check_timing.py - 20 1 57:65536).
    python3 scratch/frame_check_timing.py [out_file | - [reps [rounds [n_rows | n_payload:n_rows ...]]]]      -> profiles/r18/frame_check_kernel_durations.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
out_file = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
cases = [a for a in sys.argv[4:]] or ["4096", "65536"]
cases = [(int(a.split(":")[0]), int(a.split(":")[1])) if ":" in a else (p, int(a)) for a in cases for p in ((57, 1020) if ":" not in a else (0,))]
cases.sort(key=lambda c: c[0])
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds))
cc = gfdm_amd.ConvolutionalCode()
for n_payload, n_rows in cases:
    fc = gfdm_amd.FrameCheck(n_payload)
    nf = fc.frame_bytes
    for _ in (0,):
        g = torch.Generator(device=dev).manual_seed(1)
        payload = torch.randint(0, 256, (n_rows, n_payload), dtype=torch.uint8, device=dev, generator=g)
        frames = fc.attach(payload)
        frames[::7, 5 % nf] ^= 0x20
        o_frames, o_payload = torch.empty_like(frames), torch.empty_like(payload)
        o_ok, o_good, o_n = torch.empty(n_rows, dtype=torch.uint8, device=dev), torch.empty(n_rows, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        back, ok, good_row, n_good = fc.verify(frames, good_rows=True)
        bad = n_rows - int(n_good.item())
        assert bad == len(range(0, n_rows, 7)) and bool((back[ok != 0] == payload[ok != 0]).all())
        moved = {"attach": n_payload + nf, "verify": nf + n_payload + 1, "verify + good_row": nf + n_payload + 1 + 1 + 8}     # bytes a row, read + written
        bufs = {k: (torch.empty(n_rows * v, dtype=torch.uint8, device=dev), torch.empty(n_rows * v, dtype=torch.uint8, device=dev)) for k, v in moved.items()}
        variants = [("attach", lambda: fc.attach(payload, out=o_frames)), ("copy attach", lambda: bufs["attach"][0].copy_(bufs["attach"][1])),
                    ("verify", lambda: fc.verify(frames, out={"payload": o_payload, "ok": o_ok})), ("copy verify", lambda: bufs["verify"][0].copy_(bufs["verify"][1])),
                    ("verify + good_row", lambda: fc.verify(frames, good_rows=True, out={"payload": o_payload, "ok": o_ok, "good_row": o_good, "n_good": o_n})),
                    ("copy verify + good_row", lambda: bufs["verify + good_row"][0].copy_(bufs["verify + good_row"][1]))]
        if n_payload == 57:
            n_info = fc.frame_bits
            llr = 4.0 * (1.0 - 2.0 * torch.randint(0, 2, (n_rows, cc.coded_bits(n_info)), device=dev, generator=g).float())
            o_info = torch.empty(n_rows, cc.info_bytes(n_info), dtype=torch.uint8, device=dev)
            variants.append(("decode", lambda: cc.decode(llr, n_info, 4.0, out=o_info)))
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
        say("%d rows of %d payload bytes, frames of %d bytes; rows with a flipped bit, all dropped: %d" % (n_rows, n_payload, nf, bad))
        med = {name: float(np.median(v)) for name, v in res.items()}
        for name, _ in variants:
            v = res[name]
            extra = ""
            if name in moved:
                extra = "   %6.2f x its copy, %7.1f GB/s read + written" % (med[name] / med["copy " + name], n_rows * moved[name] / med[name] * 1e-3)
                if "decode" in med:
                    extra += ", %5.1f %% of decode" % (100 * med[name] / med["decode"])
            elif name.startswith("copy"):
                extra = "   copy of %d bytes a row" % moved[name[5:]]
            say("  %-24s median %10.2f us [%10.2f, %10.2f]%s" % (name, med[name], min(v), max(v), extra))
        del payload, frames, o_frames, o_payload, o_ok, o_good, o_n, back, ok, good_row, bufs, variants
        torch.cuda.empty_cache()
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
