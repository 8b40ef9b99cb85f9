"""ChannelModel.apply at 2^26 samples (1 GiB of traffic as complex64, beyond the 256 MiB Infinity Cache), device-resident, warm (DESIGN.md,
"Channel model"): the plain configuration (T = 1, f = 0, s = 0) and the full one (T = 4, f != 0, s > 0), each as complex64 and sc16 out and
each beside a device-to-device copy that moves the same number of bytes (read + written).  Event pairs around `reps` back-to-back calls,
`rounds` rounds with the variants alternating; median and [min, max].
    python3 scratch/channel_timing.py [out_file [reps [rounds]]]                 -> profiles/r10/channel_event_timing.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
n = 1 << 26
out_file = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d  n %d samples" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds, n))
g = torch.Generator(device=dev).manual_seed(1)
x = torch.view_as_complex(torch.randn(n, 2, device=dev, generator=g))
o64 = torch.empty(n, dtype=torch.complex64, device=dev)
o16 = torch.empty(n, 2, dtype=torch.int16, device=dev)
configs = {"plain T=1 f=0 s=0": gfdm_amd.ChannelModel(), "full T=4 f=0.01 s=0.1": gfdm_amd.ChannelModel(0.1, 0.01, 1.0, [1, 0.25 - 0.1j, 0.1j, -0.05], 11)}
variants = []
for cname, ch in configs.items():
    for fmt, moved in (("c64", 16 * n), ("sc16", 12 * n)):
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        fn = (lambda ch=ch: ch.apply(x, out=o64)) if fmt == "c64" else (lambda ch=ch: ch.apply(x, sc16=True, gain=1000.0, out=o16))
        variants.append((cname, fmt, "channel", moved, fn))
        variants.append((cname, fmt, "copy", moved, lambda src=src, dst=dst: dst.copy_(src)))
res = {}
for r in range(rounds + 1):                                  # round 0 warms up
    for cname, fmt, what, moved, fn in variants:
        for _ in range(2): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        if r: res.setdefault((cname, fmt, what), []).append(e0.elapsed_time(e1) / reps * 1e3)
for cname in configs:
    say(cname)
    for fmt, moved in (("c64", 16 * n), ("sc16", 12 * n)):
        med = {w: float(np.median(res[(cname, fmt, w)])) for w in ("channel", "copy")}
        for w in ("channel", "copy"):
            v = res[(cname, fmt, w)]
            say("  %-5s %-8s median %9.2f us [%9.2f, %9.2f]  bytes moved %11d -> %6.3f TB/s%s" % (
                fmt, w, med[w], min(v), max(v), moved, moved / med[w] / 1e6, "" if w == "copy" else "  time / copy %.2f" % (med[w] / med["copy"])))
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
