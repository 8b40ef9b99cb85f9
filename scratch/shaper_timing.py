"""BurstShaper.place at 4096 and 65 536 frames of 721 samples, gap 37, device-resident, warm ("Burst shaper"): complex64, sc16 with
a fixed gain and sc16 normalised, each beside (1) a device-to-device copy that moves the same number of bytes and (2) the torch composition a
user writes without the shaper: zeros, a strided scaled assignment, and for sc16 the max, the scale and .to(int16).  Event pairs around `reps`
back-to-back calls, `rounds` rounds with the variants alternating; median and [min, max] over the rounds.
    python3 scratch/shaper_timing.py [out_file [reps [rounds]]]                 -> profiles/r08/shaper_event_timing.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
F, gap, scale, peak = 721, 37, 0.5, 0.9 * 2048
out_file = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
sh = gfdm_amd.BurstShaper(F, scale=scale)
say("build %s  device %s  reps %d rounds %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds))
for n in (4096, 65536):
    S = F + gap
    out_len = n * S
    frames = (torch.randn(n, F, device=dev) + 1j * torch.randn(n, F, device=dev)).to(torch.complex64)
    starts = torch.arange(n, device=dev, dtype=torch.int64) * S + gap
    ws = torch.empty(sh.workspace_bytes(n, out_len), dtype=torch.uint8, device=dev)
    o64 = torch.empty(out_len, dtype=torch.complex64, device=dev)
    o16 = torch.empty(out_len, 2, dtype=torch.int16, device=dev)
    fb = 8 * F * n
    moved = {"c64": fb + 8 * out_len, "sc16": fb + 4 * out_len, "sc16n": 2 * fb + 4 * out_len}     # normalised: the frames are read twice
    src = {k: torch.empty(v // 2, dtype=torch.uint8, device=dev) for k, v in moved.items()}
    dst = {k: torch.empty(v // 2, dtype=torch.uint8, device=dev) for k, v in moved.items()}
    def t_c64():
        o = torch.zeros(out_len, dtype=torch.complex64, device=dev)
        o.view(n, S)[:, gap:] = frames * scale
        return o
    def t_sc16():
        o = torch.zeros(n, S, 2, dtype=torch.int16, device=dev)
        o[:, gap:] = torch.view_as_real(frames * scale).clamp(-32768, 32767).to(torch.int16)
        return o
    def t_sc16n():
        y = torch.view_as_real(frames * scale)
        o = torch.zeros(n, S, 2, dtype=torch.int16, device=dev)
        o[:, gap:] = (y * (peak / y.abs().max())).to(torch.int16)
        return o
    variants = [
        ("c64", "shaper", lambda: sh.place(frames, starts, out_len, out=o64)),
        ("c64", "copy", lambda: dst["c64"].copy_(src["c64"])),
        ("c64", "torch", t_c64),
        ("sc16", "shaper", lambda: sh.place(frames, starts, out_len, sc16=True, out=o16)),
        ("sc16", "copy", lambda: dst["sc16"].copy_(src["sc16"])),
        ("sc16", "torch", t_sc16),
        ("sc16n", "shaper", lambda: sh.place(frames, starts, out_len, sc16=True, peak=peak, out=o16, workspace=ws)),
        ("sc16n", "copy", lambda: dst["sc16n"].copy_(src["sc16n"])),
        ("sc16n", "torch", t_sc16n),
    ]
    # the compositions compute what the shaper computes (fixed gain: exactly; normalised: torch's gain is a float64 quotient applied in fp32)
    assert torch.equal(t_c64(), sh.place(frames, starts, out_len))
    assert torch.equal(t_sc16().view(out_len, 2), sh.place(frames, starts, out_len, sc16=True))
    d = (t_sc16n().view(out_len, 2).int() - sh.place(frames, starts, out_len, sc16=True, peak=peak).int()).abs().max().item()
    assert d <= 1, d
    res = {}
    for r in range(rounds + 1):                                  # round 0 warms up
        for fmt, what, fn in variants:
            for _ in range(3): fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): fn()
            e1.record(); torch.cuda.synchronize()
            if r: res.setdefault((fmt, what), []).append(e0.elapsed_time(e1) / reps * 1e3)
    say("n %d frames of %d, gap %d: out_len %d samples" % (n, F, gap, out_len))
    for fmt in ("c64", "sc16", "sc16n"):
        med = {w: float(np.median(res[(fmt, w)])) for w in ("shaper", "copy", "torch")}
        for w in ("shaper", "copy", "torch"):
            v = res[(fmt, w)]
            say("  %-6s %-7s median %9.2f us [%9.2f, %9.2f]  bytes moved %11d -> %6.3f TB/s%s" % (
                fmt, w, med[w], min(v), max(v), moved[fmt], moved[fmt] / med[w] / 1e6 if w != "torch" else float("nan"),
                "" if w == "copy" else "  time / copy %.2f%s" % (med[w] / med["copy"], "" if w == "shaper" else "  torch / shaper %.2f" % (med[w] / med["shaper"]))))
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
