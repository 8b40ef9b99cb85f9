"""SymbolMapper decode / soft / map at 2^24 symbols as 2^15 rows of 512, device-resident, warm ("Symbol mapper"): GNU Radio QPSK
(the sign tests; soft over 4 points) and a 256-point grid (NEAREST), each beside a device-to-device copy that moves the same number of
bytes (read + written).  Inputs and outputs rotate through rings whose footprint is above the 256 MiB Infinity Cache, so no call finds its
input in the cache.  Event pairs around `reps` back-to-back calls, `rounds` rounds with the variants alternating; median and [min, max].
    python3 scratch/symbols_timing.py [out_file [reps [rounds]]]                 -> profiles/r09/symbols_event_timing.txt"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd
n_rows, n_sym, RING = 1 << 15, 512, 4
out_file = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
dev = torch.device("cuda:0")
say("build %s  device %s  reps %d rounds %d  %d rows of %d symbols, rings of %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), reps, rounds, n_rows, n_sym, RING))
s = np.sqrt(0.5)
lv = np.arange(-15, 16, 2)
consts = {"qpsk": np.array([-s - 1j * s, s - 1j * s, -s + 1j * s, s + 1j * s]), "grid256": (lv[None, :] + 1j * lv[:, None]).ravel() / np.sqrt(170)}
n = n_rows * n_sym
for cname, pts in consts.items():
    m = gfdm_amd.SymbolMapper(pts)
    k, rb = m.bits_per_symbol(), m.row_bytes(n_sym)
    g = torch.Generator(device=dev).manual_seed(1)
    data = [torch.randint(0, 256, (n_rows, rb), dtype=torch.uint8, device=dev, generator=g) for _ in range(RING)]
    x = [(m.map(d, n_sym) + 0.1 * (torch.randn(n_rows, n_sym, device=dev, generator=g) + 1j * torch.randn(n_rows, n_sym, device=dev, generator=g))).to(torch.complex64)
         for d in data]
    o_sym = [torch.empty(n_rows, n_sym, dtype=torch.complex64, device=dev) for _ in range(RING)]
    o_dec = [torch.empty(n_rows, rb, dtype=torch.uint8, device=dev) for _ in range(RING)]
    o_soft = [torch.empty(n_rows, n_sym * k, dtype=torch.float32, device=dev) for _ in range(RING)]
    moved = {"decode": 8 * n + n_rows * rb, "soft": 8 * n + 4 * k * n, "map": n_rows * rb + 8 * n}
    assert torch.equal(m.decode(m.map(data[0], n_sym)), data[0])
    it = [0]
    def ring(fn):
        def call():
            it[0] = (it[0] + 1) % RING
            fn(it[0])
        return call
    variants = []
    for op in ("decode", "soft") + (("map",) if cname == "qpsk" else ()):
        half = moved[op] // 2
        src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(RING)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(RING)]
        fn = {"decode": lambda i: m.decode(x[i], out=o_dec[i]), "soft": lambda i: m.soft(x[i], out=o_soft[i]), "map": lambda i: m.map(data[i], n_sym, out=o_sym[i])}[op]
        variants.append((op, "mapper", ring(fn)))
        variants.append((op, "copy", ring(lambda i, src=src, dst=dst: dst[i].copy_(src[i]))))
    res = {}
    for r in range(rounds + 1):                                  # round 0 warms up
        for op, what, fn in variants:
            for _ in range(3): fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): fn()
            e1.record(); torch.cuda.synchronize()
            if r: res.setdefault((op, what), []).append(e0.elapsed_time(e1) / reps * 1e3)
    say("%s (k = %d, rule %s)" % (cname, k, m.decision_rule()))
    for op in dict.fromkeys(v[0] for v in variants):
        med = {w: float(np.median(res[(op, w)])) for w in ("mapper", "copy")}
        for w in ("mapper", "copy"):
            v = res[(op, w)]
            say("  %-6s %-6s median %9.2f us [%9.2f, %9.2f]  bytes moved %11d -> %6.3f TB/s%s" % (
                op, w, med[w], min(v), max(v), moved[op], moved[op] / med[w] / 1e6, "" if w == "copy" else "  time / copy %.2f" % (med[w] / med["copy"])))
    del data, x, o_sym, o_dec, o_soft, variants
    torch.cuda.empty_cache()
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    open(out_file, "w").write("\n".join(lines) + "\n")
