"""Host time per device call through the Python wrapper (profiles/r15): one block of K=64, M=9, `out=` given, wall time / calls, one
synchronise at the end.  python scratch/wrapper_latency.py <directory that holds the gfdm_amd package to measure> [label written as "package"]; GFDM_HIP_LIB picks the
library when that package is a copy outside the tree.  One JSON line."""
import json
import sys
import time
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
import gfdm_amd
from gfdm_amd.filters import get_frequency_domain_filter

M, K, L, CALLS = 9, 64, 2, 4000
taps = get_frequency_domain_filter("rrc", 0.2, M, K, L)
pts = np.array([-1 - 1j, 1 - 1j, -1 + 1j, 1 + 1j]) / np.sqrt(2)
mod = gfdm_amd.Modulator(M, K, L, taps)
dem = gfdm_amd.Demodulator(M, K, L, taps)
adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, np.arange(K), 2, pts)
dev = torch.device("cuda:0")
x = torch.randn(M * K, dtype=torch.complex64, device=dev)
feq = torch.ones(M * K, dtype=torch.complex64, device=dev)
out = torch.empty_like(x)
calls = {"modulate": lambda: mod.modulate(x, out=out), "demodulate_equalize": lambda: dem.demodulate_equalize(x, feq, out=out),
         "advanced_demodulate_equalize": lambda: adv.demodulate_equalize(x, feq, out=out)}
res = {"package": sys.argv[2] if len(sys.argv) > 2 else sys.argv[1], "build_id": gfdm_amd.build_id(), "calls": CALLS}
for name, f in calls.items():
    for _ in range(200):
        f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        f()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    res[name + "_us"] = (t1 - t0) / CALLS * 1e6
print(json.dumps(res))
