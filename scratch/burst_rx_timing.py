"""Post-detection step at K=64 M=9 A=52 cp=32, ZF + 2 IC, 4096 and 65 536 bursts, device-resident inputs, warm:
(a) BurstExtractor.extract + demodulate_estimated, with its two kernels also timed alone, (b) demodulate_bursts.  Back-to-back event timing
over `reps` calls, best of two alternating runs.
    python3 scratch/burst_rx_timing.py [reps]                                                   -> profiles/r07/burst_rx_event_timing.txt
    rocprofv3 --kernel-trace --stats -d out -o burst_rx -- python3 scratch/burst_rx_timing.py 20   -> profiles/r07/burst_rx_kernel_stats.csv"""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib", "oracle")]
import numpy as np, torch
import gfdm_amd, gfdm_ref as R
from gfdm_amd.filters import get_frequency_domain_filter
M, K, L, A, cp = 9, 64, 2, 52, 32
N = M * K; F = 2 * K + cp + N
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(0)
smap = np.concatenate((np.arange(1, A // 2 + 1), np.arange(K - A // 2, K)))
taps = get_frequency_domain_filter("rrc", 0.2, M, K, L)
core = np.tile(np.fft.ifft(np.exp(2j * np.pi * rng.random(K))) * np.sqrt(K), 2)
est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, core)
adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, smap, 2, R.qpsk_points())
adv.configure_frames(F, 2 * K + cp, smap, True); adv.set_channel_estimator(est)
ex = gfdm_amd.BurstExtractor(F, 0, True)
print("build", gfdm_amd.lib().gfdm_hip_build_id().decode(), "kernel", adv.kernel_name())
for n in (4096, 65536):
    gap = 64
    S = n * (F + gap)
    s = (torch.randn(S, device="cuda:0") + 1j * torch.randn(S, device="cuda:0")).to(torch.complex64)
    pre = torch.tensor(core.astype(np.complex64), device="cuda:0")
    offs = torch.arange(n, device="cuda:0", dtype=torch.int64) * (F + gap) + 17
    for b in range(0, n, max(1, n // 64)):
        s[int(offs[b]):int(offs[b]) + 2 * K] = pre
    idx = offs[:, None] + torch.arange(2 * K, device="cuda:0")[None, :]
    s[idx.reshape(-1)] = pre.repeat(n)                       # every burst has an invertible preamble
    cfo = torch.rand(n, device="cuda:0") * 0.5 - 0.25
    rot = torch.polar(torch.ones(n, device="cuda:0"), 2 * np.pi * cfo / K).to(torch.complex64)
    out = torch.empty(n, A * M, dtype=torch.complex64, device="cuda:0")
    def a():
        b_ = ex.extract(s, offs, None, rot)
        adv.demodulate_estimated(b_, b_, preamble_stride=F, out=out)
    def b():
        adv.demodulate_bursts(s, offs, rot, out=out)
    bursts = ex.extract(s, offs, None, rot)
    def a1():
        ex.extract(s, offs, None, rot)
    def a2():
        adv.demodulate_estimated(bursts, bursts, preamble_stride=F, out=out)
    res = {}
    for name, fn in (("a", a), ("b", b), ("a1", a1), ("a2", a2), ("a", a), ("b", b), ("a1", a1), ("a2", a2)):
        for _ in range(20): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        res.setdefault(name, []).append(e0.elapsed_time(e1) / reps * 1e3)
    ta, tb = min(res["a"]), min(res["b"])
    byts = n * (704 + 468) * 8
    print("n %6d  (a) alone: extract %8.2f us, demodulate_estimated %8.2f us" % (n, min(res["a1"]), min(res["a2"])))
    print("n %6d  (a) extract + demodulate_estimated %8.2f us %s | (b) demodulate_bursts %8.2f us %s | a/b %.2f | (b) %.2f TB/s = %.1f %% of 8 TB/s"
          % (n, ta, ["%.2f" % v for v in res["a"]], tb, ["%.2f" % v for v in res["b"]], ta / tb, byts / tb / 1e6, byts / tb / 1e6 / 8 * 100))
