"""Inputs and the float64 restatement (yardstick B) for the tests of demodulate_bursts (tests/test_burst_receive.py on the CPU,
tests/test_burst_receive_gpu.py on the GPU): captures with bursts [junk | core preamble | cp | block] behind a multipath channel, each
with its own gain, phase and CFO, noise 40 dB below the signal."""
import functools

import numpy as np

import gfdm_ref as R
from gfdm_amd.filters import get_frequency_domain_filter

H = np.array([1, .4 - .2j, .15j, .05])          # the multipath channel of tests/test_estimator_gpu.py
MARGIN = 0.1                                    # precondition (C): distance of every decided component from a QPSK decision boundary


def active_bins(K, A):
    return np.concatenate((np.arange(1, 1 + A // 2), np.arange(K - A // 2, K)))


@functools.lru_cache(maxsize=None)
def make_case(M, K, L, A, nb, seed=0, pre_off=0, cfo_max=0.25, gap=37, taps_kind="rrc"):
    """a capture of nb bursts `gap` samples apart (gap > 17, so a backoff of 17 stays inside the capture); the caller leaves it unchanged.
    taps_kind: "rrc", or a tap family of tests/tap_cases.py (plain demodulation only: with random taps precondition (C) does not hold)"""
    rng = np.random.default_rng(1000 * seed + M * K + A + nb)
    N, cp = M * K, K // 4 + 1
    # roll-off 0.1: the self-interference in front of the first cancellation round is then small enough for precondition (C) at every shape
    # (smallest margin over seeds 0-9: 0.19 at M = 127, K = 16; with 0.3 it falls below 0.01 at the large shapes)
    taps = get_frequency_domain_filter("rrc", 0.1, M, K, L)
    if taps_kind != "rrc":
        import tap_cases
        taps = tap_cases.make_taps(taps_kind, M, K, L)
    nt = R.normalize_taps(taps, M)
    smap = active_bins(K, A)
    pre = np.tile(np.fft.ifft(np.exp(2j * np.pi * rng.random(K))) * np.sqrt(K), 2)
    d = np.zeros((nb, K, M), complex)
    d[:, smap, :] = ((1 - 2 * rng.integers(0, 2, (nb, A, M))) + 1j * (1 - 2 * rng.integers(0, 2, (nb, A, M)))) / np.sqrt(2)
    blocks = np.fft.ifft(np.fft.fft(R.modulate(d.reshape(nb, N), nt, M, K, L), axis=-1) * np.fft.fft(H, N), axis=-1)
    rx_pre = np.tile(np.fft.ifft(np.fft.fft(pre[:K]) * np.fft.fft(H, K)), 2)
    F = pre_off + 2 * K + cp + N
    frames = rng.standard_normal((nb, F)) + 1j * rng.standard_normal((nb, F))          # junk in front of the preamble
    frames[:, pre_off:pre_off + 2 * K] = rx_pre
    frames[:, pre_off + 2 * K:pre_off + 2 * K + cp] = blocks[:, -cp:]
    frames[:, pre_off + 2 * K + cp:] = blocks
    cfo = rng.uniform(-cfo_max, cfo_max, nb)
    gain = (0.7 + 0.6 * rng.random(nb)) * np.exp(2j * np.pi * rng.random(nb))
    frames = frames * gain[:, None] * np.exp(2j * np.pi * cfo[:, None] / K * np.arange(F)[None, :])
    starts = gap + (F + gap) * np.arange(nb)
    n = int(starts[-1] + F + gap)
    sigma = np.sqrt(np.mean(np.abs(blocks) ** 2) * 1e-4 / 2)
    s = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for b in range(nb):
        s[starts[b]:starts[b] + F] += frames[b]
    sym = R.demap_from_resources(d.reshape(nb, N), M, K, smap, True)
    return dict(M=M, K=K, L=L, A=A, N=N, cp=cp, F=F, pre_off=pre_off, taps=taps, nt=nt, smap=smap, preamble=pre, stream=s.astype(np.complex64),
                starts=starts.astype(np.int64), sc_rot=np.exp(2j * np.pi * cfo / K).astype(np.complex64), cfo=cfo, sym=sym)


def virtual_bursts(stream, offsets, sc_rot, backoff, F, cfo_correction=True):
    """e_b[n] = s[off_b - backoff + n] rho_b^n in complex128, s = 0 outside the capture"""
    s = np.asarray(stream, dtype=np.complex128)
    out = np.zeros((len(offsets), F), np.complex128)
    n = np.arange(F)
    for b, off in enumerate(offsets):
        i = int(off) - backoff + n
        ok = (i >= 0) & (i < s.size)
        out[b, ok] = s[i[ok]]
        r = None if sc_rot is None else complex(sc_rot[b])
        if cfo_correction and r is not None and r != 0:
            out[b] *= (np.conj(r) / abs(r)) ** n
    return out


def restatement(c, e, ic_iter):
    """yardstick (B) on the virtual bursts e: estimate_frame (complex64 inputs), demodulate / advanced_receive, demap.
    Returns (symbols, smallest decision margin of any round: precondition C)"""
    M, K, L, A, N = c["M"], c["K"], c["L"], c["A"], c["N"]
    po, bo = c["pre_off"], c["pre_off"] + 2 * K + c["cp"]
    feq = R.estimate_frame(e[:, po:po + 2 * K].astype(np.complex64), c["preamble"].astype(np.complex64), M, K, A, True)
    if ic_iter is None:
        return R.demap_from_resources(R.demodulate(e[:, bo:bo + N], c["nt"], M, K, L, feq), M, K, c["smap"], True), np.inf
    out, st = R.advanced_receive(e[:, bo:bo + N], c["nt"], M, K, L, c["smap"], R.qpsk_points(), ic_iter, f_eq=feq, kind="qpsk", return_stages=True)
    return R.demap_from_resources(out, M, K, c["smap"], True), float(np.min(st["dec_margin"]))


# (M, K, L, A, bursts, seed): the smallest shapes at which each kernel route can go wrong
CASES = {
    "rowlane_7": (9, 64, 2, 52, 7, 0),          # compiled row-lane, one wavefront per block, a partly filled last workgroup
    "rowlane_1": (9, 64, 2, 52, 1, 0),
    "rowlane_mfma": (15, 128, 4, 110, 5, 0),    # cancellation rounds on the matrix cores
    "rowlane_jit": (3, 48, 2, 40, 5, 0),        # run-time instantiated shape
    "generic_127": (127, 16, 2, 12, 3, 0),      # generic family
    "generic_5_32": (5, 32, 2, 24, 5, 0),       # ... and a row-lane shape forced onto it
}
