"""Inputs and predictions for the poison tests (tests/test_poison.py on the CPU, tests/test_poison_gpu.py on the GPU): what a zero, an
infinite or a NaN equaliser bin, sample or symbol of ONE block may change, and what it must leave bit-identical.

Data as in test_generic_family_any_subcarrier_count: QPSK on a subcarrier map, RRC taps, a three-tap channel as f_eq.  In every launch
blocks 1 and B - 1 are poisoned: block 1 has neighbours on both sides inside the first workgroup, block B - 1 is the ragged tail.

The prediction (pinned on oracle/gfdm_ref.py by tests/test_poison.py).  A poisoned f_eq bin at subcarrier row j0, column m0 of a block
(bin j0 M + m0 of its N-point spectrum) enters the filter sum of the rows k with (k + i - L/2) mod K = j0, i in [0, L):
    k in [j0 - L + 1 + L/2, j0 + L/2] mod K                                                        (affected_rows)
In S = fft_equalize_filter_downsample only column m0 of those rows is touched; the M-point inverse transform spreads it over the whole
row, so demodulate is non-finite on those rows in full and finite elsewhere.  The cancellation rounds decide a NaN as a finite
constellation point, so after ic_iter rounds the affected rows are still non-finite (S is), every other row is finite, and only the rows
within ic_iter of the set (halo_rows) may differ from the clean result."""
import functools

import numpy as np

import gfdm_ref as R
from gfdm_amd.filters import get_frequency_domain_filter

TOL = 1e-5                     # the project's bound against the float64 oracle
DECISION_GUARD = 1e-4          # as tests/test_parity_gpu.py
IC_ITER = 2                    # cancellation rounds of every IC test here, phase compensation off
H = np.array([1, .3 - .2j, .1j])
NAN, INF = float("nan"), float("inf")
# (complex(inf, inf), not inf + 1j * inf: the latter is nan + inf j)
BINS = {"zero": 0j, "nan": complex(NAN, NAN), "inf": complex(INF, 0.0), "infinf": complex(INF, INF)}

# route: (M, K, L), B, the kernel_name() every handle must report, and how the handles are created
#   generic: under generic_family_for_testing();  ic_mx / dft_mx: set_ic_matrix_cores / set_dft_matrix_cores while creating
#   modes: which receivers the route is about ("fd" fft_equalize_filter_downsample, "zf" demodulate_equalize, "ic" AdvancedReceiver)
ALL = ("fd", "zf", "ic")
ROUTES = {
    "rowlane_2_per_wave": dict(shape=(5, 32, 2), B=2 * 8 + 3, kernel="rowlane", modes=ALL),              # a block boundary inside a wave
    "rowlane_wave": dict(shape=(9, 64, 2), B=2 * 4 + 3, kernel="rowlane", modes=ALL),                    # DPP rounds, part-filled last workgroup
    "rowlane_multiwave": dict(shape=(15, 128, 4), B=3, kernel="rowlane", modes=ALL),                     # edge rows through LDS, matrix-core IC
    "rowlane_2_per_wave_ic_mx": dict(shape=(5, 32, 2), B=2 * 8 + 3, kernel="rowlane", ic_mx=2, modes=("ic",)),
    "rowlane_wave_ic_mx": dict(shape=(9, 64, 2), B=2 * 4 + 3, kernel="rowlane", ic_mx=2, modes=("ic",)),
    "rowlane_jit": dict(shape=(7, 12, 2), B=21 + 5, kernel="rowlane_jit", modes=ALL),                    # K does not divide 64: blocks straddle wavefronts
    "generic_lds_12": dict(shape=(7, 12, 2), B=3, kernel="generic_lds", generic=True, modes=ALL),        # row confinement inside a block
    "generic_lds_32": dict(shape=(5, 32, 2), B=3, kernel="generic_lds", generic=True, modes=ALL),
    "generic_mx_dft": dict(shape=(33, 20, 2), B=3, kernel="generic_lds", generic=True, dft_mx=2, modes=ALL),   # 16-row operand groups with padding rows
    "generic_d0_parked": dict(shape=(31, 256, 2), B=3, kernel="generic_lds", generic=True, modes=ALL),   # IC with d0 parked in the output block
    "generic_global": dict(shape=(15, 1040, 2), B=3, kernel="generic_lds", modes=ALL),                   # tiles in global scratch
    "rader": dict(shape=(127, 16, 2), B=3, kernel="generic_rader", modes=ALL),
}
# the shapes on which tests/test_poison.py pins the prediction
CPU_SHAPES = [(5, 32, 2), (9, 64, 2), (15, 128, 4), (7, 12, 2), (127, 16, 2), (33, 20, 2), (6, 40, 5)]


def bits(a):
    """the raw 32-bit words of a complex64 / float32 array: NaN payloads and signed zeros compare as they are"""
    return np.ascontiguousarray(a).view(np.uint32)


def subcarrier_map(K):
    return np.arange(K) if K < 8 else np.concatenate((np.arange(1, K // 2 - 1), np.arange(K // 2 + 2, K)))


def affected_rows(K, L, j0):
    return sorted({(j0 - L + 1 + L // 2 + i) % K for i in range(L)})


def halo_rows(K, L, j0, ic_iter):
    """rows within ic_iter of the affected set (cyclically), the set itself excluded"""
    aff = set(affected_rows(K, L, j0))
    near = {(k + d) % K for k in aff for d in range(-ic_iter, ic_iter + 1)}
    return sorted(near - aff)


def row_mask(K, M, rows, col=None):
    """(K, M) bool: the whole rows, or only their column `col`"""
    m = np.zeros((K, M), bool)
    if col is None:
        m[list(rows), :] = True
    else:
        m[list(rows), col] = True
    return m


def sites(M, K, B):
    """(block, j0, m0) of every poisoned bin: j0 = K - 1, so that the affected set wraps inside the block"""
    return [(1, K - 1, 1 % M), (B - 1, K - 1, M - 1)]


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def make_case(M, K, L, B):
    """clean inputs and the clean float64 results of one shape; shared between tests, read-only"""
    rng = np.random.default_rng(100 * K + 10 * M + L)
    N = M * K
    taps = get_frequency_domain_filter("rrc", 0.4, M, K, L)
    nt = R.normalize_taps(taps, M)
    smap = subcarrier_map(K)
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = ((1 - 2 * rng.integers(0, 2, (B, len(smap), M))) + 1j * (1 - 2 * rng.integers(0, 2, (B, len(smap), M)))) / np.sqrt(2)
    sym = d.reshape(B, N)
    x = R.modulate(sym, nt, M, K, L)
    feq = np.fft.fft(H, N)[None, :] * np.ones((B, 1))
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    ref_ic, st = R.advanced_receive(xe, nt, M, K, L, smap, R.qpsk_points(), IC_ITER, f_eq=feq, kind="qpsk", return_stages=True)
    return _freeze(dict(M=M, K=K, L=L, B=B, N=N, taps=taps, nt=nt, smap=smap, sym=sym, x=x, feq=feq, xe=xe,
                        ref_fd=R.fft_filter_downsample(xe, nt, M, K, L, feq), ref_zf=R.demodulate(xe, nt, M, K, L, feq), ref_ic=ref_ic,
                        keep_ic=guarded(st, smap, K, M), sites=tuple(sites(M, K, B))))


def guarded(ref_stages, smap, K, M):
    """blocks whose every decided component (all IC iterations) is at least DECISION_GUARD away from zero (tests/test_parity_gpu.py)"""
    keep = None
    for d in [ref_stages["d0"]] + ref_stages["iters"][:-1]:
        v = d.reshape(-1, K, M)[:, smap, :]
        ok = (np.minimum(np.abs(v.real), np.abs(v.imag)).reshape(v.shape[0], -1).min(axis=1) > DECISION_GUARD)
        keep = ok if keep is None else (keep & ok)
    return keep


def poisoned_blocks(c):
    return sorted({b for b, _, _ in c["sites"]})


def clean_blocks(c):
    return [b for b in range(c["B"]) if b not in poisoned_blocks(c)]


def poisoned_feq(c, value):
    feq = np.array(c["feq"], dtype=np.complex128)
    for b, j0, m0 in c["sites"]:
        feq[b, j0 * c["M"] + m0] = value
    return feq


def poisoned_samples(c, src="xe"):
    """a NaN sample in block 1, an inf sample in block B - 1"""
    x = np.array(c[src], dtype=np.complex128)
    (b0, _, _), (b1, _, _) = c["sites"]
    x[b0, c["N"] // 3] = complex(NAN, 0.0)
    x[b1, c["N"] - 1] = complex(0.0, INF)
    return x


def oracle(c, mode, feq, x=None):
    """the float64 result of `mode` on the case's blocks (or x) with the equaliser feq (None: matched filter), shape (B, K, M)"""
    M, K, L = c["M"], c["K"], c["L"]
    x = c["xe"] if x is None else x
    with np.errstate(all="ignore"):
        if mode == "fd":
            r = R.fft_filter_downsample(x, c["nt"], M, K, L, feq)
        elif mode == "zf":
            r = R.demodulate(x, c["nt"], M, K, L, feq)
        else:
            r = R.advanced_receive(x, c["nt"], M, K, L, c["smap"], R.qpsk_points(), IC_ITER, f_eq=feq, kind="qpsk")
    return r.reshape(c["B"], K, M)


def predicted_mask(c, mode):
    """(B, K, M) bool: where a zero, NaN or inf + inf j bin at the case's sites makes `mode` non-finite"""
    M, K, L = c["M"], c["K"], c["L"]
    m = np.zeros((c["B"], K, M), bool)
    for b, j0, m0 in c["sites"]:
        m[b] |= row_mask(K, M, affected_rows(K, L, j0), m0 if mode == "fd" else None)
    return m


def halo_mask(c, mode):
    """(B, K, M) bool: finite elements that may differ from the clean launch (IC only: the rows within IC_ITER of the affected set)"""
    M, K, L = c["M"], c["K"], c["L"]
    m = np.zeros((c["B"], K, M), bool)
    if mode == "ic":
        for b, j0, _ in c["sites"]:
            m[b] |= row_mask(K, M, halo_rows(K, L, j0, IC_ITER))
    return m


def affected_mask(c):
    """(B, K, M) bool: the affected rows of the poisoned blocks in full"""
    return predicted_mask(c, "zf")
