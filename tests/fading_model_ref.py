"""float64 numpy restatement of the fading model's contract (include/gfdm_hip.h, gfdm_hip_fading_model) and of the two table helpers
(gfdm_amd.fading_taps, gfdm_amd.fading_sinusoids) with its own splitmix64: the integer phases, the gains, the delay lines with their
history of zeros, the error budget, a float32 emulation of the run-of-eight scheme, plus the case table of the GPU tests, the case of
the grid-bound test and the constants of the loop test.  Shared by tests/test_fading_model.py (CPU), tests/test_fading_model_gpu.py and
tests/test_fading_grid_bound_gpu.py, and the yardstick of all three: nothing here calls the library."""
import functools
import itertools

import numpy as np

from channel_model_ref import GUARD_CAP, q16, sc16, share_of_budget, signal  # noqa: F401  (the sc16 rule and the seeded inputs are the channel model's)

U64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_PATHS, MAX_SINUSOIDS, MAX_TAPS = 8, 17, 64


# ---- the helpers ----
def mix(z):
    """the splitmix64 finaliser on a Python integer below 2^64"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def hash64(seed, p, s, w):
    return mix((mix(((seed & U64) * GOLDEN + (p << 40 | s << 8 | w)) & U64) + GOLDEN) & U64)


def taps(delays, mags, ntaps):
    """c[p][k] = mags[p] sinc(k - delays[p]) in float64 (an integer distance gives exactly 0 or 1), then float32"""
    out = np.zeros((len(delays), ntaps))
    for p, (d, m) in enumerate(zip(delays, mags)):
        for k in range(ntaps):
            u = k - float(d)
            out[p, k] = float(m) * ((1.0 if u == 0 else 0.0) if u == round(u) else np.sin(np.pi * u) / (np.pi * u))
    return out.astype(np.float32)


def _freq(fd, alpha):
    return min(int(np.rint(fd * np.cos(alpha) * 2.0 ** 64)), (1 << 63) - 1)


def sinusoids(n_paths, N, fd, seed, los=False, k_factor=0.0):
    """(A float32, F int64, phase0 uint64), each (n_paths, N + los): the stratified Clarke model of the issue, value by value"""
    S = N + (1 if los else 0)
    A, F, ph = np.zeros((n_paths, S), np.float32), np.zeros((n_paths, S), np.int64), np.zeros((n_paths, S), np.uint64)
    for p in range(n_paths):
        k = float(k_factor) if (los and p == 0) else 0.0
        for s in range(N):
            u = hash64(seed, p, s, 0) * 2.0 ** -64
            F[p, s] = _freq(fd, 2 * np.pi * (s + u) / N)
            ph[p, s] = hash64(seed, p, s, 1)
            A[p, s] = np.sqrt(1.0 / (N * (1.0 + k)))
        if los and p == 0:
            F[p, N] = _freq(fd, 2 * np.pi * (hash64(seed, 0, N, 0) * 2.0 ** -64))
            ph[p, N] = hash64(seed, 0, N, 1)
            A[p, N] = np.sqrt(k / (k + 1.0))
    return A, F, ph


def j0(x):
    """the Bessel function J0 from its integral (1 / pi) int_0^pi cos(x sin t) dt: the midpoint rule on a periodic integrand, exact to
    rounding at 4096 points for the |x| < 100 of the tests"""
    t = (np.arange(4096) + 0.5) * (np.pi / 4096)
    return float(np.mean(np.cos(float(x) * np.sin(t))))


# ---- the contract ----
def phase(F, Ph0, idx):
    """Phi = (F a + Ph0) mod 2^64 for the absolute indices idx (uint64 array): uint64 arithmetic wraps, which is the contract"""
    with np.errstate(over="ignore"):
        return np.uint64(int(F) & U64) * np.asarray(idx, np.uint64) + np.uint64(int(Ph0))


def phase_bigint(F, Ph0, a):
    """the same with Python integers"""
    return (int(F) * int(a) + int(Ph0)) % (1 << 64)


def gains_at(A, F, Ph0, idx):
    """g[p](a) for the absolute indices idx, complex128 (P, len(idx))"""
    A, F, Ph0 = np.asarray(A, np.float32), np.asarray(F, np.int64), np.asarray(Ph0, np.uint64)
    idx = np.asarray(idx, np.uint64)
    g = np.zeros((A.shape[0], idx.size), np.complex128)
    if A.size * idx.size <= 1 << 16:                                  # few indices: all sinusoids at once
        with np.errstate(over="ignore"):
            top = ((F.astype(np.uint64)[:, :, None] * idx[None, None, :] + Ph0[:, :, None]) >> np.uint64(32)).astype(np.float64)
        return np.sum(A.astype(np.float64)[:, :, None] * np.exp(2j * np.pi * (top * 2.0 ** -32)), axis=1)
    for p in range(A.shape[0]):
        for s in range(A.shape[1]):
            top = (phase(F[p, s], Ph0[p, s], idx) >> np.uint64(32)).astype(np.float64)
            g[p] += float(A[p, s]) * np.exp(2j * np.pi * (top * 2.0 ** -32))
    return g


def gains(A, F, Ph0, offset, n):
    """g[p](a) for a = offset .. offset + n - 1, complex128 (P, n)"""
    return gains_at(A, F, Ph0, np.uint64(offset) + np.arange(n, dtype=np.uint64))


def delay_lines(x, history, c):
    """v[p][i] = sum_k c[p][k] x[i - k] for the n = len(x) - history samples behind the history, zeros before x; and S_pi = sum_k |c[p][k]| |x[i - k]|"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    c = np.asarray(c, np.float32).astype(np.float64)
    P, T = c.shape
    xz = np.concatenate((np.zeros(T - 1, np.complex128), x))
    n = x.size - history
    lo = T - 1 + history
    v, S = np.zeros((P, n), np.complex128), np.zeros((P, n))
    with np.errstate(invalid="ignore"):
        for p in range(P):
            v[p] = np.convolve(xz, c[p])[lo:lo + n]
            S[p] = np.convolve(np.abs(xz), np.abs(c[p]))[lo:lo + n]
    return v, S


def budget_factor(P, T):
    return (T + P + 16) * 2.0 ** -23


def apply(x, history, c, A, F, Ph0, offset):
    """the contract in float64 on complex64 inputs -> (y64, budget): |y - y64| <= budget is what the kernel owes"""
    c, A = np.asarray(c, np.float32), np.asarray(A, np.float32)
    v, S = delay_lines(x, history, c)
    g = gains(A, F, Ph0, offset, v.shape[1])
    with np.errstate(invalid="ignore"):
        y = np.sum(g * v, axis=0)
        abar = np.sum(np.abs(A.astype(np.float64)), axis=1)
        budget = budget_factor(*c.shape) * np.sum(abar[:, None] * S, axis=0)
    return y, budget


# ---- a float32 emulation of the run-of-eight scheme: phasor at the aligned index, the others by at most three fp32 rotations ----
def _c32(re, im):
    return np.asarray(re, np.float32), np.asarray(im, np.float32)


def _cmul32(a, b):
    """(a.re b.re - a.im b.im, a.re b.im + a.im b.re), every operation rounded to float32 (no fused multiply-add: never better than the kernel's)"""
    return _c32(a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _turn32(w):
    """exp(j 2 pi w / 2^64) of uint64 phases from float64, rounded to float32: the tables of create"""
    t = 2 * np.pi * (np.asarray(w, np.uint64).astype(np.int64).astype(np.float64) * 2.0 ** -64)
    return _c32(np.cos(t), np.sin(t))


def gains32(A, F, Ph0, offset, n):
    """g[p](a) as float32 arithmetic forms it -> complex128 (P, n) of float32 values"""
    A, F, Ph0 = np.asarray(A, np.float32), np.asarray(F, np.int64), np.asarray(Ph0, np.uint64)
    r0, r1 = offset >> 3, (offset + n - 1) >> 3
    a0 = np.arange(r0, r1 + 1, dtype=np.uint64) << np.uint64(3)
    out = np.zeros((A.shape[0], n), np.complex128)
    for p in range(A.shape[0]):
        gre, gim = np.zeros((8, a0.size), np.float32), np.zeros((8, a0.size), np.float32)
        for s in range(A.shape[1]):
            f = np.uint64(int(F[p, s]) & U64)
            with np.errstate(over="ignore"):
                top = ((phase(F[p, s], Ph0[p, s], a0) >> np.uint64(32)) + np.uint64(128)) & np.uint64(0xFFFFFFFF)
                steps = {m: _turn32(f * np.uint64(m)) for m in (1, 2, 4)}
            hi = (top.astype(np.int64) >> 8).astype(np.int64)
            hi = np.where(hi >= 1 << 23, hi - (1 << 24), hi)                               # the signed 24 bits
            delta = ((top & np.uint64(255)).astype(np.int64) - 128).astype(np.float32) * np.float32(2 * np.pi * 2.0 ** -32)
            arg = hi.astype(np.float64) * 2.0 ** -23                                      # exact; the sine and cosine correctly rounded
            cs, sn = _c32(np.cos(np.pi * arg), np.sin(np.pi * arg))
            e = [None] * 8
            e[0] = _c32(A[p, s] * (cs - sn * delta), A[p, s] * (sn + cs * delta))
            e[1] = _cmul32(e[0], steps[1])
            e[2] = _cmul32(e[0], steps[2])
            e[3] = _cmul32(e[2], steps[1])
            e[4] = _cmul32(e[0], steps[4])
            e[5] = _cmul32(e[4], steps[1])
            e[6] = _cmul32(e[4], steps[2])
            e[7] = _cmul32(e[6], steps[1])
            for j in range(8):
                gre[j] += e[j][0]
                gim[j] += e[j][1]
        flat = (gre.T.astype(np.float64) + 1j * gim.T.astype(np.float64)).reshape(-1)
        out[p] = flat[offset - (r0 << 3):offset - (r0 << 3) + n]
    return out


def apply32(x, history, c, A, F, Ph0, offset):
    """the kernel's scheme in float32 numpy: the gains of gains32, the delay lines and the sum over the paths accumulated in float32"""
    c = np.asarray(c, np.float32)
    P, T = c.shape
    x = np.asarray(x, np.complex64)
    xz = np.concatenate((np.zeros(T - 1, np.complex64), x))
    n = x.size - history
    g = gains32(A, F, Ph0, offset, n)
    yre, yim = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for p in range(P):
        vre, vim = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for k in range(T):
            seg = xz[T - 1 + history - k:T - 1 + history - k + n]
            vre += c[p, k] * seg.real
            vim += c[p, k] * seg.imag
        gre, gim = g[p].real.astype(np.float32), g[p].imag.astype(np.float32)
        yre = yre + gre * vre - gim * vim
        yim = yim + gre * vim + gim * vre
    return yre.astype(np.float64) + 1j * yim.astype(np.float64)


# ---- the case table of the GPU tests ----
SHAPES = ((1, 1, 1), (1, 8, 1), (2, 3, 3), (4, 8, 16), (8, 17, 64))
NS = (1, 2, 7, 8, 9, 255, 256, 257, 4097, 65539)
OFFSETS = (0, 1, 7, 2 ** 31 - 1, 2 ** 33 - 3, 2 ** 40 + 1)
FD = 0.05                                   # the Doppler of the table's Clarke-like sinusoids, cycles per sample


def histories(T):
    return (0, 1, max(T - 2, 0), T - 1, T + 5)


def sc16_gain(shape):
    """the gain of the table's sc16 cases: far from saturation, and small enough that the guard band gain * budget around every step of q
    holds under GUARD_CAP of a case's components on the restatement alone (tests/test_fading_model.py asserts it); the budget grows with
    T + P + 16 and with the sum of the amplitudes"""
    return {(1, 8, 1): 64.0, (2, 3, 3): 128.0, (4, 8, 16): 16.0, (8, 17, 64): 4.0}.get(tuple(shape), 256.0)


@functools.lru_cache(maxsize=None)
def tables_for(shape, seed=0):
    """(c, A, F, Ph0) of a shape: c with the first coefficient 1 and a decaying tail of both signs; every path of about unit power over its
    sinusoids, divided by sqrt P; the even sinusoids Clarke-like at FD, the odd ones anywhere in the 64 bits (the wrap-around is the
    contract); seeded start phases"""
    P, S, T = shape
    rng = np.random.default_rng([2000, P, S, T, seed])
    c = rng.standard_normal((P, T)) * 0.5 ** (1 + np.arange(T) / 4.0)
    c[:, 0] = 1.0
    A = (0.5 + rng.random((P, S))) / np.sqrt(S * P)
    F = np.rint(FD * np.cos(2 * np.pi * rng.random((P, S))) * 2.0 ** 64).astype(np.int64)
    wide = rng.integers(-2 ** 63, 2 ** 63 - 1, (P, S), dtype=np.int64, endpoint=True)
    F[:, 1::2] = wide[:, 1::2]
    Ph0 = rng.integers(0, 2 ** 64 - 1, (P, S), dtype=np.uint64, endpoint=True)
    return c.astype(np.float32), A.astype(np.float32), F, Ph0


@functools.lru_cache(maxsize=None)
def cases(shape):
    """the 20 cases of one shape: every n twice, and going round with the case number every kind of history, every offset, both parities
    of the input's alignment, every alignment of the output, complex64 and sc16 (as channel_model_ref.cases does it)"""
    out = []
    si = SHAPES.index(tuple(shape))
    T = shape[2]
    for k, n in enumerate(NS):
        for j in range(2):
            c = 2 * k + j + si
            fmt = "sc16" if (k + j) % 2 else "c64"
            out.append(dict(shape=tuple(shape), n=n, history=histories(T)[c % 5], offset=OFFSETS[(c + 3 * j + c // 6) % 6], in_shift=(k + si) % 2,
                            out_shift=(k // 2 + si) % (4 if fmt == "sc16" else 2), fmt=fmt, seed=1000 * si + c))
    return out


def all_cases():
    return list(itertools.chain.from_iterable(cases(s) for s in SHAPES))


@functools.lru_cache(maxsize=None)
def case_data(shape, idx):
    """inputs and float64 expectation of case idx of a shape: x (history + n complex64), the four tables, y, budget"""
    d = dict(cases(shape)[idx])
    d["x"] = signal(d["seed"], d["history"] + d["n"])
    d["c"], d["A"], d["F"], d["Ph0"] = tables_for(tuple(shape))
    d["y"], d["budget"] = apply(d["x"], d["history"], d["c"], d["A"], d["F"], d["Ph0"], d["offset"])
    return d


# ---- past the bounded grid: the constants of gr-gfdm_amd/csrc/gfdm_fading.hip, MIRRORED (tests/test_fading_model.py holds them to the source) ----
FADING_SOURCE = "gr-gfdm_amd/csrc/gfdm_fading.hip"
K_TILE, K_MAX_TILES, K_RUN = 2040, 2048, 8
GRID_OFFSET = 2 ** 33 - 3
GRID_CASES = [
    dict(id="c64-P2-S3-T3", sc16=False, shape=(2, 3, 3), mis=0, seed=71),
    dict(id="sc16-P4-S8-T16-mis", sc16=True, shape=(4, 8, 16), mis=1, seed=72),
]


def grid_geometry(case):
    """n and the Tiling of a grid-bound case: 2 G + 3 tiles with a ragged last one (grid_bound_cases' Tiling and sizing rule)"""
    import grid_bound_cases as G
    n = G.sized(K_MAX_TILES, K_TILE, 1, case["mis"]) - K_TILE // 3
    return dict(n=n, tiling=G.Tiling(K_MAX_TILES, K_TILE, n, case["mis"]))


# ---- the loop with a fading channel: burst_shaper_ref.loop_case() through two paths, Rician on the first, then the channel model's CFO and noise ----
LOOP_DELAYS, LOOP_MAGS, LOOP_NTAPS = (0.0, 1.5), (1.0, 0.3), 8
LOOP_N = 8
LOOP_K = 4.0
LOOP_SEED = 5
LOOP_FDTS_LADDER = (1e-5, 2e-5, 5e-5, 1e-4, 2e-4)                # candidates for the Doppler; the largest at which the margins hold is used
LOOP_FDTS = 5e-5                                                 # chosen by tests/test_fading_model.py::test_loop_preconditions, which asserts the choice


def loop_tables(fd=LOOP_FDTS):
    A, F, Ph0 = sinusoids(len(LOOP_DELAYS), LOOP_N, fd, LOOP_SEED, True, LOOP_K)
    return taps(LOOP_DELAYS, LOOP_MAGS, LOOP_NTAPS), A, F, Ph0


@functools.lru_cache(maxsize=None)
def loop_stream(fd=LOOP_FDTS):
    """(x, z, zbudget, y, budget): the placed stream of the loop case, its faded version (float64 and its budget), and the channel model's
    output for the faded stream rounded to complex64 (taps [1], the channel loop's CFO, noise and seed)"""
    import channel_model_ref as C
    x = C.loop_stream()[0]
    z, zb = apply(x, 0, *loop_tables(fd), 0)
    y, budget = C.apply(z.astype(np.complex64), 0, [1], C.LOOP_F, C.LOOP_NOISE_VOLTAGE, C.LOOP_SEED, 0)
    return x, z, zb, y, budget


def loop_gain_change(fd=LOOP_FDTS):
    """(between, inside): | |g_0| at the middle of the first burst - |g_0| at the middle of the last |, and the largest max - min of |g_0|
    inside one burst"""
    import burst_shaper_ref as B
    c = B.loop_case()
    _, A, F, Ph0 = loop_tables(fd)
    g0 = np.abs(gains(A, F, Ph0, 0, c["out_len"])[0])
    spans = [(int(s), int(s) + c["frame_len"]) for s in c["starts"]]
    mid = [g0[(a + b) // 2] for a, b in spans]
    inside = max(float(g0[a:b].max() - g0[a:b].min()) for a, b in spans)
    return float(abs(mid[0] - mid[-1])), inside
