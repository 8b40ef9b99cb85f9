"""float64 numpy restatement of the channel model's contract (include/gfdm_hip.h, gfdm_hip_channel_model): Philox4x32-10, the noise w(a), the
FIR with its history of zeros, the mixer, the error budget and the sc16 rule with its guard band, plus the case table of the GPU tests and
the constants of the loop test.  Shared by tests/test_channel_model.py (CPU) and tests/test_channel_model_gpu.py, and the yardstick of
both: nothing here calls the library."""
import functools
import itertools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """ten rounds on four arrays of counter words (values below 2^32, any common shape) under the key (k0, k1) -> four uint64 arrays of
    32-bit words"""
    c = [np.asarray(x, np.uint64) for x in counter]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 bits: no overflow of uint64
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return c


def noise_words(offset, n, seed):
    """(k0, k1) of the samples offset .. offset + n - 1: one Philox call per aligned pair, even indices take words (0, 1), odd ones (2, 3)"""
    idx = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    pair = idx >> np.uint64(1)
    zero = np.zeros_like(pair)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10([pair & _MASK, pair >> _32, zero, zero], [seed & 0xFFFFFFFF, seed >> 32])
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])


def noise(offset, n, seed):
    """w(a) for a = offset .. offset + n - 1, complex128: E|w|^2 = 2"""
    k0, k1 = noise_words(offset, n, seed)
    u = ((k0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    t = (k1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.cos(2 * np.pi * t) + 1j * r * np.sin(2 * np.pi * t)


W_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))                     # 5.887...: the largest |w|


def fir(x, history, taps):
    """v[i] = sum_t h[t] x[i - t] for the n = len(x) - history samples behind the history, zeros before x; and S_i = sum_t |h[t]| |x[i - t]|"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    h = np.asarray(taps, np.complex64).astype(np.complex128)
    T = h.size
    xz = np.concatenate((np.zeros(T - 1, np.complex128), x))
    n = x.size - history
    with np.errstate(invalid="ignore"):
        v = np.convolve(xz, h)[T - 1 + history:T - 1 + history + n]
        S = np.convolve(np.abs(xz), np.abs(h))[T - 1 + history:T - 1 + history + n]
    return v, S


def rotation(f, offset, n):
    """exp(j 2 pi frac(f a)): the product rounded to float64 once, its distance to the nearest integer exact"""
    a = (np.uint64(offset) + np.arange(n, dtype=np.uint64)).astype(np.float64)
    p = np.float64(f) * a
    return np.exp(2j * np.pi * (p - np.rint(p)))


def apply(x, history, taps, f, s, seed, offset):
    """the contract in float64 on complex64 inputs -> (y64, budget): |y - y64| <= budget is what the kernel owes"""
    taps = np.asarray(taps, np.complex64)
    v, S = fir(x, history, taps)
    n = v.size
    r = v * rotation(f, offset, n) if f != 0 else v
    sigma = float(s) / np.sqrt(2.0)
    w = noise(offset, n, seed) if s != 0 else np.zeros(n, np.complex128)
    y = r + sigma * w
    budget = (taps.size + 10) * 2.0 ** -23 * S + 2.0 ** -20 * sigma * np.abs(w) + 2.0 ** -23 * np.abs(y)
    return y, budget


def share_of_budget(got, y, budget):
    """the worst |got - y| / budget (0 / 0 counts as 0: an exact zero owes nothing and must be exact)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - y)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(err == 0, 0.0, err / budget)
    return float(np.max(share)) if share.size else 0.0


def q16(v):
    """truncation toward zero, saturated to int16, NaN -> 0 (the burst shaper's rule), of float64 values"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.trunc(np.clip(np.where(np.isnan(v), 0.0, v), -32768.0, 32767.0)).astype(np.int16)


def sc16(y, budget, gain):
    """(int16 (n, 2) = q(y * gain), guard (n, 2)): guard marks the components whose float64 value times gain lies within gain * budget of a
    point where q steps -- a non-zero integer; the saturation edges are such integers -- and may therefore come out one LSB off"""
    val = np.stack((y.real, y.imag), axis=1) * float(gain)
    near = np.clip(np.rint(val), -32768.0, 32767.0)                  # (beyond the edges q does not step any more)
    dist = np.where(near == 0, 1.0 - np.abs(val), np.abs(val - near))
    guard = dist <= float(gain) * budget[:, None]
    return q16(val), guard


GUARD_CAP = 0.01                                                     # of the components of a case


def signal(seed, n):
    """n seeded complex64 samples of unit variance per component"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def taps_for(T, seed=0):
    """T complex taps, the first the largest, the tail decaying: complex64"""
    rng = np.random.default_rng(1000 + 17 * T + seed)
    h = (rng.standard_normal(T) + 1j * rng.standard_normal(T)) * 0.5 ** (1 + np.arange(T) / 4.0)
    h[0] = 1.0
    return h.astype(np.complex64)


TS = (1, 2, 3, 8, 64)
NS = (1, 2, 3, 255, 256, 257, 4097, 65539)
FS = (0.0, 0.002, 1.0 / 3.0, 0.4999, -0.5)
SS = (0.0, 1.0)
OFFSETS = (0, 1, 2 ** 31 - 1, 2 ** 33 - 3, 2 ** 40 + 1)


def sc16_gain(T):
    """the gain of the table's sc16 cases: |y| stays below ~15 there, far from saturation (which has its own test); smaller for T = 64, whose
    budget -- and with it the guard band gain * budget around every step of q -- is the widest"""
    return 256.0 if T <= 8 else 32.0



def histories(T):
    return (0, 1, max(T - 2, 0), T - 1, T + 5)


@functools.lru_cache(maxsize=None)
def cases(T):
    """the cases of one T: every n, and going round with the case number every history, f, s, offset, both parities of the input's
    alignment, every alignment of the output, complex64 and sc16.  The strides are chosen so that over the eight n every f meets both s,
    every offset both parities of n, and the (f == 0, s == 0) corner occurs."""
    out = []
    for k, n in enumerate(NS):
        for j in range(2):                                            # two cases per n
            c = 2 * k + j + TS.index(T)
            fmt = "sc16" if (k + j) % 2 else "c64"
            out.append(dict(T=T, n=n, history=histories(T)[c % 5], f=FS[(c // 2 + j) % 5], s=SS[(k + j + c // 5) % 2], offset=OFFSETS[(3 * c + j) % 5],
                            in_shift=c % 2, out_shift=(c // 2) % (4 if fmt == "sc16" else 2), fmt=fmt, seed=100 * T + c))
    return out


def all_cases():
    return list(itertools.chain.from_iterable(cases(T) for T in TS))


@functools.lru_cache(maxsize=None)
def case_data(T, idx):
    """inputs and float64 expectation of case idx of T: x (history + n complex64), taps, y, budget"""
    c = dict(cases(T)[idx])
    c["x"] = signal(c["seed"], c["history"] + c["n"])
    c["taps"] = taps_for(T)
    c["y"], c["budget"] = apply(c["x"], c["history"], c["taps"], c["f"], c["s"], c["seed"], c["offset"])
    return c


# ---- the loop with a channel: burst_shaper_ref.loop_case() at scale 0.5 through three taps, a CFO and noise 20 dB below the frames ----
LOOP_TAPS = (1, 0.25 - 0.1j, 0.1j)
LOOP_F = -0.003
LOOP_NOISE_VOLTAGE = 0.0059
LOOP_SEED = 11
LOOP_GAIN = 11000.0                                                   # sc16: keeps the restatement's output inside 12 bits (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def loop_stream():
    """(x, y, budget): the placed stream of the loop case (complex64, the burst shaper's restatement) and the channel's output for it"""
    import burst_shaper_ref as B
    c = B.loop_case()
    x = B.place_c64(c["frames"], c["frame_len"], c["starts"], c["out_len"], B.LOOP_SCALE)
    y, budget = apply(x, 0, LOOP_TAPS, LOOP_F, LOOP_NOISE_VOLTAGE, LOOP_SEED, 0)
    return x, y, budget
