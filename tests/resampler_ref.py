"""numpy restatement of the resampler's contract (include/gfdm_hip.h, gfdm_hip_resampler): Python integers for the positions P = pos + i *
step and what is cut from them (idx, frac, p, q, w), float64 for the coefficients and the sum over the same fp32 table and samples, the
error budget, and plan() with a brute-force twin.  Shared by tests/test_resampler.py (CPU) and tests/test_resampler_gpu.py, and the
yardstick of both: nothing here calls the library."""
import numpy as np

ONE = 1 << 32
STEP_MIN, STEP_MAX = 1 << 29, 1 << 35


def lg2(L):
    assert L >= 1 and L & (L - 1) == 0
    return L.bit_length() - 1


def positions(step, pos, n_out):
    """(idx, frac) of outputs 0 .. n_out - 1 as int64 arrays, cut from exact Python integers"""
    P = [pos + i * step for i in range(n_out)]
    return np.array([p >> 32 for p in P], np.int64), np.array([p & (ONE - 1) for p in P], np.int64)


def rows(frac, L, interp):
    """interp 0 -> (p, None); interp 1 -> (q, w): int64 row numbers and w as float64 (a 24-bit integer times 2^-24, exact)"""
    lg = lg2(L)
    if not interp:
        return (frac + (1 << (31 - lg))) >> (32 - lg), None
    q = frac >> (32 - lg)
    w = (((frac << lg) & (ONE - 1)) >> 8).astype(np.float64) * 2.0 ** -24
    return q, w


def coefficients(taps, frac, interp):
    """c[i][t] in float64 from the fp32 table of shape (L + 1, T); d = fp32(h[q + 1] - h[q]), rounded once"""
    h = np.asarray(taps, np.float32)
    L = h.shape[0] - 1
    r, w = rows(frac, L, interp)
    if not interp:
        assert r.min(initial=0) >= 0 and r.max(initial=0) <= L
        return h[r].astype(np.float64)
    assert r.min(initial=0) >= 0 and r.max(initial=0) <= L - 1
    d = (h[1:] - h[:-1]).astype(np.float32)
    return h[r].astype(np.float64) + w[:, None] * d[r].astype(np.float64)


def window(x, history, idx, T):
    """x[idx - D + t] for every output and tap: x holds history + n_in samples, zeros in front of it and behind it"""
    x = np.asarray(x)
    n_in = x.size - history
    j = idx[:, None] - (T - 1) // 2 + np.arange(T)[None, :]
    ok = (j >= -history) & (j < n_in)
    xv = np.zeros(j.shape, np.complex128)
    xv[ok] = x[(j + history)[ok]]
    return xv, j


def resample(x, history, taps, interp, step, pos, n_out):
    """the contract in float64 -> (y64, budget): |y - y64| <= budget = (T + 4) 2^-23 S_i is what the kernel owes"""
    h = np.asarray(taps, np.float32)
    T = h.shape[1]
    idx, frac = positions(step, pos, n_out)
    c = coefficients(h, frac, interp)
    xv, _ = window(np.asarray(x, np.complex64), history, idx, T)
    with np.errstate(invalid="ignore"):
        y = np.sum(c * xv, axis=1)
        S = np.sum(np.abs(c) * np.abs(xv), axis=1)
    return y, (T + 4) * 2.0 ** -23 * S


def share_of_budget(got, y, budget):
    """the worst |got - y| / budget (0 / 0 counts as 0: an exact zero owes nothing and must be exact)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - y)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(err == 0, 0.0, err / budget)
    return float(np.max(share)) if share.size else 0.0


def plan(step, T, pos, n_in, flush):
    """(n_out, advance, next_pos) in closed form"""
    D = (T - 1) // 2
    lim = n_in if flush else n_in + D - T + 1                       # idx(i) < lim
    n_out = 0
    if lim > 0 and (lim << 32) > pos:
        n_out = ((lim << 32) - pos + step - 1) // step
    P = pos + n_out * step
    advance = min(n_in, P >> 32)
    return n_out, advance, P - (advance << 32)


def plan_brute(step, T, pos, n_in, flush):
    """the same by counting: outputs are taken while the condition of the contract holds"""
    D = (T - 1) // 2
    i = 0
    while ((pos + i * step) >> 32) < n_in if flush else ((pos + i * step) >> 32) - D + T - 1 < n_in:
        i += 1
    P = pos + i * step
    advance = min(n_in, P >> 32)
    return i, advance, P - (advance << 32)


def widen(iq):
    """int16 (n, 2) -> complex64, exact"""
    iq = np.asarray(iq, np.int16).reshape(-1, 2)
    return (iq[:, 0].astype(np.float32) + 1j * iq[:, 1].astype(np.float32)).astype(np.complex64)


def signal(seed, n):
    """n seeded complex64 samples of unit variance per component"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def signal_sc16(seed, n):
    """n seeded int16 I/Q pairs over the whole range, both extremes among the first four"""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    iq[:2] = np.array([[-32768, 32767], [32767, -32768]], np.int16)[:min(n, 2)]
    return iq


def table_for(L, T, seed=0):
    """a seeded fp32 table of shape (L + 1, T) whose rows differ (so that a wrong row shows), the centre tap the largest; row L is row 0
    moved by one sample"""
    rng = np.random.default_rng(5000 + 131 * L + 17 * T + seed)
    h = rng.standard_normal((L + 1, T)) * 0.5
    h[:, (T - 1) // 2] += 1.0
    h = h.astype(np.float32)
    h[L, 1:] = h[0, :-1]
    h[L, 0] = 0.0
    return h


def tone_error(T, L, interp, step, f=0.11, n=2048, taps=None):
    """the restatement on exp(j 2 pi f n) with the default table: the worst distance from the tone at f * step / 2^32, away from the ends"""
    import gfdm_amd
    h = gfdm_amd.resampler_taps(L, T, min(1.0, ONE / step)) if taps is None else taps
    x = np.exp(2j * np.pi * f * np.arange(n)).astype(np.complex64)
    pos = T << 32
    n_out = ((n - 2 * T) << 32) // step
    y, _ = resample(x, 0, h, interp, step, pos, n_out)
    t = (pos + step * np.arange(n_out, dtype=np.float64)) / ONE
    return float(np.max(np.abs(y - np.exp(2j * np.pi * f * t))))
