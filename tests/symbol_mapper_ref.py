"""numpy restatement of the symbol mapper's contract (include/gfdm_hip.h, gfdm_hip_symbol_mapper): bit packing, map, decode and the
max-log soft bits, computed in float64 on the float32 inputs.  Shared by the CPU tests (tests/test_symbol_mapper.py) and the GPU tests
(tests/test_symbol_mapper_gpu.py), and the yardstick of both: nothing here calls the library.  Also the constellations and the seeded
inputs of the GPU tests, so that their preconditions can be checked without a device."""
import functools

import numpy as np

import gfdm_ref as R

GUARD = 1e-5                     # NEAREST decisions are compared where the float64 margin is at least GUARD * max(1, |x|)
GUARD_CAP = 1e-3                 # ... and at most this share of a case's symbols may fall below it
SOFT_ULPS = 8                    # |got - ref| <= SOFT_ULPS * 2^-24 * |s_r| * (d0 + d1)
N_SYMS = (1, 3, 5, 7, 8, 63, 64, 65, 257, 468, 4097)
N_ROWS = (1, 7)
MANY_ROWS = ((5000, 3), (32768 + 7, 5))          # (n_rows, n_sym)
MANY_ROWS_NAMES = ("gr_qpsk", "psk8", "qam64")    # ... on a sign rule, on k = 3 and on k = 6 (rows that end inside a byte)


def _grid(levels):
    """index = len(levels) * a + b  ->  levels[b] + 1j * levels[a]"""
    lv = np.asarray(levels, np.float64)
    return (lv[None, :] + 1j * lv[:, None]).ravel()


def constellations():
    """name -> (points complex64, the rule a handle must report for them under AUTO)"""
    s = np.sqrt(0.5)
    c = {
        "gr_bpsk": (np.array([-1, 1], complex), "bpsk"),                                    # gr::digital::constellation_bpsk
        "gr_qpsk": (R.qpsk_points(), "qpsk"),                                               # gr::digital::constellation_qpsk
        "pygfdm_qpsk": (np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) * s, "nearest"),       # pygfdm/symbolmapping.py constellations[2]
        "psk8": (np.exp(2j * np.pi * np.arange(8) / 8), "nearest"),
        "qam16_grid": (_grid((-3, -1, 1, 3)), "nearest"),                                   # integers: midpoints tie exactly in fp32
        "qam16": (_grid((-3, -1, 1, 3)) / np.sqrt(10), "nearest"),
        "qam64": (_grid(range(-7, 8, 2)) / np.sqrt(42), "nearest"),
        "grid256": (_grid(range(-15, 16, 2)) / np.sqrt(170), "nearest"),
    }
    return {k: (v[0].astype(np.complex64), v[1]) for k, v in c.items()}


def bits_per_symbol(points):
    n = len(points)
    k = int(n).bit_length() - 1
    assert 1 <= k <= 8 and n == 1 << k
    return k


def row_bytes(n_sym, k):
    return (n_sym * k + 7) // 8


def live(count, n_rows):
    return n_rows if count is None else min(max(int(count), 0), n_rows)


def pack(indices, k):
    """point indices (n_rows, n_sym) -> bytes (n_rows, row_bytes): bit j of a symbol is bit k-1-j of its index, rows packed MSB first, every
    row starting on a byte, spare bits 0"""
    idx = np.asarray(indices, np.int64)
    bits = (idx[..., None] >> np.arange(k - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(idx.shape[0], -1).astype(np.uint8), axis=1)


def unpack(data, n_sym, k):
    """bytes (n_rows, row_bytes) -> point indices (n_rows, n_sym); the spare bits are ignored"""
    d = np.asarray(data, np.uint8)
    bits = np.unpackbits(d, axis=1)[:, :n_sym * k].reshape(d.shape[0], n_sym, k).astype(np.int64)
    return (bits << np.arange(k - 1, -1, -1)).sum(axis=-1)


def spare_mask(n_sym, k):
    """(row_bytes,) uint8: the bits of a packed row that carry symbols"""
    m = np.zeros(row_bytes(n_sym, k) * 8, np.uint8)
    m[:n_sym * k] = 1
    return np.packbits(m)


def map(data, n_sym, points, count=None):                # noqa: A001 (the contract's name)
    p = np.asarray(points, np.complex64)
    d = np.asarray(data, np.uint8)
    out = np.zeros((d.shape[0], n_sym), np.complex64)
    n = live(count, d.shape[0])
    out[:n] = p[unpack(d[:n], n_sym, bits_per_symbol(p))]
    return out


def _dist(x, p):
    """d_i in the direct form, float64 on the float32 values: (..., n_points)"""
    x = np.asarray(x, np.complex64)
    xr, xi = x.real.astype(np.float64)[..., None], x.imag.astype(np.float64)[..., None]
    pr, pi = p.real.astype(np.float64), p.imag.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (xr - pr) ** 2 + (xi - pi) ** 2


def indices(symbols, points, rule):
    """the contract's index formulas: the sign tests, or the first strict minimum starting from +inf (so NaN and +inf distances never win)"""
    x = np.asarray(symbols, np.complex64)
    p = np.asarray(points, np.complex64)
    if rule == "qpsk":
        return 2 * (x.imag > 0).astype(np.int64) + (x.real > 0).astype(np.int64)
    if rule == "bpsk":
        return (x.real > 0).astype(np.int64)
    out = np.empty(x.shape, np.int64)
    flat, o = x.ravel(), out.reshape(-1)
    for s in range(0, flat.size, 1 << 15):
        d = _dist(flat[s:s + (1 << 15)], p)
        o[s:s + (1 << 15)] = np.argmin(np.where(np.isnan(d), np.inf, d), axis=-1)        # all +inf: index 0
    return out


def decode(symbols, points, rule, count=None):
    """(bytes (n_rows, row_bytes), margin (n_rows, n_sym)): margin is gfdm_ref.decision_margin of every symbol, +inf in the rows from count on"""
    x = np.asarray(symbols, np.complex64)
    p = np.asarray(points, np.complex64)
    k = bits_per_symbol(p)
    n = live(count, x.shape[0])
    idx = np.zeros(x.shape, np.int64)
    idx[:n] = indices(x[:n], p, rule)
    margin = np.full(x.shape, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        margin[:n] = R.decision_margin(x[:n], p, rule)
    return pack(idx, k), margin


def guarded(symbols, margin):
    """where a NEAREST decision is compared: the float64 margin is at least GUARD * max(1, |x|)"""
    with np.errstate(invalid="ignore", over="ignore"):
        size = np.abs(np.asarray(symbols, np.complex64).astype(np.complex128))
        size[np.isinf(margin) & (margin > 0)] = 0                     # rows beyond count: never read, whatever they hold
        return margin >= GUARD * np.maximum(1.0, size)


def soft(symbols, points, scale=None, count=None):
    """(llr, d0, d1), each float64 (n_rows, n_sym * k): llr = s_r (d1 - d0), d0 / d1 the minima over the points whose bit is 0 / 1; zeros in
    the rows from count on"""
    x = np.asarray(symbols, np.complex64)
    p = np.asarray(points, np.complex64)
    k = bits_per_symbol(p)
    n_rows, n_sym = x.shape
    n = live(count, n_rows)
    s = np.ones(n_rows) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
    d0, d1 = np.zeros((n_rows * n_sym, k)), np.zeros((n_rows * n_sym, k))
    one = ((np.arange(len(p))[:, None] >> np.arange(k - 1, -1, -1)) & 1).astype(bool)                # (n_points, k)
    flat = x[:n].ravel()
    for a in range(0, flat.size, 1 << 14):
        d = _dist(flat[a:a + (1 << 14)], p)
        for j in range(k):
            d1[a:a + d.shape[0], j] = d[:, one[:, j]].min(axis=-1)
            d0[a:a + d.shape[0], j] = d[:, ~one[:, j]].min(axis=-1)
    d0, d1 = d0.reshape(n_rows, n_sym * k), d1.reshape(n_rows, n_sym * k)
    with np.errstate(invalid="ignore"):
        llr = s[:, None] * (d1 - d0)
    llr[n:] = 0
    return llr, d0, d1


def soft_bound(scale, d0, d1):
    """four roundings per distance (two differences, a product, a fused or unfused sum), one for d1 - d0, one for the scale: relative
    to d0 + d1 that is below 6 * 2^-24 to first order; SOFT_ULPS = 8 leaves the second order room.  It holds wherever fp32 picks another
    minimiser than float64 does, because a minimum of rounded values is within the same relative error of the minimum of the exact ones."""
    s = np.ones(d0.shape[0]) if scale is None else np.abs(np.asarray(scale, np.float32).astype(np.float64))
    return SOFT_ULPS * 2.0 ** -24 * s[:, None] * (d0 + d1)


# ---- seeded inputs of the GPU tests ----
def noise_sigma(points):
    """a third of the smallest distance between two points: errors happen, ties do not"""
    p = np.asarray(points, np.complex128)
    d = np.abs(p[:, None] - p[None, :])
    return float(d[d > 0].min()) / 3


@functools.lru_cache(maxsize=None)
def case(name, n_rows, n_sym, seed=0):
    """dict: points, rule, k, idx (n_rows, n_sym), data (the packed bytes), sym (what map must give), x (seeded points plus noise, complex64),
    scale (float32 (n_rows,)).  Cached and never modified."""
    points, rule = constellations()[name]
    k = bits_per_symbol(points)
    rng = np.random.default_rng([seed, n_rows, n_sym, k, len(name)])
    idx = rng.integers(0, 1 << k, (n_rows, n_sym))
    sg = noise_sigma(points)
    x = (points[idx] + sg * (rng.standard_normal((n_rows, n_sym)) + 1j * rng.standard_normal((n_rows, n_sym)))).astype(np.complex64)
    scale = (0.25 + 4 * rng.random(n_rows)).astype(np.float32)
    c = dict(name=name, points=points, rule=rule, k=k, n_rows=n_rows, n_sym=n_sym, idx=idx, data=pack(idx, k), sym=points[idx], x=x, scale=scale)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def shapes():
    return [(r, s) for s in N_SYMS for r in N_ROWS]


def tie_inputs():
    """(x complex64, known index) on the integer 16-QAM grid: midpoints of two and of four points, where every candidate distance is an
    integer and equal in float32 with or without a fused multiply-add; the first index wins.  Index = 4 a + b, point = lv[b] + 1j lv[a]."""
    x = np.array([0 + 1j, 2 + 3j, -2 - 3j, 1 + 0j, 3 + 2j, -1 - 2j, 0 + 0j, 2 + 2j, -2 + 2j, 2 - 2j, -2 - 2j, 0 + 2j], np.complex64)
    want = np.array([9, 14, 0, 6, 11, 1, 5, 10, 8, 2, 0, 9], np.int64)
    return x, want


def special_inputs():
    """NaN and infinite inputs (and zeros) whose index follows from the contract's formulas: (x complex64, index under 'qpsk', under 'bpsk',
    under 'nearest' for any points)"""
    nan, inf = np.nan, np.inf
    x = np.array([complex(nan, 1), complex(1, nan), complex(nan, nan), complex(inf, 1), complex(-inf, 1), complex(1, inf), complex(1, -inf),
                  complex(inf, inf), complex(-inf, -inf), complex(inf, nan), 0j, complex(-0.0, 0.0), complex(0.0, 1), complex(1, 0.0)], np.complex64)
    qpsk = np.array([2, 1, 0, 3, 2, 3, 1, 3, 0, 1, 0, 0, 2, 1], np.int64)
    bpsk = np.array([0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1], np.int64)
    nearest = np.zeros(10, np.int64)                      # the ten non-finite ones: index 0 whatever the points are
    return x, qpsk, bpsk, nearest
