"""Filter taps, kernel routes and wrong tap handlings for the tap tests (tests/test_taps.py on the CPU, tests/test_taps_gpu.py on the GPU).

The suite's other parity tests feed the kernels root-raised-cosine taps: real, even in the bin index (t[i] == t[(L M - i) % (L M)]) and, above
overlap 2, nearly empty outside the two main parts.  A kernel that conjugates the taps, reads a part back to front, swaps the cross terms
of the complex product or drops the outer parts is the same function on such taps, to 1e-15 or to below TOL (asserted once in
tests/test_taps.py).  The families here are not:

  rand        i.i.d. complex Gaussian, all L M taps: complex, asymmetric, full-band.  Complex filter, general cancellation kernel.
  real_asym   i.i.d. real Gaussian, imaginary parts exactly 0.  Real filter, general cancellation kernel.
  cplx_icsym  a complex filter whose cancellation kernel g = IDFT_M(ic) / M is EXACTLY real and even, so a handle takes the real-symmetric
              rounds (or, created under set_ic_matrix_cores(2) with QPSK decisions, the matrix-core rounds) with a complex filter in front.
              Part 0 is a[m] j^s[m], part L - 1 is b[m] (-j)^s[m], with a and b exactly representable in float32 and exactly even in m
              (a[m] == a[(M - m) % M]) and s[m] drawn from {0, 1, 2, 3}; the parts between are `rand`.  Every tap of the two main parts is
              purely real or purely imaginary, the normalisation scales a[m] and a[M - m] alike, and so the float32 products
              ic[m] = t[m] t[(L - 1) M + m] are exactly (a b)[m]: real, and even in m.  There is no rounding margin to argue about, whatever
              rule the host applies to g.
  imag        1j * rrc: for the known-answer relation f(1j t) = 1j f(t) only.

All are seeded and handed to the constructors UNNORMALISED (the constructors normalise, lib/modulator_kernel_cc.cc:70-85)."""
import functools
import zlib

import numpy as np

import gfdm_ref as R
from gfdm_amd.filters import get_frequency_domain_filter

TOL = 1e-5                     # the project's bound against the float64 oracle (BASELINE north_star)
CROSS = 2e-6                   # two forms of the same sum (the suite's cross-variant tests)
DECISION_GUARD = 1e-4          # as tests/test_parity_gpu.py
IC_ITER = 2
IC_BLOCKS = 8
IC_NOISE = 0.05
H = np.array([1, .5, .1j, .1 + .05j])          # the channel of tests/test_parity_gpu.py
FAMILIES = ("rand", "real_asym", "cplx_icsym")

# route: (M, K, L), B, the kernel_name() every handle must report, and how the handles are created
#   generic: under generic_family_for_testing();  dft_mx: set_dft_matrix_cores while creating
ROUTES = {
    "rowlane_2_per_wave": dict(shape=(5, 32, 2), B=19, kernel="rowlane"),                       # taps preloaded into registers, L M = 10
    "rowlane_k4": dict(shape=(8, 4, 2), B=37, kernel="rowlane"),                                # many blocks per wavefront
    "rowlane_wave": dict(shape=(9, 64, 2), B=11, kernel="rowlane"),                             # the DPP filter path of K = 64, L = 2
    "rowlane_multiwave": dict(shape=(15, 128, 4), B=5, kernel="rowlane"),                       # the only compiled overlap 4: outer parts, taps not preloaded (L M = 60)
    "rowlane_jit_l4": dict(shape=(13, 32, 4), B=21, kernel="rowlane_jit"),                      # overlap 4
    "rowlane_jit_odd": dict(shape=(4, 16, 3), B=37, kernel="rowlane_jit"),                      # odd overlap
    "rowlane_jit_wrap": dict(shape=(5, 4, 8), B=37, kernel="rowlane_jit"),                      # L > K: a row is met twice, with different tap parts
    "rowlane_jit_mixed": dict(shape=(9, 48, 4), B=21, kernel="rowlane_jit"),                    # mixed-radix K
    "generic_lds_12": dict(shape=(7, 12, 2), B=3, kernel="generic_lds", generic=True),
    "generic_odd": dict(shape=(6, 40, 5), B=3, kernel="generic_lds", generic=True),             # odd overlap
    "generic_mx_dft": dict(shape=(33, 20, 2), B=3, kernel="generic_lds", generic=True, dft_mx=2),
    "generic_global": dict(shape=(15, 1040, 2), B=2, kernel="generic_lds"),                     # tiles in global scratch
    "rader_l2": dict(shape=(127, 16, 2), B=5, kernel="generic_rader"),                          # filter in registers
    "rader_l4": dict(shape=(127, 16, 4), B=5, kernel="generic_rader"),
    "rader_l3": dict(shape=(127, 16, 3), B=5, kernel="generic_rader"),                          # run-time filter loop
}
# the odd-overlap shapes on which tests/test_taps.py holds the two oracles against each other
ODD_SHAPES = [(4, 16, 3), (6, 40, 5), (127, 16, 3)]
# seed offsets of the cancellation cases, chosen so that the decision guard keeps at least half of the blocks (tests/test_taps.py asserts it)
IC_SEED = {("rader_l2", "cplx_icsym"): 1}            # (offset 0 keeps 3 of 8 with matched-filter input)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _gauss(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def qpsk(rng, shape):
    return ((1 - 2 * rng.integers(0, 2, shape)) + 1j * (1 - 2 * rng.integers(0, 2, shape))) / np.sqrt(2)


def rrc(M, K, L, alpha=0.4):
    """root-raised-cosine taps, exactly real (the designer's inverse transform leaves imaginary parts of 1e-17)"""
    return get_frequency_domain_filter("rrc", alpha, M, K, L).real.astype(complex)


def make_taps(kind, M, K, L):
    """the unnormalised taps of a family at a shape (complex128, L M)"""
    rng = np.random.default_rng(_seed("taps", kind, M, K, L))
    if kind == "rrc":
        return rrc(M, K, L)
    if kind == "imag":
        return 1j * rrc(M, K, L)
    if kind == "rand":
        return _gauss(rng, M * L)
    if kind == "real_asym":
        return rng.standard_normal(M * L).astype(complex)
    if kind == "cplx_icsym":
        def even():          # float32-exact (multiples of 1/64 in [0.5, 1.5]), exactly even in m
            h = (32 + rng.integers(0, 65, M // 2 + 1)) / 64.0
            v = np.array([h[min(m, M - m)] for m in range(M)])
            assert np.array_equal(v, v.astype(np.float32)) and all(v[m] == v[(M - m) % M] for m in range(M))
            return v
        a, b, s = even(), even(), rng.integers(0, 4, M)
        t = _gauss(rng, M * L)
        t[:M] = a * np.array([1, 1j, -1, -1j])[s]
        t[(L - 1) * M:] = b * np.array([1, -1j, -1, 1j])[s]
        return t
    raise ValueError(kind)


def mutations(nt, M, L):
    """(name, taps) of every wrong tap handling a correct kernel must be told apart from"""
    nt = np.asarray(nt)
    n = M * L
    p = nt.reshape(L, M)

    def parts(order):
        return p[list(order)].reshape(n)
    yield "conj", np.conj(nt)
    yield "mirror", nt[(n - np.arange(n)) % n]
    yield "swap_main", parts([L - 1] + list(range(1, L - 1)) + [0])
    yield "shift1", np.roll(nt, 1)
    if L >= 4:
        yield "swap_outer", parts([0, L - 2] + list(range(2, L - 2)) + [1, L - 1])
        z = p.copy()
        z[1:L - 1] = 0
        yield "zero_outer", z.reshape(n)


def subcarrier_map(K, M):
    """A partial map: the one of tests/test_parity_gpu.py, cut to the max(4, 600 / M) entries around its hole at K / 2.  The guard drops a
    block when ANY decided component of any round is within DECISION_GUARD of zero.  With random taps the components are of unit scale without structure, so that
    happens about once per 1e4 of them: 600 symbols x 2 components x 2 decided stages lose about a fifth of the blocks, the full map of
    K = 1040, M = 15 would lose all of them."""
    if K < 8:
        return np.arange(K)
    full = np.concatenate((np.arange(1, K // 2 - 1), np.arange(K // 2 + 2, K)))
    A, mid = max(4, 600 // M), K // 2 - 2
    return full if len(full) <= A else full[mid - A // 2:mid + A - A // 2]


def per_block_rel(a, b):
    """relative L2 distance of a from b for every block (last axis)"""
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-30)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def make_case(route, kind):
    """inputs of one route with one tap family, and their float64 results; shared between tests, read-only"""
    M, K, L = ROUTES[route]["shape"]
    B = ROUTES[route]["B"]
    return make_shape_case(M, K, L, B, kind)


@functools.lru_cache(maxsize=None)
def make_shape_case(M, K, L, B, kind):
    N = M * K
    rng = np.random.default_rng(_seed("case", M, K, L, B))              # the same data for every family of a shape
    taps = make_taps(kind, M, K, L)
    nt = R.normalize_taps(taps, M)
    sym, gauss = qpsk(rng, (B, N)), _gauss(rng, (B, N))
    x = R.modulate(sym, nt, M, K, L)
    feq = np.fft.fft(H, N)[None, :] * np.exp(0.01j * np.arange(B))[:, None]
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    return _freeze(dict(M=M, K=K, L=L, B=B, N=N, kind=kind, taps=taps, nt=nt, ic=R.ic_filter_taps(nt, M, L), sym=sym, gauss=gauss, x=x, feq=feq, xe=xe))


def guarded(ref_stages, smap, K, M):
    """blocks whose every decided component (all IC iterations) is at least DECISION_GUARD away from zero (tests/test_parity_gpu.py)"""
    keep = None
    for d in [ref_stages["d0"]] + ref_stages["iters"][:-1]:
        v = d.reshape(-1, K, M)[:, smap, :]
        ok = (np.minimum(np.abs(v.real), np.abs(v.imag)).reshape(v.shape[0], -1).min(axis=1) > DECISION_GUARD)
        keep = ok if keep is None else (keep & ok)
    return keep


# the two decision rules: the sign test on the QPSK points, and the nearest-point search on a rotated constellation (as test_parity_gpu.py)
RULES = (("qpsk", "auto", R.qpsk_points()), ("nearest", "nearest", R.qpsk_points() * np.exp(0.1j)))


@functools.lru_cache(maxsize=None)
def make_ic_case(route, kind):
    """IC_BLOCKS noisy blocks on a partial subcarrier map, matched-filter ("mf") and zero-forcing ("zf") input, the float64 result of IC_ITER
    rounds under both decision rules and the blocks the decision guard keeps"""
    M, K, L = ROUTES[route]["shape"]
    N, B = M * K, IC_BLOCKS
    rng = np.random.default_rng(_seed("ic", M, K, L) + IC_SEED.get((route, kind), 0))
    taps = make_taps(kind, M, K, L)
    nt = R.normalize_taps(taps, M)
    smap = subcarrier_map(K, M)
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = qpsk(rng, (B, len(smap), M))
    x = R.modulate(d.reshape(B, N), nt, M, K, L) + IC_NOISE * _gauss(rng, (B, N))
    feq = np.fft.fft(H, N)[None, :] * np.exp(0.01j * np.arange(B))[:, None]
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    c = dict(M=M, K=K, L=L, B=B, N=N, kind=kind, taps=taps, nt=nt, smap=smap, x=x, xe=xe, feq=feq)
    for rule, _, pts in RULES:
        for inp, src, eq in (("mf", x, None), ("zf", xe, feq)):
            ref, st = R.advanced_receive(src, nt, M, K, L, smap, pts, IC_ITER, f_eq=eq, kind=rule, return_stages=True)
            c["ref_%s_%s" % (inp, rule)] = ref
            c["keep_%s_%s" % (inp, rule)] = guarded(st, smap, K, M) if rule == "qpsk" else st["dec_margin"] > DECISION_GUARD
    return _freeze(c)
