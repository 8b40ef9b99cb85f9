"""Routes, inputs, error figures and bounds for the accuracy tests (tests/test_accuracy.py on the CPU, tests/test_accuracy_gpu.py on the GPU).

The parity tests hold the HIP path to TOL = 1e-5 per-block relative L2 against the float64 oracle.  Float32 arithmetic needs 1e-7 to
4.3e-7 on these sums (the plain-C float32 port of the reference algorithm, oracle/gfdm_oracle.c), so TOL passes taps with 18 mantissa
bits, one output element off by 1e-4 of the block's RMS, and one output position that is worse in every block.  Here the bound of every
figure is the C oracle's own figure ON THE SAME INPUTS times a small margin:

    bound = min(TOL, MARGIN[figure] * figure of the C oracle)

  l2    the worst per-block relative L2 error (conftest.rel_err)
  peak  the largest single |a - b| / rms_b           (rms_b: the RMS of block b of the float64 result)
  pos   over output positions, the largest RMS over blocks of |a - b| / rms_b

MARGIN is 2 for l2 and pos: both sides evaluate the same sums in float32 in another order; a transform with twice the stages, or
Rader's three transforms in place of one, raises the RMS rounding error by at most sqrt 2 to sqrt 3.  It is 3 for peak: the same 2, times
1.5 for the scatter of a maximum over a few thousand values.  No margin is set from what the GPU measured; a route whose kernel provably
performs more roundings than the C oracle may carry margin 2 sqrt(ratio of the counts), at most 4, with the count written next to it
(ROUTES[...]["margin"]; none does).

Inputs.  Symbols, samples and f_eq are rounded to float32 ONCE; the float64 oracle, the C oracle and the GPU all see those values (the
taps likewise: what a constructor receives is complex64).  Taps are root-raised-cosine and tap_cases' family `rand`.  Blocks: 64 + 3
where N <= 1024 (the 3 leave the last workgroup part-filled), 29 above that, 8 for generic_global, 4 for K = 1024.  The cancellation
cases are tap_cases': a partial subcarrier map, noise 0.05, 2 rounds, the decision guard."""
import functools
import zlib

import numpy as np

import gfdm_ref as R
import poison_cases as P
import tap_cases as T

TOL = T.TOL
MARGIN = {"l2": 2.0, "pos": 2.0, "peak": 3.0}
FIGURES = ("l2", "peak", "pos")
REF_L2_CAP = 5e-7              # the C oracle's l2 stays below this on every route's inputs, so no l2 bound rises above 1e-6
KINDS = ("rrc", "rand")
IC_ITER, IC_NOISE, DECISION_GUARD = T.IC_ITER, T.IC_NOISE, T.DECISION_GUARD
H = T.H
PLAIN = ("modulate", "fd", "fdeq", "demodulate", "demodulate_equalize", "to_td", "cancel")
IC = ("ic_mf", "ic_zf")
SCALES = (0, -40, 15, 40)      # block b of a mixed-scale launch is multiplied by 2^SCALES[b % 4] (+15: the amplitude of an int16 capture)
JOINT = (-20, 15)              # x and f_eq (block and rx preamble) both times 2^k


def _blocks(M, K, name):
    return 8 if name == "generic_global" else 4 if K == 1024 else 67 if M * K <= 1024 else 29


def _routes():
    r = {}
    # the fifteen routes of the tap tests; the cancellation rounds on the vector ALU (set_ic_matrix_cores(0))
    for name, d in T.ROUTES.items():
        r[name] = dict(d, ic_mx=0)
    # the two forced matrix-core forms of the cancellation rounds (the form needs a real even kernel: RRC taps only)
    for name in ("rowlane_2_per_wave_ic_mx", "rowlane_wave_ic_mx"):
        d = P.ROUTES[name]
        r[name] = dict(shape=d["shape"], kernel=d["kernel"], ic_mx=2, kinds=("rrc",), entries=IC)
    # where the number of roundings per output is largest, each the smallest shape of its kind
    r["deep_three_wide_passes"] = dict(shape=(9, 200, 2), kernel="rowlane_jit", ic_mx=0)
    r["deep_butterfly_31"] = dict(shape=(9, 31, 2), kernel="rowlane_jit", ic_mx=0)
    r["deep_prime_timeslots_37"] = dict(shape=(37, 32, 2), kernel="rowlane_jit", ic_mx=0)
    r["deep_rowlane_1024"] = dict(shape=(15, 1024, 2), kernel="rowlane_jit", ic_mx=0)
    # the generic family on the tuned shapes (generic_family_for_testing)
    for K, M, L in ((32, 5, 2), (64, 9, 2), (128, 15, 4), (256, 31, 2)):
        r["generic_tuned_%d" % K] = dict(shape=(M, K, L), kernel="generic_lds", generic=True, ic_mx=0)
    for name, d in r.items():
        M, K, _ = d["shape"]
        d["B"] = _blocks(M, K, name)
        d.setdefault("kinds", KINDS)
        d.setdefault("entries", PLAIN + IC)
        d.setdefault("margin", MARGIN)
    return r


ROUTES = _routes()
CASES = [(route, kind) for route in sorted(ROUTES) for kind in ROUTES[route]["kinds"]]
# seed offsets of the cancellation cases, chosen so that the decision guard keeps at least half of the blocks (tests/test_accuracy.py asserts it)
IC_SEED = {}
# Cutting the normalised taps to 18 mantissa bits moves a table of many taps of equal weight by 2^-18 / sqrt 12 = 1.1e-6 (the common part
# of the cut goes when the constructor normalises again).  The figures are always computed and held against the case's own bounds; the one
# case listed here stays inside them: with RRC taps at M = 5, K = 4, L = 8 three taps of one binade (0.714, 0.702, 0.662) carry the filter,
# the cut moves them alike, and the normalised table ends up about 1e-7 from the uncut one, below the reference's own error.  The test
# asserts that it does stay inside (so the entry goes when it no longer does); the `rand` taps of the same route are caught.
CUT_STAYS_INSIDE = {("rowlane_jit_wrap", "rrc")}
# Routes whose blocks are shorter than 100 samples: l2, a maximum over blocks, scatters by tens of percent between seeds there
SHORT_BLOCKS = {r for r, d in ROUTES.items() if d["shape"][0] * d["shape"][1] < 100}
# Transmitter.transmit against COracleTx: one row-lane, one run-time instantiated and one generic route
TX_ROUTES = ("rowlane_wave", "rowlane_jit_mixed", "generic_lds_12")
TX_CP, TX_CS, TX_RAMP, TX_SHIFTS, TX_PRE = 5, 3, 2, (0, 2), 11


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def c64(a):
    """rounded to float32 once, handed on as complex128: the oracles and the GPU get the same values"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def figures(a, b):
    """dict(l2, peak, pos) of the result a against the float64 result b, both (B, n)"""
    b = np.asarray(b)
    a = np.asarray(a).reshape(b.shape)
    rms = np.sqrt(np.mean(np.abs(b) ** 2, axis=-1))
    d = np.abs(a - b) / np.maximum(rms, 1e-300)[:, None]
    return dict(l2=float(np.sqrt(np.mean(d ** 2, axis=-1)).max()), peak=float(d.max()), pos=float(np.sqrt(np.mean(d ** 2, axis=0)).max()))


def where(a, b):
    """where the figures of a against b sit: (block, position) of the peak, and the position of pos"""
    b = np.asarray(b)
    a = np.asarray(a).reshape(b.shape)
    d = np.abs(a - b) / np.sqrt(np.mean(np.abs(b) ** 2, axis=-1))[:, None]
    blk, at = np.unravel_index(int(np.argmax(d)), d.shape)
    return "peak at block %d position %d, pos at position %d, l2 in block %d" % (blk, at, int(np.argmax(np.mean(d ** 2, axis=0))), int(np.argmax(np.mean(d ** 2, axis=-1))))


def bounds(ref_figs, margin=MARGIN):
    """the bound of every figure from the C oracle's figures on the same inputs"""
    return {f: min(TOL, margin[f] * ref_figs[f]) for f in FIGURES}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def make_case(route, kind, seed=0):
    """inputs of one route with one tap family (all exactly representable in float32), the float64 result of every entry point on
    them, and the cancellation case with its guard; shared between tests, read-only"""
    r = ROUTES[route]
    return make_shape_case(route, r["shape"], r["B"], kind, seed, IC_SEED.get((route, kind), 0))


@functools.lru_cache(maxsize=None)
def make_shape_case(route, shape, B, kind, seed=0, ic_seed=0, ic=True):
    """make_case for any shape (tests/codelet_cases.py has its own list); ic=False leaves the cancellation case out"""
    M, K, L = shape
    N = M * K
    rng = np.random.default_rng(_seed("accuracy", M, K, L, B, seed))
    taps = c64(T.make_taps(kind, M, K, L))
    nt = R.normalize_taps(taps, M)
    sym = c64(T.qpsk(rng, (B, N)))
    x = c64(R.modulate(sym, nt, M, K, L))
    feq = c64(np.fft.fft(H, N)[None, :] * np.exp(0.01j * np.arange(B))[:, None])
    xe = c64(np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1))
    S = c64(R.fft_filter_downsample(x, nt, M, K, L))
    smap = T.subcarrier_map(K, M)
    c = dict(route=route, M=M, K=K, L=L, B=B, N=N, kind=kind, taps=taps, nt=nt, sym=sym, x=x, feq=feq, xe=xe, S=S, smap=smap)
    c["ref_modulate"] = R.modulate(sym, nt, M, K, L)
    c["ref_fd"] = R.fft_filter_downsample(x, nt, M, K, L)
    c["ref_fdeq"] = R.fft_filter_downsample(xe, nt, M, K, L, feq)
    c["ref_demodulate"] = R.demodulate(x, nt, M, K, L)
    c["ref_demodulate_equalize"] = R.demodulate(xe, nt, M, K, L, feq)
    c["ref_to_td"] = R.transform_subcarriers_to_td(S, M, K)
    if not ic:
        return _freeze(c)
    ict = R.ic_filter_taps(nt, M, L)
    c["ref_cancel"] = R.cancel_sc_interference(sym, S, ict, M, K)
    # the cancellation case: a partial map, noisy blocks, matched-filter and zero-forcing input, QPSK sign decisions
    rng = np.random.default_rng(_seed("accuracy_ic", M, K, L, B, seed) + ic_seed)
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = T.qpsk(rng, (B, len(smap), M))
    xi = c64(R.modulate(d.reshape(B, N), nt, M, K, L) + IC_NOISE * T._gauss(rng, (B, N)))
    xie = c64(np.fft.ifft(np.fft.fft(xi, axis=-1) * feq, axis=-1))
    c.update(ic_x=xi, ic_xe=xie)
    for inp, src, eq in (("mf", xi, None), ("zf", xie, feq)):
        ref, st = R.advanced_receive(src, nt, M, K, L, smap, R.qpsk_points(), IC_ITER, f_eq=eq, kind="qpsk", return_stages=True)
        c["ref_ic_" + inp] = ref
        c["keep_ic_" + inp] = T.guarded(st, smap, K, M)
    return _freeze(c)


def keep(c, entry):
    """the blocks of an entry point that are compared: all, or those the decision guard keeps"""
    return c["keep_" + entry] if entry in IC else np.ones(c["B"], bool)


class Handles:
    """The calls of the accuracy tests on one set of handles with the interface of gfdm_amd.Modulator / Demodulator / AdvancedReceiver:
    the C oracle (oracle_handles) and the GPU see the same calls."""

    def __init__(self, mod, dem, adv):
        self.mod, self.dem, self.adv = mod, dem, adv

    def run(self, entry, c, sx=None, sf=None):
        """one call of `entry` on the case's inputs; sx scales the samples or symbols per block, sf the equaliser (None: unscaled)"""
        one = np.ones((c["B"], 1))
        sx = one if sx is None else np.asarray(sx).reshape(-1, 1)
        sf = one if sf is None else np.asarray(sf).reshape(-1, 1)
        mod, dem, adv = self.mod, self.dem, self.adv
        if entry == "modulate":
            return mod.modulate(c["sym"] * sx)
        if entry == "fd":
            return dem.fft_filter_downsample(c["x"] * sx)
        if entry == "fdeq":
            return dem.fft_equalize_filter_downsample(c["xe"] * sx, c["feq"] * sf)
        if entry == "demodulate":
            return dem.demodulate(c["x"] * sx)
        if entry == "demodulate_equalize":
            return dem.demodulate_equalize(c["xe"] * sx, c["feq"] * sf)
        if entry == "to_td":
            return dem.transform_subcarriers_to_td(c["S"] * sx)
        if entry == "cancel":
            return dem.cancel_sc_interference(c["sym"] * sx, c["S"] * sx)
        if entry == "ic_mf":
            return adv.demodulate(c["ic_x"] * sx)
        if entry == "ic_zf":
            return adv.demodulate_equalize(c["ic_xe"] * sx, c["feq"] * sf)
        raise ValueError(entry)

    def figures(self, entry, c):
        """(figures, the result on the compared blocks, the float64 result on them)"""
        k = keep(c, entry)
        got, ref = np.asarray(self.run(entry, c)).reshape(c["B"], -1)[k], c["ref_" + entry][k]
        return figures(got, ref), got, ref


class _OracleReceiver:
    def __init__(self, o):
        self.o = o
        self.modulate, self.demodulate, self.fft_filter_downsample = o.modulate, o.demodulate, o.fft_filter_downsample
        self.transform_subcarriers_to_td, self.cancel_sc_interference = o.transform_subcarriers_to_td, o.cancel_sc_interference

    def demodulate_equalize(self, x, f_eq):
        return self.o.demodulate(x, f_eq)

    def fft_equalize_filter_downsample(self, x, f_eq):
        return self.o.fft_filter_downsample(x, f_eq)


class _OracleAdvanced:
    def __init__(self, o, smap):
        self.o, self.smap = o, smap

    def demodulate(self, x):
        return self.o.advanced_receive(x, self.smap, R.qpsk_points(), IC_ITER, kind="qpsk")

    def demodulate_equalize(self, x, f_eq):
        return self.o.advanced_receive(x, self.smap, R.qpsk_points(), IC_ITER, f_eq=f_eq, kind="qpsk")


def oracle_handles(c, taps=None):
    """the plain-C float32 oracle behind the interface of the GPU handles (taps: in place of the case's, for the tap mutation)"""
    import c_oracle
    o = _OracleReceiver(c_oracle.COracle(c["M"], c["K"], c["L"], c["taps"] if taps is None else taps))
    return Handles(o, o, _OracleAdvanced(o.o, c["smap"]))


@functools.lru_cache(maxsize=None)
def reference_figures(route, kind, seed=0):
    """{entry: figures of the C oracle on the case's inputs}: what float32 arithmetic needs on these sums"""
    return case_reference_figures(make_case(route, kind, seed), ROUTES[route]["entries"])


def case_reference_figures(c, entries):
    h = oracle_handles(c)
    return {e: h.figures(e, c)[0] for e in entries}


# ---------------------------------------------------------------- mutations: what TOL lets through and the bounds must not

def chop_mantissa(a, bits=18):
    """float32 values cut to `bits` mantissa bits (the implicit one not counted), as from a table stored or split too coarsely"""
    a = np.ascontiguousarray(a, dtype=np.complex64).copy()
    w = a.view(np.uint32)
    w &= np.uint32(0xFFFFFFFF ^ ((1 << (23 - bits)) - 1))
    return a.astype(np.complex128)


def off_one_element(got, ref, rel=1e-4):
    """the last element of the last block wrong by rel times the block's RMS"""
    out = np.array(got, dtype=np.complex128)
    out[-1, -1] += rel * np.sqrt(np.mean(np.abs(ref[-1]) ** 2))
    return out


def off_one_position(got, ref, rel=1e-6, position=1, seed=0):
    """one output position wrong by rel times the block's RMS, with another phase in every block (one wrong twiddle literal, one lane on
    a cheaper path)"""
    out = np.array(got, dtype=np.complex128)
    rng = np.random.default_rng(_seed("phase", seed))
    out[:, position] += rel * np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1)) * np.exp(2j * np.pi * rng.random(out.shape[0]))
    return out


# ---------------------------------------------------------------- exact power-of-two homogeneity

def times(a, s):
    """the complex64 blocks a (B, n) times the real factor s[b] of their block, component by component (a complex product with s + 0j can
    turn a -0.0 into +0.0)"""
    a = np.ascontiguousarray(a, dtype=np.complex64)
    a = a.reshape(len(s), -1)
    return (a.view(np.float32) * np.asarray(s, dtype=np.float32)[:, None]).view(np.complex64)


def block_scales(B):
    """2^k per block, k cycling through SCALES: exact in float32, and nothing over- or underflows on data of unit scale"""
    return np.ldexp(1.0, np.array(SCALES)[np.arange(B) % len(SCALES)])


# ---------------------------------------------------------------- transmitter

@functools.lru_cache(maxsize=None)
def make_tx_case(route, kind="rand"):
    """Transmitter.transmit with a partial map, cyclic prefix, suffix, ramp, two cyclic shifts and a preamble: arguments (float32-exact) and
    the float64 frames of every port"""
    r = ROUTES[route]
    (M, K, L), B = r["shape"], r["B"]
    N = M * K
    rng = np.random.default_rng(_seed("accuracy_tx", M, K, L, B))
    taps = c64(T.make_taps(kind, M, K, L))
    nt = R.normalize_taps(taps, M)
    smap = P.subcarrier_map(K)
    A = len(smap)
    window = c64(np.concatenate((np.linspace(0.1, 0.9, TX_RAMP), np.ones(N + TX_CP + TX_CS - 2 * TX_RAMP), np.linspace(0.9, 0.1, TX_RAMP))))
    pre = [c64(T._gauss(rng, TX_PRE)) for _ in TX_SHIFTS]
    sym = c64(T.qpsk(rng, (B, A * M)))
    refs = [R.transmit(sym, nt, M, K, L, smap, True, TX_CP, TX_CS, TX_RAMP, window, s, p) for s, p in zip(TX_SHIFTS, pre)]
    return _freeze(dict(route=route, M=M, K=K, L=L, B=B, N=N, A=A, taps=taps, nt=nt, smap=smap, window=window, pre=pre, sym=sym, refs=refs))


def tx_args(c):
    """the constructor arguments COracleTx and gfdm_amd.Transmitter share"""
    return (c["M"], c["K"], c["A"], TX_CP, TX_CS, TX_RAMP, c["smap"], True, c["L"], c["taps"], c["window"], list(TX_SHIFTS), c["pre"])


# ---------------------------------------------------------------- estimator (homogeneity only: the C oracle has no estimator)

def active(K):
    A = 2 * ((3 * K // 4) // 2)
    return A, np.concatenate((np.arange(1, 1 + A // 2), np.arange(K - A // 2, K)))


@functools.lru_cache(maxsize=None)
def estimator_inputs(K, B):
    """a known preamble (flat spectrum, two identical halves) and every block's received preamble behind the channel H, float32-exact"""
    rng = np.random.default_rng(_seed("accuracy_est", K, B))
    pre = np.tile(np.fft.ifft(np.exp(2j * np.pi * rng.random(K))) * np.sqrt(K), 2)
    gains = np.exp(0.3j * np.arange(B)) * (1 + 0.02 * np.arange(B))
    rx = np.tile(np.fft.ifft(np.fft.fft(pre[:K]) * np.fft.fft(H, K)), 2)[None, :] * gains[:, None]
    pre, rx = c64(pre), c64(rx + 1e-3 * T._gauss(rng, (B, 2 * K)))
    pre.setflags(write=False)
    rx.setflags(write=False)
    return pre, rx
