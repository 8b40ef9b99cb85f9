"""The case table of the resampler's GPU tests (tests/test_resampler_gpu.py) and what tests/test_resampler.py checks of it on the CPU:
every value the contract's "tested range" names occurs, going round with the case number."""
import fractions
import functools
import itertools

import numpy as np

import resampler_ref as Q

TS = (1, 2, 3, 8, 16, 64)
LS = (1, 2, 128, 1024)
NS = (1, 2, 3, 255, 256, 257, 4097, 65539)
STEPS = (1 << 29, 1 << 32, (1 << 32) + 1, round(1.0001 * 2 ** 32), 3 << 31, 1 << 35)
POSS = tuple((ip << 32) + fr for ip in (0, 5) for fr in (0, 1 << 31, (1 << 32) - 1))
SHORT = (0, 1, 3)                     # samples by which n_in ends before the last output's own sample idx
TABLE_CAP = 8256
PER_N = 3                             # cases per n_out


def phases_for(T):
    return tuple(L for L in LS if (L + 1) * T <= TABLE_CAP)


def histories(T):
    D = (T - 1) // 2
    return (0, 1, max(D - 1, 0), D, D + 5)


@functools.lru_cache(maxsize=None)
def cases(T):
    """the cases of one T: every n_out three times, and going round with the case number every (L, interp), step, pos, history, every
    alignment of the input (two of complex64, four of sc16) and of the output, an n_in that ends at, one and three samples before the
    last output's own sample -- so that its window, and with 1 and 3 the sample itself, reads the zeros behind the end"""
    combos = list(itertools.product(phases_for(T), (0, 1)))
    out = []
    for k, n_out in enumerate(NS):
        for j in range(PER_N):
            c = PER_N * k + j + TS.index(T)
            L, interp = combos[c % len(combos)]
            fmt = "sc16" if (k + j) % 2 else "c64"
            step, pos = STEPS[(c + c // len(combos)) % 6], POSS[(c + c // 6 + j) % 6]
            last = (pos + (n_out - 1) * step) >> 32
            out.append(dict(T=T, L=L, interp=interp, n_out=n_out, step=step, pos=pos, history=histories(T)[(c + c // 5) % 5],
                            n_in=max(last + 1 - SHORT[c % 3], 0), in_shift=(c // 2) % (4 if fmt == "sc16" else 2), out_shift=(c // 4 + j) % 2, fmt=fmt,
                            seed=100 * T + c))
    return out


def all_cases():
    return list(itertools.chain.from_iterable(cases(T) for T in TS))


@functools.lru_cache(maxsize=None)
def case_data(T, idx):
    """inputs and float64 expectation of case idx of T: x (history + n_in samples: complex64, or int16 pairs with xw their widening), the
    table, y, budget"""
    c = dict(cases(T)[idx])
    n = c["history"] + c["n_in"]
    if c["fmt"] == "sc16":
        c["x"] = Q.signal_sc16(c["seed"], n)
        c["xw"] = Q.widen(c["x"])
    else:
        c["x"] = c["xw"] = Q.signal(c["seed"], n)
    c["taps"] = Q.table_for(c["L"], T)
    c["y"], c["budget"] = Q.resample(c["xw"], c["history"], c["taps"], c["interp"], c["step"], c["pos"], c["n_out"])
    return c


def tag(c):
    return "T %d L %d interp %d n_out %d step %d pos %d history %d n_in %d %s in+%d out+%d" % (
        c["T"], c["L"], c["interp"], c["n_out"], c["step"], c["pos"], c["history"], c["n_in"], c["fmt"], c["in_shift"], c["out_shift"])


# ---- split invariance: one flushed call of 4097 outputs against its pieces ----
SPLIT_N_OUT = 4097
SPLIT_CUTS = (1, 2, 255, 1000)
SPLIT_STEPS = ((1 << 32) + 1, 3 << 31, 1 << 29)


def split_start(step):
    """(n_in, pos): the shortest input that holds output SPLIT_N_OUT - 1 from pos 0, and the pos >= 0 from which its flushed plan gives
    exactly SPLIT_N_OUT outputs (0 unless step < 2^32 puts several outputs behind that one)"""
    n_in = (((SPLIT_N_OUT - 1) * step) >> 32) + 1
    return n_in, max((n_in << 32) - SPLIT_N_OUT * step, 0)


def split_cuts(n_total):
    """SPLIT_CUTS inside a stream of n_total samples: at step 2^29 the 4097 outputs need 513 samples only, and the cut at 1000 becomes
    one at the last sample"""
    return sorted({min(cut, n_total - 1) for cut in SPLIT_CUTS})


def chain(step, T, n_total, cut, pos=0):
    """the pieces of a stream of n_total samples cut at `cut`: [(first sample of the piece, history, n_in, pos, n_out)], by plan"""
    D = (T - 1) // 2
    pieces, start = [], 0
    for end, flush in ((cut, False), (n_total, True)):
        n_in = end - start
        n_out, advance, nxt = Q.plan(step, T, pos, n_in, flush)
        pieces.append((start, min(D, start), n_in, pos, n_out))
        start, pos = start + advance, nxt
    return pieces


# ---- exact arithmetic: integer taps and samples whose partial sums stay below 2^24 ----
EXACT_SHAPES = ((2, 4), (8, 4), (16, 4), (64, 4))                     # (T, L)
EXACT_STEPS = {0: (1 << 32) + (1 << 30), 1: (1 << 32) + (1 << 27)}    # frac a multiple of 2^30: rows hit exactly; of 2^27: w a multiple of 1/8


def exact_inputs(T, L):
    """(table, x): taps that are multiples of 8 in -64 .. 64 (a w of three bits keeps c an integer), samples with integer components in
    -64 .. 64: every product and partial sum is an integer below 2^24, so the fp32 chain is exact"""
    rng = np.random.default_rng(T)
    h = rng.integers(-8, 9, (L + 1, T)).astype(np.float32) * 8.0
    h[L, 1:] = h[0, :-1]
    h[L, 0] = 0
    x = (rng.integers(-64, 65, 2048) + 1j * rng.integers(-64, 65, 2048)).astype(np.complex64)
    return h, x


# ---- the two loops: burst_shaper_ref.loop_case() through the channel constants of channel_model_ref, with a resampler in the chain ----
LOOP_PPMS = (25, 50, 100, 200)                    # candidates for the clock offset e; the largest at which the margins hold is used
LOOP_POS = 1 << 31                                # half a sample of static offset
LOOP_NTAPS = (8, 16, 32)                          # candidates for the rate-change loop; the smallest at which the margins hold is used
LOOP_UP, LOOP_DOWN = fractions.Fraction(4, 5), fractions.Fraction(5, 4)       # the radio runs at 5/4 of the GFDM rate
LOOP_PPM = 100                                    # chosen by tests/test_resampler.py::test_loop_preconditions, which asserts the choice
LOOP_RATE_NTAPS = 8                               # likewise


def loop_step(rate):
    import gfdm_amd
    return gfdm_amd.resampler_step(rate)


def default_taps(step, n_taps, n_phases=128):
    """the table Resampler(step, n_phases=.., n_taps=..) builds: cutoff min(1, 2^32 / step)"""
    import gfdm_amd
    return gfdm_amd.resampler_taps(n_phases, n_taps, min(1.0, float(1 << 32) / step))


def restated(x, step, pos, n_taps):
    """the flushed call Resampler(step, n_taps=n_taps).resample(x, pos=pos) by the restatement, rounded to complex64 -> (y, y64, budget)"""
    n_out = Q.plan(step, n_taps, pos, np.asarray(x).size, True)[0]
    y, budget = Q.resample(x, 0, default_taps(step, n_taps), 1, step, pos, n_out)
    return y.astype(np.complex64), y, budget


@functools.lru_cache(maxsize=None)
def clock_offset_stream(ppm):
    """(s, y, budget): the placed loop stream resampled at 1 + ppm 1e-6 from half a sample in (default table, 16 taps, linear), then the
    channel of channel_model_ref; s is the capture as complex64"""
    import channel_model_ref as C
    x = C.loop_stream()[0]
    z = restated(x, loop_step(1 + ppm * 1e-6), LOOP_POS, 16)[0]
    y, budget = C.apply(z, 0, C.LOOP_TAPS, C.LOOP_F, C.LOOP_NOISE_VOLTAGE, C.LOOP_SEED, 0)
    return y.astype(np.complex64), y, budget


@functools.lru_cache(maxsize=None)
def rate_change_stream(n_taps, fmt):
    """the capture of the rate-change loop at the GFDM rate: placed stream -> 4/5 -> channel (complex64, or sc16 at LOOP_GAIN) -> 5/4"""
    import channel_model_ref as C
    import gfdm_amd
    x = C.loop_stream()[0]
    up = restated(x, loop_step(LOOP_UP), 0, n_taps)[0]
    y, budget = C.apply(up, 0, C.LOOP_TAPS, C.LOOP_F, C.LOOP_NOISE_VOLTAGE, C.LOOP_SEED, 0)
    radio = y.astype(np.complex64) if fmt == "c64" else gfdm_amd.from_sc16(C.sc16(y, budget, C.LOOP_GAIN)[0])
    return restated(radio, loop_step(LOOP_DOWN), 0, n_taps)[0]


@functools.lru_cache(maxsize=None)
def rate_change_evm(n_taps):
    """the error-vector magnitude of 4/5 then 5/4 alone (no channel) on the placed stream, relative to its RMS over the frames"""
    import channel_model_ref as C
    x = C.loop_stream()[0]
    back = restated(restated(x, loop_step(LOOP_UP), 0, n_taps)[0], loop_step(LOOP_DOWN), 0, n_taps)[0]
    n = min(x.size, back.size)
    live = x[:n] != 0
    return float(np.sqrt(np.mean(np.abs(back[:n][live].astype(np.complex128) - x[:n][live]) ** 2) / np.mean(np.abs(x[:n][live]) ** 2)))


def expected_frame_starts(step, pos):
    """where detect should find the bursts behind a resampler: round((start + pcp - pos / 2^32) / (step / 2^32))"""
    import burst_shaper_ref as B
    c = B.loop_case()
    return np.array([round(fractions.Fraction((int(st) + c["pcp"]) * (1 << 32) - pos, step)) for st in c["starts"]], np.int64)


def loop_margins(s, want_starts):
    """what the loops rely on, on the float64 restatements of detect and of both receivers: dict(found, thr, ic, mf, right)"""
    import burst_shaper_ref as B
    import gfdm_ref as R
    from burst_detect_ref import nms_maxima, ref_detect
    from burst_receive_cases import restatement, virtual_bursts
    c = B.loop_case()
    d = ref_detect(s, c["preamble"], c["K"], c["pcp"], c["window_len"], B.LOOP_THRESHOLD, c["min_distance"], c["lead"])
    fs = np.asarray(d["frame_start"], np.int64)
    found = fs.size == c["nb"] and bool(np.all(np.abs(fs - want_starts) <= 1))
    out = dict(found=found, thr=0.0, ic=0.0, mf=0.0, right=False, frame_start=fs)
    if not found:
        return out
    maxima = nms_maxima(d["ic"], c["min_distance"])
    out["thr"] = float(np.min(np.abs(d["ic"][maxima] - B.LOOP_THRESHOLD)))
    e = virtual_bursts(s, d["frame_start"], d["sc_rot"], 0, c["F"])
    ic, out["ic"] = restatement(c, e, 2)
    mf, _ = restatement(c, e, None)
    out["mf"] = float(np.min(R.decision_margin(mf, R.qpsk_points(), "qpsk")))
    out["right"] = all(np.array_equal(o.real > 0, c["sym"].real > 0) and np.array_equal(o.imag > 0, c["sym"].imag > 0) for o in (ic, mf))
    return out


def loop_holds(m):
    from burst_receive_cases import MARGIN
    return m["found"] and m["right"] and m["thr"] >= 1e-3 and m["ic"] >= MARGIN and m["mf"] >= MARGIN
