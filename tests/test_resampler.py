"""CPU-side checks of the resampler (contract in include/gfdm_hip.h, gfdm_hip_resampler): the entry points are exported and bound, the
argument table answers without a device, there is no CPU fallback, Python-side argument errors come before any device, plan() agrees
with the restatement of tests/resampler_ref.py and with brute-force counting, pieces chained by plan cover a stream exactly once, the
default table has the properties its docstring states, the case table of the GPU tests covers the range the header names, and the
preconditions of the GPU tests hold on the restatements alone."""
import ctypes
import fractions

import numpy as np
import pytest

import resampler_cases as RC
import resampler_ref as Q
from conftest import have_gpu

PLAIN = ("create", "destroy", "n_taps", "n_phases", "interp", "taps", "step", "set_step", "check", "plan")
ONE = 1 << 32


def test_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.capi.exported_symbols())
    for kind in ("host", "device", "sc16_host", "sc16_device"):
        assert "gfdm_hip_resampler_resample_%s" % kind in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_resampler_resample_%s" % kind)
    for name in PLAIN:
        assert "gfdm_hip_resampler_" + name in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_resampler_" + name)
    assert gfdm_amd.Resampler is gfdm_amd.capi.Resampler
    assert gfdm_amd.resampler_step is gfdm_amd.capi.resampler_step and gfdm_amd.resampler_taps is gfdm_amd.capi.resampler_taps


# (n_taps, n_phases, interp, step, n_out, n_in, history, pos) -> what the message names; None = accepted
TABLE = [
    ((1, 1, 0, 1 << 29, 0, 0, 0, 0), None),
    ((64, 128, 1, 1 << 35, 1 << 40, 1 << 40, 63, (1 << 62) - 1), None),
    ((8, 1024, 1, ONE, 1, 1, 0, 0), None),                            # 1025 * 8 = 8200
    ((64, 128, 0, ONE, 1, 1, 0, 0), None),                            # 129 * 64 = 8256: the cap itself
    ((16, 2, 0, 1 << 29, 1, 0, 1 << 59, 0), None),
    ((16, 2, 0, ONE, (1 << 60) - 1, 0, 0, 0), None),                  # 8 n_out just fits
    ((16, 2, 0, 1 << 34, (1 << 60) - (1 << 28) - 1, 0, 0, (1 << 62) - 1), None),      # pos + n_out * step = 2^94 - 2^62 - 2^34 + 2^62 - 1 < 2^94
    ((16, 2, 0, ONE, 0, 1 << 59, (1 << 60) - (1 << 59) - 1, 0), None),                # 8 (history + n_in) just fits
    ((0, 2, 0, ONE, 1, 1, 0, 0), "n_taps"),
    ((65, 2, 0, ONE, 1, 1, 0, 0), "n_taps"),
    ((-1, 2, 0, ONE, 1, 1, 0, 0), "n_taps"),
    ((8, 0, 0, ONE, 1, 1, 0, 0), "n_phases"),
    ((8, 3, 0, ONE, 1, 1, 0, 0), "n_phases"),                          # no power of two
    ((8, 96, 0, ONE, 1, 1, 0, 0), "n_phases"),
    ((4, 2048, 0, ONE, 1, 1, 0, 0), "n_phases"),
    ((8, -4, 0, ONE, 1, 1, 0, 0), "n_phases"),
    ((43, 128, 0, ONE, 1, 1, 0, 0), None),                             # 129 * 43 = 5547
    ((64, 256, 0, ONE, 1, 1, 0, 0), "8256"),
    ((9, 1024, 0, ONE, 1, 1, 0, 0), "8256"),                           # 1025 * 9 = 9225
    ((33, 256, 0, ONE, 1, 1, 0, 0), "8256"),                           # 257 * 33 = 8481
    ((8, 2, 2, ONE, 1, 1, 0, 0), "interp"),
    ((8, 2, -1, ONE, 1, 1, 0, 0), "interp"),
    ((8, 2, 0, (1 << 29) - 1, 1, 1, 0, 0), "step"),
    ((8, 2, 0, (1 << 35) + 1, 1, 1, 0, 0), "step"),
    ((8, 2, 0, 0, 1, 1, 0, 0), "step"),
    ((8, 2, 0, (1 << 64) - 1, 1, 1, 0, 0), "step"),
    ((8, 2, 0, 1 << 29, 1, 1, 0, 0), None),
    ((8, 2, 0, 1 << 35, 1, 1, 0, 0), None),
    ((8, 2, 0, ONE, -1, 1, 0, 0), "n_out"),
    ((8, 2, 0, ONE, 1, -1, 0, 0), "n_in"),
    ((8, 2, 0, ONE, 1, 1, -1, 0), "history"),
    ((8, 2, 0, ONE, 1, 1, 0, -1), "pos"),
    ((8, 2, 0, ONE, 1, 1, 0, 1 << 62), "pos"),
    ((8, 2, 0, ONE, 1 << 60, 1, 0, 0), "overflow"),                    # 8 n_out
    ((8, 2, 0, ONE, 1, 1 << 60, 0, 0), "overflow"),                    # 8 n_in
    ((8, 2, 0, ONE, 1, 1 << 59, 1 << 59, 0), "overflow"),              # 8 (history + n_in)
    ((8, 2, 0, 1 << 35, 1 << 59, 1, 0, 0), "2^94"),                    # n_out * step = 2^94
    ((8, 2, 0, 1 << 35, (1 << 59) - 1, 1, 0, 1 << 35), "2^94"),        # pos + n_out * step = 2^94
    ((8, 2, 0, 1 << 35, (1 << 59) - 1, 1, 0, (1 << 35) - 1), None),    # ... one below
]


def test_cap_table_entry_is_exact():
    assert 129 * 64 == RC.TABLE_CAP and 1025 * 8 <= RC.TABLE_CAP < 257 * 33


@pytest.mark.parametrize("args,names", TABLE)
def test_check_table(args, names):
    import gfdm_amd
    L = gfdm_amd.lib()
    rc = L.gfdm_hip_resampler_check(*args)
    if names is None:
        assert rc == 0, L.gfdm_hip_last_error()
    else:
        assert rc == gfdm_amd.capi.EINVAL and names in L.gfdm_hip_last_error().decode(), (rc, L.gfdm_hip_last_error())


def _create(taps, n_taps, n_phases, interp, step):
    import gfdm_amd
    h = ctypes.c_void_p()
    t = np.ascontiguousarray(taps, np.float32)
    rc = gfdm_amd.lib().gfdm_hip_resampler_create(ctypes.byref(h), t.ctypes.data if t.size else None, n_taps, n_phases, interp, step, 0)
    return rc, h


def test_no_cpu_fallback_and_create_refuses_first():
    """what create can refuse without a device it refuses (EINVAL) whether or not there is one; what it accepts answers ENODEV here"""
    import gfdm_amd
    good = Q.table_for(4, 8)
    for bad in ((good, 8, 3, 0, ONE), (good, 8, 4, 2, ONE), (good, 8, 4, 0, 1), (good, 0, 4, 0, ONE), (good, 64, 256, 0, ONE), (np.zeros(0), 8, 4, 0, ONE)):
        rc, h = _create(*bad)
        assert rc == gfdm_amd.capi.EINVAL and not h.value, bad[1:]
    for value in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[4, 7] = value                                                # the last float of the table
        rc, h = _create(t, 8, 4, 1, ONE)
        assert rc == gfdm_amd.capi.EINVAL and b"finite" in gfdm_amd.lib().gfdm_hip_last_error()
    if have_gpu():
        return
    rc, h = _create(good, 8, 4, 1, ONE)
    assert rc == gfdm_amd.capi.ENODEV and not h.value
    with pytest.raises(gfdm_amd.GfdmHipError) as e:
        gfdm_amd.Resampler(1.0)
    assert e.value.status == gfdm_amd.capi.ENODEV


def test_python_argument_errors_come_before_any_device():
    import gfdm_amd
    with pytest.raises(ValueError, match="interp"):
        gfdm_amd.Resampler(1.0, interp="cubic")
    with pytest.raises(ValueError, match="1/8"):
        gfdm_amd.Resampler(8.5)
    with pytest.raises(ValueError, match="2\\^29"):
        gfdm_amd.Resampler(1)                                          # an int is the Q32.32 step itself
    with pytest.raises(ValueError, match="shape"):
        gfdm_amd.Resampler(1.0, taps=np.ones(16, np.float32))
    with pytest.raises(ValueError, match="n_phases"):
        gfdm_amd.Resampler(1.0, n_phases=100)
    with pytest.raises(ValueError, match="n_taps"):
        gfdm_amd.Resampler(1.0, n_taps=65)
    with pytest.raises(ValueError, match="8256"):
        gfdm_amd.Resampler(1.0, taps=np.zeros((257, 33), np.float32))
    with pytest.raises(ValueError, match="finite"):
        gfdm_amd.Resampler(1.0, taps=np.full((3, 4), np.nan, np.float32))


def test_resampler_step():
    import gfdm_amd
    f = gfdm_amd.resampler_step
    assert f(1.0) == ONE and f(1) == ONE and f(0.125) == 1 << 29 and f(8.0) == 1 << 35
    assert f(fractions.Fraction(4, 5)) == round(fractions.Fraction(4, 5) * ONE) == 3435973837
    assert f(fractions.Fraction(5, 4)) == 5 << 30 and f(1.0001) == round(fractions.Fraction(1.0001) * ONE)
    assert f(fractions.Fraction(2 * ONE + 1, 2 * ONE)) == ONE and f(fractions.Fraction(2 * ONE + 3, 2 * ONE)) == ONE + 2      # ties to even
    for bad in (0.1249, 8.001, -1.0, 0):
        with pytest.raises(ValueError):
            f(bad)


PLAN_STEPS = (1 << 29, ONE - 1, ONE, ONE + 1, 3 << 31, 1 << 35)
PLAN_TS = (1, 2, 8, 63, 64)


@pytest.mark.parametrize("T", PLAN_TS)
def test_plan_against_the_restatement_and_brute_force(T):
    import gfdm_amd
    L = gfdm_amd.lib()
    n_out, adv, nxt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    for step in PLAN_STEPS:
        for pos in RC.POSS:
            for n_in in (0, 1, T - 1, T, 4097):
                for flush in (0, 1):
                    want = Q.plan(step, T, pos, n_in, flush)
                    assert want == Q.plan_brute(step, T, pos, n_in, flush), (step, T, pos, n_in, flush)
                    assert L.gfdm_hip_resampler_plan(step, T, pos, n_in, flush, ctypes.byref(n_out), ctypes.byref(adv), ctypes.byref(nxt)) == 0
                    assert (n_out.value, adv.value, nxt.value) == want, (step, T, pos, n_in, flush)
                    assert 0 <= want[2] < 1 << 62 and 0 <= want[1] <= n_in
    assert L.gfdm_hip_resampler_plan(ONE, T, 0, 10, 1, None, None, None) == 0                   # any result pointer may be NULL
    for bad in ((1, T, 0, 10), (ONE, 65, 0, 10), (ONE, T, -1, 10), (ONE, T, 1 << 62, 10), (ONE, T, 0, -1), (1 << 29, T, 0, 1 << 59)):
        assert L.gfdm_hip_resampler_plan(*bad, 1, ctypes.byref(n_out), ctypes.byref(adv), ctypes.byref(nxt)) == gfdm_amd.capi.EINVAL, bad


@pytest.mark.parametrize("T", PLAN_TS)
def test_chained_pieces_cover_the_stream_exactly_once(T):
    """the outputs of a flushed call on the whole stream, by absolute position, are those of its pieces chained by plan, in order and
    once each -- for two and for many pieces"""
    D = (T - 1) // 2
    for step in PLAN_STEPS:
        for total in (1, 5, 130, 1000):
            for piece in (1, 7, 64, 333):
                whole = [i * step for i in range(Q.plan(step, T, 0, total, True)[0])]
                got, start, pos = [], 0, 0
                for end in list(range(piece, total, piece)) + [total]:             # the stream arrives in chunks that end at `end`
                    last = end == total
                    n_in = end - start                                  # what plan did not advance over is passed again
                    n_out, advance, nxt = Q.plan(step, T, pos, n_in, last)
                    P = [(start << 32) + pos + i * step for i in range(n_out)]
                    for p in P:                                        # the window of every output of a piece lies in the piece and its history
                        assert (p >> 32) >= start and (last or (p >> 32) - D + T - 1 < end)
                    got += P
                    if last:
                        break
                    start, pos = start + advance, nxt
                assert got == whole, (T, step, total, piece)


def test_default_table():
    import gfdm_amd
    for L, T in ((128, 16), (128, 8), (32, 32), (1, 2), (1024, 8), (128, 64), (4, 15)):
        for cutoff in (1.0, 0.8):
            h = gfdm_amd.resampler_taps(L, T, cutoff)
            D = (T - 1) // 2
            assert h.dtype == np.float32 and h.shape == (L + 1, T)
            assert np.array_equal(h[L, 1:], h[0, :-1]) and h[L, 0] == 0                        # row L is row 0 moved by one tap
            if T % 2 == 0:
                assert h[0, T - 1] == 0                                # ... and nothing of row 0 is lost by the move
            gain = h.astype(np.float64).sum(axis=1)
            assert np.all(np.abs(gain[:L] - 1) <= T * 2.0 ** -24), (L, T, cutoff)              # unit DC gain up to the fp32 rounding of T taps
            if cutoff == 1.0:
                assert np.array_equal(h[0], np.eye(T, dtype=np.float32)[D])
    with pytest.raises(ValueError):
        gfdm_amd.resampler_taps(128, 1)
    with pytest.raises(ValueError):
        gfdm_amd.resampler_taps(100, 16)
    with pytest.raises(ValueError):
        gfdm_amd.resampler_taps(128, 16, 1.5)


def test_a_tone_comes_out_as_the_tone_at_f_times_step():
    """the restatement on a complex tone with the default table: the measured error per (T, L, interp) is printed (and recorded in
    profiles/r19); asserted is only that linear is not worse than nearest and that T = 16 is not worse than T = 8"""
    step = round(1.0001 * 2 ** 32)
    err = {}
    for T in (8, 16, 32):
        for L in (32, 128):
            for interp in (0, 1):
                err[T, L, interp] = Q.tone_error(T, L, interp, step)
                print("tone error T %2d L %3d interp %d: %.3e" % (T, L, interp, err[T, L, interp]))
    for T in (8, 16, 32):
        for L in (32, 128):
            assert err[T, L, 1] <= err[T, L, 0]
    for L in (32, 128):
        assert err[16, L, 1] <= err[8, L, 1]
        # with the nearest row the error is that of the row's position, at most half a row = 1 / (2 L) samples of a tone that turns by
        # 2 pi f per sample, whatever T is (measured: 1.0794e-2 at T = 8 against 1.0801e-2 at T = 16 for L = 32, 2.720e-3 against
        # 2.717e-3 for L = 128): T = 16 against T = 8 compares the two filters only where their own error shows, with linear
        for T in (8, 16, 32):
            assert err[T, L, 0] <= 2 * np.pi * 0.11 / (2 * L) + err[T, L, 1]


def test_the_case_table_covers_the_tested_range():
    """every value the header's "tested range" names occurs in tests/resampler_cases.py, every (L, interp) with every T it fits"""
    cs = RC.all_cases()
    assert {c["T"] for c in cs} == set(RC.TS) and {c["n_out"] for c in cs} == set(RC.NS) and {c["step"] for c in cs} == set(RC.STEPS)
    assert {c["pos"] for c in cs} == set(RC.POSS)
    for T in RC.TS:
        mine = [c for c in cs if c["T"] == T]
        assert {(c["L"], c["interp"]) for c in mine} == {(L, i) for L in RC.phases_for(T) for i in (0, 1)}
        assert {c["history"] for c in mine} == set(RC.histories(T))
        assert {(c["fmt"], c["in_shift"]) for c in mine} >= {("c64", 0), ("c64", 1), ("sc16", 0), ("sc16", 1), ("sc16", 2), ("sc16", 3)}
        assert {c["out_shift"] for c in mine} == {0, 1}
        assert {c["step"] for c in mine} == set(RC.STEPS)
        for c in mine:
            assert (c["L"] + 1) * T <= RC.TABLE_CAP and c["pos"] + c["n_out"] * c["step"] < 1 << 94
    assert RC.phases_for(64) == (1, 2, 128) and RC.phases_for(16) == (1, 2, 128) and RC.phases_for(8) == RC.LS
    short = [c for c in cs if ((c["pos"] + (c["n_out"] - 1) * c["step"]) >> 32) - (c["T"] - 1) // 2 + c["T"] - 1 >= c["n_in"]]
    assert len(short) > len(cs) // 2                                   # the zeros behind the end are read


def test_split_preconditions():
    """the pieces of the split-invariance test, by the restatement's plan: together SPLIT_N_OUT outputs, every piece non-empty in input"""
    for T in (1, 8, 16, 64):
        for step in RC.SPLIT_STEPS:
            total, pos = RC.split_start(step)
            assert Q.plan(step, T, pos, total, True)[0] == RC.SPLIT_N_OUT
            for cut in RC.split_cuts(total):
                pieces = RC.chain(step, T, total, cut, pos)
                assert sum(p[4] for p in pieces) == RC.SPLIT_N_OUT and all(p[2] > 0 for p in pieces), (T, step, cut)


def test_exact_arithmetic_preconditions():
    """the inputs of the GPU test on exact arithmetic: integer taps and samples whose partial sums stay below 2^24 in magnitude, and in
    interp 1 a w of few bits, so that every fp32 operation of the contract's chain is exact and float64 gives the same integers"""
    for T, L in RC.EXACT_SHAPES:
        h, x = RC.exact_inputs(T, L)
        assert np.abs(h).max() * np.abs(x.real).max() * T * 1.25 < 2 ** 24
        for interp, step in RC.EXACT_STEPS.items():
            y, _ = Q.resample(x, 0, h, interp, step, 0, 512)
            assert np.array_equal(y, y.astype(np.complex64)) and np.abs(y.real).max() < 2 ** 24
            assert np.array_equal(y.real * 8, np.rint(y.real * 8))


def test_loop_preconditions():
    """what the two loops of tests/test_resampler_gpu.py rely on, on the restatements alone (resampler, channel, detector and both
    receivers in float64), as tests/test_channel_model.py::test_loop_preconditions does for the loop without a resampler: detect finds
    exactly the placed bursts within 1 of round((start + pcp - pos / 2^32) / (step / 2^32)), every maximum of ic is at least 1e-3 from
    the threshold, every decision of the matched-filter receiver and of every round of ZF + 2 IC is at least MARGIN = 0.1 from a
    boundary and equals the transmitted symbol.
    Clock offset (default table, 16 taps, linear, pos = half a sample), measured while writing, threshold / IC / MF margin:
        25 ppm 0.194 / 0.217 / 0.280;  50 ppm 0.194 / 0.181 / 0.244;  100 ppm 0.193 / 0.190 / 0.190;  200 ppm 0.190 / 0.081 / 0.100
    so e = 100 ppm is the largest at which they hold (at 200 ppm the IC margin falls below 0.1): RC.LOOP_PPM.
    Rate change (4/5, channel at the radio's rate, 5/4; complex64 and sc16 between them give the same figures to three digits), EVM of
    the two resamplers alone / threshold / decision margin:
        8 taps 0.131 / 0.184 / 0.155;  16 taps 0.0315 / 0.182 / 0.213;  32 taps 0.0068 / 0.182 / 0.217
    so 8 taps are the smallest at which they hold: RC.LOOP_RATE_NTAPS.  The EVM per n_taps is in profiles/r19/resampler_accuracy.json."""
    held = []
    for ppm in RC.LOOP_PPMS:
        step = RC.loop_step(1 + ppm * 1e-6)
        m = RC.loop_margins(RC.clock_offset_stream(ppm)[0], RC.expected_frame_starts(step, RC.LOOP_POS))
        print("clock offset %3d ppm: found %s right %s threshold margin %.4f, decision margin IC %.3f MF %.3f" % (ppm, m["found"], m["right"], m["thr"], m["ic"], m["mf"]))
        if RC.loop_holds(m):
            held.append(ppm)
    assert held and max(held) == RC.LOOP_PPM
    for fmt in ("c64", "sc16"):
        held = []
        for T in RC.LOOP_NTAPS:
            m = RC.loop_margins(RC.rate_change_stream(T, fmt), RC.expected_frame_starts(ONE, 0))
            print("rate change %s %2d taps: EVM %.4f found %s right %s threshold margin %.4f, decision margin IC %.3f MF %.3f" % (
                fmt, T, RC.rate_change_evm(T), m["found"], m["right"], m["thr"], m["ic"], m["mf"]))
            if RC.loop_holds(m):
                held.append(T)
        assert held and min(held) == RC.LOOP_RATE_NTAPS
    evm = [RC.rate_change_evm(T) for T in RC.LOOP_NTAPS]
    assert evm[0] > evm[1] > evm[2]
