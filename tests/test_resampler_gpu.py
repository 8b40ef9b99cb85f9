"""GPU tests of the resampler (contract in include/gfdm_hip.h, gfdm_hip_resampler).  The yardstick is the restatement of
tests/resampler_ref.py (Python integers for the positions, float64 for the sum, on the same fp32 table and samples), never the code
under test, and the bound is the contract's error budget
    |y - y64| <= (T + 4) 2^-23 S_i,        S_i = sum_t |c[t]| |x[idx - D + t]|,
derived there from the operations, not from what the kernel gives; every test prints the worst share of it that it saw.  Every output
lies between guard words."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import gfdm_ref as R
import resampler_cases as RC
import resampler_ref as Q
import symbol_mapper_ref as S
from conftest import have_gpu, rel_err

pytestmark = pytest.mark.gpu
GUARD = 16                                  # guard elements on either side of a buffer: a multiple of 16 bytes for both dtypes
FILL = {"int16": 0x5A5A, "complex64": 7 + 7j}
ONE = 1 << 32


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.complex64 else np.uint16)


class Window:
    """n samples (complex64, or sc16 as int16 pairs) inside a larger device buffer, `shift` samples past a 16-byte boundary, guard words on
    either side"""

    def __init__(self, n, shift, sc16=False, content=None):
        import torch
        self.per = 2 if sc16 else 1
        self.lo, self.n = (GUARD + shift) * self.per, n * self.per
        name = "int16" if sc16 else "complex64"
        self.buf = torch.full((self.lo + self.n + GUARD * self.per,), FILL[name], dtype=getattr(torch, name), device="cuda:0")
        self.view = self.buf[self.lo:self.lo + self.n]
        self.fill = _h(self.buf[:1]).copy()
        assert self.view.is_contiguous() and (not n or self.view.data_ptr() % 16 == (shift * (4 if sc16 else 8)) % 16)
        if content is not None and self.n:
            self.view.copy_(_t(np.ascontiguousarray(content).ravel()))

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.fill) and np.all(b[self.lo + self.n:] == self.fill), "guard words overwritten"
        got = b[self.lo:self.lo + self.n]
        return got.reshape(-1, 2) if self.per == 2 else got


def _check(got, y, budget, tag):
    assert got.dtype == np.complex64 and got.shape == y.shape
    share = Q.share_of_budget(got, y, budget)
    print("%s: worst error %.3f of the budget" % (tag, share))
    assert share <= 1.0, (tag, share)
    return share


def _rs(c, **kw):
    import gfdm_amd
    return gfdm_amd.Resampler(kw.get("step", c["step"]), c["taps"], interp="linear" if c["interp"] else "nearest")


@pytest.mark.parametrize("T", RC.TS)
def test_every_shape(T):
    """the case table of tests/resampler_cases.py for one T: every n_out from 1 to 65539, every (L, interp) that fits, every step, pos and
    kind of history, an n_in that ends before the last windows do, input and output at every alignment of one element, complex64 and
    sc16 in"""
    worst = 0.0
    for idx in range(len(RC.cases(T))):
        c = RC.case_data(T, idx)
        sc16 = c["fmt"] == "sc16"
        x = Window(c["history"] + c["n_in"], c["in_shift"], sc16, content=c["x"])
        w = Window(c["n_out"], c["out_shift"])
        res = _rs(c).resample(x.view, c["history"], c["pos"], n_out=c["n_out"], out=w.view)
        assert res is w.view
        worst = max(worst, _check(w.result(), c["y"], c["budget"], RC.tag(c)))
        assert np.array_equal(_bits(x.result()), _bits(c["x"]))                 # the input is left alone
    print("T %d: worst share of the budget %.3f" % (T, worst))


def test_unit_tap_is_a_bit_copy():
    """T = 1, h = 1, step = 2^32, pos = 0: the output is the input, bit for bit -- signed zeros, infinities and denormals included"""
    import gfdm_amd
    x = Q.signal(5, 4099)
    x[:8] = np.array([0, -0.0, complex(-0.0, 0.0), complex(np.inf, -1), complex(1e-42, -1e-42), complex(-np.inf, np.inf), 3e38, -1e-45], np.complex64)
    for interp in ("nearest", "linear"):
        for L in (1, 128):
            rs = gfdm_amd.Resampler(ONE, np.ones((L + 1, 1), np.float32), interp=interp)
            for shift in (0, 1):
                w = Window(x.size, shift)
                rs.resample(_t(x), out=w.view)
                assert np.array_equal(_bits(w.result()), _bits(x)), (interp, L, shift)
            w = Window(x.size - 3, 1)
            rs.resample(_t(x), history=3, out=w.view)
            assert np.array_equal(_bits(w.result()), _bits(x[3:]))


@pytest.mark.parametrize("T", [2, 8, 16, 63, 64])
def test_default_table_copies_at_unit_step(T):
    """the default table, step = 2^32, pos = 0: row 0 is the unit impulse at tap D, so finite (non-zero) input is copied bit for bit"""
    import gfdm_amd
    x = Q.signal(6 + T, 4099)
    assert np.all(x.real != 0) and np.all(x.imag != 0)
    for interp in ("nearest", "linear"):
        rs = gfdm_amd.Resampler(1.0, n_phases=128, n_taps=T, interp=interp)
        got = _h(rs.resample(_t(x)))
        assert got.shape == x.shape and np.array_equal(_bits(got), _bits(x)), (T, interp)


@pytest.mark.parametrize("T,L", RC.EXACT_SHAPES)
def test_exact_arithmetic(T, L):
    """small-integer taps and samples (tests/test_resampler.py::test_exact_arithmetic_preconditions): every partial sum is an integer
    below 2^24, so the fp32 chain is exact and the kernel must give the restatement's integers to the bit; interp 1 with w a multiple
    of 1/8"""
    import gfdm_amd
    h, x = RC.exact_inputs(T, L)
    for interp, step in RC.EXACT_STEPS.items():
        want, _ = Q.resample(x, 0, h, interp, step, 0, 1500)
        rs = gfdm_amd.Resampler(step, h, interp="linear" if interp else "nearest")
        w = Window(1500, 1)
        rs.resample(_t(x), n_out=1500, out=w.view)
        assert np.array_equal(w.result(), want.astype(np.complex64)), (T, interp)


@pytest.mark.parametrize("T", [1, 8, 16, 64])
def test_split_invariance(T):
    """one flushed call of 4097 outputs equals, to the bit, its pieces chained through plan: the input cut at 1, 2, 255 and 1000, steps
    2^32 + 1, 3 * 2^31 and 2^29, both interp, complex64 and sc16 in"""
    import gfdm_amd
    L = 128 if T > 1 else 2
    for step in RC.SPLIT_STEPS:
        total, pos0 = RC.split_start(step)
        iq = Q.signal_sc16(50 + T, total)
        for interp in ("nearest", "linear"):
            rs = gfdm_amd.Resampler(step, Q.table_for(L, T), interp=interp)
            for x in (_t(Q.signal(40 + T, total)), _t(iq)):
                whole = _h(rs.resample(x, pos=pos0))
                assert whole.shape == (RC.SPLIT_N_OUT,) and rs.plan(total, pos0)[0] == RC.SPLIT_N_OUT
                for cut in RC.split_cuts(total):
                    parts = []
                    for k, (start, hist, n_in, pos, n_out) in enumerate(RC.chain(step, T, total, cut, pos0)):
                        assert rs.plan(n_in, pos, flush=k == 1)[0] == n_out
                        parts.append(_h(rs.resample(x[start - hist:start + n_in], history=hist, pos=pos, flush=k == 1)))
                    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole)), (T, step, interp, cut)


def test_sc16_twin_equals_the_widened_call():
    """int16 I/Q in, both extremes included, at every alignment of 4 bytes, (n, 2) and flat: bit-equal to the complex64 call on the
    widened capture"""
    import gfdm_amd
    n, hist = 3001, 7
    iq = Q.signal_sc16(9, n + hist)
    assert iq.min() == -32768 and iq.max() == 32767
    for T, interp, step in ((16, "linear", round(1.0001 * 2 ** 32)), (8, "nearest", 5 << 30), (3, "linear", 1 << 29)):
        rs = gfdm_amd.Resampler(step, Q.table_for(128, T), interp=interp)
        wide = _h(rs.resample(_t(Q.widen(iq)), history=hist, pos=1 << 31))
        for shift in range(4):
            x = Window(n + hist, shift, True, content=iq)
            got = _h(rs.resample(x.view.reshape(-1, 2), history=hist, pos=1 << 31))
            flat = _h(rs.resample(x.view, history=hist, pos=1 << 31))
            assert np.array_equal(_bits(got), _bits(wide)) and np.array_equal(_bits(flat), _bits(wide)), (T, shift)
        y, budget = Q.resample(Q.widen(iq), hist, rs.taps(), interp == "linear", step, 1 << 31, wide.size)
        _check(wide, y, budget, "sc16 twin T %d" % T)


@pytest.mark.parametrize("T", [1, 3, 16, 64])
def test_a_nan_reaches_its_window_and_no_other_output(T):
    """a NaN in x[j] shows only in outputs whose window [idx - D, idx - D + T) holds j; every other output is bit-equal to the call on
    clean input -- also where j lies in the history, at a tile's edge, or in the last sample"""
    import gfdm_amd
    n_in, history, step, pos = 4500, T + 5, round(1.0001 * 2 ** 32), 1 << 31
    D = (T - 1) // 2
    x = Q.signal(60 + T, n_in + history)
    rs = gfdm_amd.Resampler(step, Q.table_for(128 if T > 1 else 1, T), interp="linear")
    clean = _h(rs.resample(_t(x), history, pos))
    idx, _ = Q.positions(step, pos, clean.size)
    bad = x.copy()
    hit = np.zeros(clean.size, bool)
    for j in (-2, 700, 2047, 2048, n_in - 1):
        bad[history + j] = complex(np.nan, 1.0)
        hit |= (idx - D <= j) & (j < idx - D + T)
    got = _h(rs.resample(_t(bad), history, pos))
    assert not np.isnan(clean).any() and hit.any()
    assert not np.isnan(got[~hit]).any() and np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))
    assert np.isnan(got[hit].real).all()


def test_overlapping_buffers_are_refused():
    """out anywhere inside [in - history, in + n_in) is EINVAL; out right behind or in front of that range is fine"""
    import torch
    import gfdm_amd
    rs = gfdm_amd.Resampler(ONE, Q.table_for(2, 4))
    buf = torch.zeros(400, dtype=torch.complex64, device="cuda:0")
    x = buf[100:200]                                                         # history 10 + n_in 90
    for lo in (100, 110, 50, 199, 11):
        with pytest.raises(ValueError, match="overlap"):
            rs.resample(x, history=10, n_out=90, out=buf[lo:lo + 90])
    rs.resample(x, history=10, n_out=90, out=buf[200:290])
    rs.resample(x, history=10, n_out=90, out=buf[10:100])
    as16 = buf.view(torch.float32).view(torch.int16)
    with pytest.raises(ValueError, match="overlap"):
        rs.resample(as16[400:800], history=10, n_out=90, out=buf[140:230])      # 200 sc16 samples = complex samples 100 .. 199
    rs.resample(as16[400:800], history=10, n_out=90, out=buf[200:290])
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,interp,step", [(1, "nearest", ONE), (16, "linear", round(1.0001 * 2 ** 32)), (64, "linear", 1 << 35), (8, "nearest", 1 << 29)])
def test_host_flavour_equals_device_flavour(T, interp, step):
    import gfdm_amd
    rs = gfdm_amd.Resampler(step, Q.table_for(128 if T > 1 else 1, T), interp=interp)
    x = Q.signal(70 + T, 4097 + T)
    iq = Q.signal_sc16(71 + T, 4097 + T)
    for src in (x, iq):
        host = rs.resample(src, T, 5 * ONE + 1)
        dev = rs.resample(_t(src), T, 5 * ONE + 1)
        assert isinstance(host, np.ndarray) and host.dtype == np.complex64 and host.shape == tuple(dev.shape) and host.size > 0
        assert np.array_equal(_bits(host), _bits(_h(dev)))
    out = np.zeros(rs.plan(4097)[0], np.complex64)
    assert rs.resample(x, T, out=out) is out and out.any()
    assert rs.resample(x[:T], T).shape == (0,) and tuple(rs.resample(_t(x[:T]), T).shape) == (0,)      # n_out == 0: no launch
    with pytest.raises(TypeError):
        rs.resample(_t(x), out=out)


def test_set_step_is_read_at_enqueue():
    """set_step changes the next call: it equals a new handle's with that step, and the restatement"""
    import gfdm_amd
    x = _t(Q.signal(80, 1000))
    h = Q.table_for(128, 16)
    rs = gfdm_amd.Resampler(1.0, h)
    base = _h(rs.resample(x))
    rs.set_step(1.25)
    assert rs.step() == 5 << 30 and rs.n_taps() == 16 and rs.n_phases() == 128 and rs.interp() == "linear" and np.array_equal(rs.taps(), h)
    got = _h(rs.resample(x, pos=3))
    fresh = _h(gfdm_amd.Resampler(5 << 30, h).resample(x, pos=3))
    assert got.size == 800 and base.size == 1000 and np.array_equal(_bits(got), _bits(fresh))
    y, budget = Q.resample(_h(x), 0, h, 1, 5 << 30, 3, 800)
    _check(got, y, budget, "after set_step")
    with pytest.raises(ValueError):
        rs.set_step(9.0)
    assert rs.step() == 5 << 30


def test_graph_replay():
    """one capture of resample (a single kernel on the capturing stream), replayed after the input changed on the device: the
    restatement each time; set_step after the capture does not reach the replays"""
    import torch
    import gfdm_amd
    T, n_in, hist, step, pos = 16, 4097, 7, round(1.0001 * 2 ** 32), 1 << 31
    h = Q.table_for(128, T)
    rs = gfdm_amd.Resampler(step, h)
    n_out = rs.plan(n_in, pos)[0]
    x = torch.zeros(n_in + hist, dtype=torch.complex64, device="cuda:0")
    out = torch.zeros(n_out, dtype=torch.complex64, device="cuda:0")
    x.copy_(_t(Q.signal(90, n_in + hist)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        rs.resample(x, hist, pos, n_out=n_out, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rs.resample(x, hist, pos, n_out=n_out, out=out)
    rs.set_step(1.25)                                    # the graph keeps its step
    for seed in (91, 92):
        xs = Q.signal(seed, n_in + hist)
        x.copy_(_t(xs))
        graph.replay()
        torch.cuda.synchronize()
        y, budget = Q.resample(xs, hist, h, 1, step, pos, n_out)
        _check(_h(out), y, budget, "replay with input %d" % seed)


def _loop_front():
    """payload bytes -> map -> transmit -> place, on the device: (case, mapper, payload, placed stream)"""
    import gfdm_amd
    c = B.loop_case()
    M, K, L, A, N, cp = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"]
    pts = R.qpsk_points().astype(np.complex64)
    payload = S.pack(S.indices(c["sym"], pts, "qpsk"), 2)
    m = gfdm_amd.SymbolMapper(pts)
    sym = m.map(_t(payload), A * M)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < 1e-5            # the frames the CPU-side preconditions were checked on
    placed = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE).place(frames, _t(c["starts"]), c["out_len"])[0]
    return c, m, payload, placed


def _loop_back(c, m, payload, ds, want_starts):
    """detect -> demodulate_bursts -> decode on the device capture ds: every burst found within 1 of want_starts, payload bytes equal on
    the matched-filter receiver and on ZF + 2 IC rounds"""
    import gfdm_amd
    M, K, L, A, cp, nb = c["M"], c["K"], c["L"], c["A"], c["cp"], c["nb"]
    assert ds.is_cuda
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb
    fs = _h(r["frame_start"])[:nb]
    print("frame_start - expected:", (fs - want_starts).tolist())
    assert np.all(np.abs(fs - want_starts) <= 1)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    for rx in (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())):
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
        assert demod.is_cuda and tuple(demod.shape) == (nb + 3, A * M)
        got = _h(m.decode(demod, count=r["count"]))
        assert got.shape == (nb + 3, payload.shape[1]) and np.array_equal(got[:nb], payload) and not got[nb:].any()


def test_loop_with_a_clock_offset():
    """payload bytes -> map -> transmit -> place -> RESAMPLE -> apply -> detect -> demodulate_bursts -> decode -> payload bytes:
    tests/test_channel_model_gpu.py::test_loop_with_a_channel with the transmitter's clock e = 100 ppm off the receiver's (step =
    resampler_step(1 + e)) and half a sample of static offset (pos fraction 2^31), default table, 16 taps, linear.  e is the largest of
    25, 50, 100, 200 ppm at which tests/test_resampler.py::test_loop_preconditions shows the margins to hold on the restatements: at
    100 ppm threshold margin 0.193, decision margins 0.190 (ZF + 2 IC) and 0.190 (MF); at 200 ppm the IC margin is 0.081 < 0.1.
    Asserted: count == nb, every frame_start within 1 of round((start + pcp - pos / 2^32) / (step / 2^32)), payload bytes equal; the
    resampled stream is also held to the budget against the restatement on the stream the device placed."""
    import gfdm_amd
    c, m, payload, placed = _loop_front()
    step = gfdm_amd.resampler_step(1 + RC.LOOP_PPM * 1e-6)
    rs = gfdm_amd.Resampler(1 + RC.LOOP_PPM * 1e-6)
    assert rs.step() == step and np.array_equal(rs.taps(), RC.default_taps(step, 16))
    z = rs.resample(placed, pos=RC.LOOP_POS)
    y, budget = Q.resample(_h(placed), 0, rs.taps(), 1, step, RC.LOOP_POS, z.numel())
    _check(_h(z), y, budget, "loop stream")
    ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    _loop_back(c, m, payload, ch.apply(z), RC.expected_frame_starts(step, RC.LOOP_POS))


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_with_a_rate_change(fmt):
    """the same chain with place -> resample(step 4/5) -> apply -> resample(step 5/4) -> detect: the radio, and the channel with it,
    runs at 5/4 of the GFDM rate; with fmt sc16 apply writes int16 I/Q (gain LOOP_GAIN) and the second resampler reads it.  n_taps = 8
    is the smallest of 8, 16, 32 at which tests/test_resampler.py::test_loop_preconditions shows the margins to hold on the
    restatements (EVM of the two resamplers alone 0.131, threshold margin 0.184, decision margin 0.155; per n_taps in
    profiles/r19/resampler_accuracy.json).  Asserted: count == nb, payload bytes equal, every intermediate is a device tensor."""
    import fractions
    import gfdm_amd
    c, m, payload, placed = _loop_front()
    T = RC.LOOP_RATE_NTAPS
    up, down = gfdm_amd.Resampler(fractions.Fraction(4, 5), n_taps=T), gfdm_amd.Resampler(fractions.Fraction(5, 4), n_taps=T)
    assert np.array_equal(down.taps(), RC.default_taps(5 << 30, T))
    ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    kw = dict(sc16=True, gain=C.LOOP_GAIN) if fmt == "sc16" else {}
    at_radio = up.resample(placed)
    radio = ch.apply(at_radio, **kw)
    ds = down.resample(radio)
    assert at_radio.is_cuda and radio.is_cuda and radio.dtype == (__import__("torch").int16 if fmt == "sc16" else __import__("torch").complex64)
    assert abs(at_radio.numel() - placed.numel() * 5 // 4) <= 1 and abs(ds.numel() - placed.numel()) <= 2
    _loop_back(c, m, payload, ds, RC.expected_frame_starts(ONE, 0))


def test_no_input_at_all_gives_zeros():
    """history + n_in == 0 with n_out > 0: every x is zero and `in` is not touched, so it may be NULL -- host flavour (nothing is
    uploaded) and device flavour, complex64 and sc16"""
    import ctypes
    import torch
    import gfdm_amd
    L = gfdm_amd.lib()
    rs = gfdm_amd.Resampler(3 << 31, Q.table_for(128, 16))
    for stem in ("gfdm_hip_resampler_resample", "gfdm_hip_resampler_resample_sc16"):
        out = np.full(37, 7 + 7j, np.complex64)
        assert getattr(L, stem + "_host")(rs._h, out.ctypes.data, None, 37, 0, 0, 1 << 31) == 0, L.gfdm_hip_last_error()
        assert not out.any()
        w = Window(37, 1)
        assert getattr(L, stem + "_device")(rs._h, w.view.data_ptr(), None, 37, 0, 0, 1 << 31, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert not w.result().any()
        assert getattr(L, stem + "_host")(rs._h, out.ctypes.data, None, 37, 1, 0, 0) == gfdm_amd.capi.EINVAL      # a sample it would read
        assert getattr(L, stem + "_host")(rs._h, None, None, 37, 0, 0, 0) == gfdm_amd.capi.EINVAL
