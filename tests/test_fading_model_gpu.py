"""GPU tests of the fading model (contract in include/gfdm_hip.h, gfdm_hip_fading_model).  The yardstick is the float64 numpy restatement
of tests/fading_model_ref.py on the same complex64 inputs, never the code under test, and the bound is the contract's error budget
    |y - y64| <= (T + P + 16) 2^-23 sum_p Abar_p S_pi,        Abar_p = sum_s |A[p][s]|,  S_pi = sum_k |c[p][k]| |x[i - k]|,
counted from the roundings, not from what the kernel gives; every test prints the worst share of it that it saw.  sc16 output equals q
of the restatement except inside the guard band (within gain * budget of a step of q), where it may be one LSB off;
tests/test_fading_model.py holds that band under 1 % on the restatement alone.  Every output lies between guard words.  What the phases
being integers promises -- any cut of a stream gives the same samples -- is tested bit for bit."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import fading_model_ref as Fd
import gfdm_ref as R
import symbol_mapper_ref as S
from conftest import have_gpu, rel_err

pytestmark = pytest.mark.gpu
GUARD = 16                                  # guard elements on either side of a buffer: a multiple of 16 bytes for both dtypes
FILL = {"int16": 0x5A5A, "complex64": 7 + 7j}


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
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * (4 if sc16 else 8)) % 16
        if content is not None:
            self.view.copy_(_t(np.ascontiguousarray(content).ravel()))

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.fill) and np.all(b[self.lo + self.n:] == self.fill), "guard words overwritten"
        got = b[self.lo:self.lo + self.n]
        return got.reshape(-1, 2) if self.per == 2 else got


def _model(shape, seed=0):
    import gfdm_amd
    return gfdm_amd.FadingModel.from_tables(*Fd.tables_for(tuple(shape), seed))


def _check_c64(got, y, budget, tag):
    assert got.dtype == np.complex64 and got.shape == y.shape
    share = Fd.share_of_budget(got, y, budget)
    print("%s: worst error %.3f of the budget" % (tag, share))
    assert share <= 1.0, (tag, share)
    return share


def _check_sc16(got, y, budget, gain, tag):
    want, guard = Fd.sc16(y, budget, gain)
    assert got.dtype == np.int16 and got.shape == want.shape
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d components inside the guard band, %d of them one LSB off" % (tag, int(guard.sum()), guard.size, int(np.count_nonzero(d[guard]))))
    assert guard.sum() <= max(1, Fd.GUARD_CAP * guard.size), tag
    assert np.array_equal(got[~guard], want[~guard]), tag
    assert d.max(initial=0) <= 1, tag


@pytest.mark.parametrize("shape", Fd.SHAPES)
def test_every_shape(shape):
    """the case table of tests/fading_model_ref.py for one (P, S, T): every n from 1 to 65539, every kind of history, offsets of every
    position inside a run of eight up to 2^40 + 1, input at both alignments, output at every alignment of one sample, complex64 and sc16"""
    fm = _model(shape)
    gain = Fd.sc16_gain(shape)
    worst = 0.0
    for idx in range(len(Fd.cases(shape))):
        c = Fd.case_data(shape, idx)
        sc16 = c["fmt"] == "sc16"
        tag = "P %d S %d T %d n %d history %d offset %d %s in+%d out+%d" % (shape + (c["n"], c["history"], c["offset"], c["fmt"], c["in_shift"], c["out_shift"]))
        x = Window(c["history"] + c["n"], c["in_shift"], content=c["x"])
        w = Window(c["n"], c["out_shift"], sc16)
        res = fm.apply(x.view, c["history"], c["offset"], out=w.view, gain=gain if sc16 else 1.0)
        assert res is w.view
        if sc16:
            _check_sc16(w.result(), c["y"], c["budget"], gain, tag)
        else:
            worst = max(worst, _check_c64(w.result(), c["y"], c["budget"], tag))
        assert np.array_equal(_bits(x.result()), _bits(c["x"]))                 # the input is left alone
    print("P %d S %d T %d: worst share of the budget %.3f" % (shape + (worst,)))


def _pieces(n, cuts):
    edges = [0] + sorted(set(c for c in cuts if 0 < c < n)) + [n]
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("shape", [(1, 8, 1), (2, 3, 3), (4, 8, 16), (8, 17, 64)])
def test_split_invariance(shape):
    """one call of 4500 samples equals, to the bit, the same stream in pieces: cut once at 1, 7, 8 and 9 (cuts that are no multiple of
    eight, and a first piece shorter than T), and cut at a seeded ragged list of some forty points; each piece with history =
    min(T - 1, samples before it) and the advanced offset, from offsets of both kinds (inside a run and at its start); complex64 and sc16"""
    T = shape[2]
    n = 4500
    x = C.signal(40 + T, n)
    fm = _model(shape)
    dx = _t(x)
    rng = np.random.default_rng(shape)
    ragged = sorted(set(int(v) for v in np.cumsum(rng.integers(1, 230, 40))))
    assert any(c % 8 for c in ragged) and ragged[0] < 230
    for offset in (2 ** 31 - 1, 2 ** 40 + 8):
        for kw in (dict(), dict(sc16=True, gain=Fd.sc16_gain(shape))):
            whole = _h(fm.apply(dx, offset=offset, **kw))
            for cuts in ([1], [7], [8], [9], ragged):
                parts = []
                for a, b in _pieces(n, cuts):
                    hist = min(T - 1, a)
                    parts.append(_h(fm.apply(dx[a - hist:b], history=hist, offset=offset + a, **kw)))
                assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole)), (shape, offset, cuts[:3], kw)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 3), (8, 17, 64)])
def test_sc16_is_q_of_the_complex64_call(shape):
    """the sc16 twin writes q(y.re * gain), q(y.im * gain) from the same fp32 y as the complex64 call, the products in fp32: bit-equal,
    at every alignment of the output, for a gain that keeps values inside int16 and one that saturates some"""
    fm = _model(shape)
    n, hist, offset = 4099, shape[2] - 1, 2 ** 33 - 3
    dx = _t(C.signal(50 + shape[2], n + hist))
    y = _h(fm.apply(dx, hist, offset))
    for gain in (Fd.sc16_gain(shape), 20000.0, -3.5):
        want = np.stack((C.q16(y.real * np.float32(gain)), C.q16(y.imag * np.float32(gain))), axis=1)
        assert (y.real * np.float32(gain)).dtype == np.float32
        for shift in range(4):
            w = Window(n, shift, True)
            fm.apply(dx, hist, offset, out=w.view, gain=gain)
            assert np.array_equal(w.result(), want), (shape, gain, shift)
    assert np.abs(want).max() < 32767 and np.any(np.abs(C.q16(y.real * np.float32(20000.0))) == 32767)


@pytest.mark.parametrize("shape", [(1, 8, 1), (4, 8, 16)])
def test_scaling_is_exact(shape):
    """every step is linear in x, so apply(4 x) == 4 * apply(x) bit for bit"""
    fm = _model(shape)
    x = C.signal(55, 4097 + shape[2])
    a = _h(fm.apply(_t(x), shape[2], 12345))
    b = _h(fm.apply(_t(4 * x), shape[2], 12345))
    assert a.any() and np.array_equal(_bits(b), _bits((4 * a).astype(np.complex64)))


def test_all_frequencies_zero_is_the_channel_models_fir():
    """every F = 0: g_p is a constant and y = FIR(h) of x with h = sum_p g_p c[p][:], which ChannelModel runs: equal within the two
    budgets added (the taps reach the channel model rounded to complex64, 2^-24 |h| per tap: a twentieth of its budget at the most)"""
    import gfdm_amd
    worst = 0.0
    for shape in ((2, 3, 3), (8, 17, 64)):
        c, A, F, ph = Fd.tables_for(shape)
        F = np.zeros_like(F)
        g = Fd.gains(A, F, ph, 0, 1)[:, 0]
        h = np.sum(g[:, None] * c.astype(np.float64), axis=0).astype(np.complex64)
        T = shape[2]
        x = C.signal(60 + T, 4097 + T)
        for offset in (0, 2 ** 40 + 1):
            got = _h(gfdm_amd.FadingModel.from_tables(c, A, F, ph).apply(_t(x), T, offset))
            other = _h(gfdm_amd.ChannelModel(taps=h).apply(_t(x), T, offset))
            _, fb = Fd.apply(x, T, c, A, F, ph, offset)
            _, cb = C.apply(x, T, h, 0.0, 0.0, 0, offset)
            share = Fd.share_of_budget(got, other.astype(np.complex128), fb + cb)
            print("P %d S %d T %d offset %d: worst difference %.3f of the two budgets" % (shape + (offset, share)))
            worst = max(worst, share)
    assert worst <= 1.0


@pytest.mark.parametrize("f", [0.002, 1.0 / 3.0, -0.5])
def test_one_sinusoid_is_the_channel_models_mixer(f):
    """P = S = T = 1, A = c = 1, F = rint(f 2^64): y = x exp(j 2 pi f a), which ChannelModel([1], f) runs: equal within the two budgets
    added, at offsets up to 2^33 (where the channel model's float64 product f a carries 2^-22 of a cycle of its own)"""
    import gfdm_amd
    F = np.array([[int(np.rint(f * 2.0 ** 64)) if f != -0.5 else -2 ** 63]], np.int64)
    fm = gfdm_amd.FadingModel.from_tables([[1.0]], [[1.0]], F, np.zeros((1, 1), np.uint64))
    ch = gfdm_amd.ChannelModel(0.0, f, 1.0, [1])
    x = C.signal(70, 4097)
    worst = 0.0
    for offset in (0, 5, 2 ** 31 - 1, 2 ** 33):
        got, other = _h(fm.apply(_t(x), 0, offset)), _h(ch.apply(_t(x), 0, offset))
        y, fb = Fd.apply(x, 0, [[1.0]], [[1.0]], F, [[0]], offset)
        _, cb = C.apply(x, 0, [1], f, 0.0, 0, offset)
        _check_c64(got, y, fb, "f %g offset %d against the restatement" % (f, offset))
        share = Fd.share_of_budget(got, other.astype(np.complex128), fb + cb)
        print("f %g offset %d: worst difference %.3f of the two budgets" % (f, offset, share))
        worst = max(worst, share)
    assert worst <= 1.0


def test_unit_gain_returns_x():
    """A = 1, F = 0, Ph0 = 0 (and c = 1): x comes back equal in every component, whatever history and offset are"""
    import gfdm_amd
    fm = gfdm_amd.FadingModel.from_tables([[1.0]], [[1.0]], np.zeros((1, 1), np.int64), np.zeros((1, 1), np.uint64))
    x = C.signal(5, 4099)
    x[:4] = np.array([0, 3e38, complex(1e-42, -1e-42), -1e-45], np.complex64)
    for shift in (0, 1):
        w = Window(x.size, shift)
        fm.apply(_t(x), out=w.view)
        assert np.array_equal(w.result(), x)
    w = Window(x.size - 3, 1)
    fm.apply(_t(x), history=3, offset=2 ** 40 + 1, out=w.view)
    assert np.array_equal(w.result(), x[3:])


@pytest.mark.parametrize("shape", [(1, 8, 1), (2, 3, 3), (8, 17, 64)])
def test_a_nan_reaches_its_T_outputs_and_no_other(shape):
    """a NaN in x[j] shows in outputs j .. j + T - 1 (every coefficient non-zero); every other output is bit-equal to the call on clean
    input -- also where j lies in the history, at a tile's edge, inside and at the ends of a run of eight, or in the last sample"""
    T = shape[2]
    n, history = 4500, T + 5
    x = C.signal(60 + T, n + history)
    fm = _model(shape)
    assert np.all(Fd.tables_for(shape)[0] != 0)
    clean = _h(fm.apply(_t(x), history, offset=9))
    hit = np.zeros(n, bool)
    bad = x.copy()
    for j in (-2, 700, 1111, 2039, 2040, n - 1):                                # sample indices relative to the first output
        bad[history + j] = complex(np.nan, 1.0)
        hit[max(j, 0):max(min(j + T, n), 0)] = True
    got = _h(fm.apply(_t(bad), history, offset=9))
    assert np.all(np.isnan(got[hit].real) & np.isnan(got[hit].imag))
    assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit])) and not np.isnan(clean).any()


def test_overlapping_buffers_are_refused():
    """out anywhere inside [in - history, in + n) is EINVAL (the delay lines read neighbours: no in-place call); out right behind or in
    front of that range is fine"""
    import torch
    fm = _model((2, 3, 3))
    buf = torch.zeros(400, dtype=torch.complex64, device="cuda:0")
    x = buf[100:200]                                                         # history 10 + n 90
    for lo in (100, 110, 50, 199, 11):
        with pytest.raises(ValueError, match="overlap"):
            fm.apply(x, history=10, out=buf[lo:lo + 90])
    as16 = buf.view(torch.float32).view(torch.int16)
    with pytest.raises(ValueError, match="overlap"):
        fm.apply(x, history=10, out=as16[4 * 199:4 * 199 + 180])
    fm.apply(x, history=10, out=buf[200:290])
    fm.apply(x, history=10, out=buf[10:100])
    fm.apply(x, history=10, out=as16[4 * 55:4 * 55 + 180])                   # 90 sc16 samples end at sample 100 of the complex buffer
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 3), (8, 17, 64)])
def test_host_flavour_equals_device_flavour(shape):
    fm = _model(shape)
    T = shape[2]
    x = C.signal(70 + T, 4097 + T)
    for kw in (dict(), dict(sc16=True, gain=50.0)):
        host = fm.apply(x, T, 2 ** 40 + 1, **kw)
        dev = fm.apply(_t(x), T, 2 ** 40 + 1, **kw)
        assert isinstance(host, np.ndarray) and host.shape == tuple(dev.shape) and np.array_equal(_bits(host), _bits(_h(dev)))
    out = np.zeros(4097, np.complex64)
    assert fm.apply(x, T, out=out) is out and out.any()
    out16 = np.zeros((4097, 2), np.int16)
    assert fm.apply(x, T, out=out16, gain=50.0) is out16 and out16.any()             # an int16 out selects sc16
    assert fm.apply(x[:T], T).shape == (0,) and tuple(fm.apply(_t(x[:T]), T, sc16=True).shape) == (0, 2)      # n == 0: no launch
    with pytest.raises(TypeError):
        fm.apply(_t(x), out=out)
    with pytest.raises(ValueError, match="overlap"):
        fm.apply(x, T, out=x[T:])                                                 # in place


def test_graph_replay():
    """one capture of apply (a single kernel on the capturing stream), replayed twice after the input changed on the device: equal to the
    eager call, bit for bit, and inside the budget"""
    import torch
    shape, n, hist, offset = (4, 8, 16), 4097, 15, 2 ** 33 - 3
    fm = _model(shape)
    x = torch.zeros(n + hist, dtype=torch.complex64, device="cuda:0")
    out = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    x.copy_(_t(C.signal(90, n + hist)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        fm.apply(x, hist, offset, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fm.apply(x, hist, offset, out=out)
    for seed in (91, 92):
        xs = C.signal(seed, n + hist)
        x.copy_(_t(xs))
        graph.replay()
        torch.cuda.synchronize()
        got = _h(out).copy()
        assert np.array_equal(_bits(got), _bits(_h(fm.apply(_t(xs), hist, offset))))
        y, budget = Fd.apply(xs, hist, *Fd.tables_for(shape), offset)
        _check_c64(got, y, budget, "replay with input %d" % seed)


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_with_a_fading_channel(fmt):
    """payload bytes -> map -> transmit -> place -> FADE -> apply(taps = [1], CFO, noise) -> detect -> match -> demodulate_bursts -> decode
    -> payload bytes: tests/test_channel_model_gpu.py::test_loop_with_a_channel with the fixed taps replaced by two fading paths (delays
    0 and 1.5, mags 1 and 0.3, 8 taps), Rician on the first (K = 4), N = 8, fDTs = 5e-5 -- the largest of the ladder 1e-5, 2e-5, 5e-5, 1e-4,
    2e-4 at which tests/test_fading_model.py::test_loop_preconditions shows the margins to hold on the restatements.  With fmt sc16 the
    channel model writes int16 I/Q.  Asserted: the faded stream within the budget of the restatement; every sent burst detected and
    matched; every payload right on both receivers; and |g_0| of the restatement differs between the first and the last burst by more
    than it changes inside one -- every burst saw another channel."""
    import gfdm_amd
    c = B.loop_case()
    M, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym = A * M
    pts = R.qpsk_points().astype(np.complex64)
    payload = S.pack(S.indices(c["sym"], pts, "qpsk"), 2)
    m = gfdm_amd.SymbolMapper(pts)
    sym = m.map(_t(payload), n_sym)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < 1e-5            # the frames the CPU-side preconditions were checked on
    placed = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE).place(frames, _t(c["starts"]), c["out_len"])[0]
    fm = gfdm_amd.FadingModel(Fd.LOOP_N, Fd.LOOP_FDTS, True, Fd.LOOP_K, Fd.LOOP_SEED, Fd.LOOP_DELAYS, Fd.LOOP_MAGS, Fd.LOOP_NTAPS)
    tables = Fd.loop_tables()
    for got, want in zip((fm.taps(), fm.amplitudes(), fm.frequencies(), fm.phases()), tables):
        assert np.array_equal(got, want)
    faded = fm.apply(placed)
    z, zbudget = Fd.apply(_h(placed), 0, *tables, 0)                                   # the restatement on the stream the device placed
    _check_c64(_h(faded), z, zbudget, "faded loop stream")
    ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, [1], C.LOOP_SEED)
    ds = ch.apply(faded, **(dict(sc16=True, gain=C.LOOP_GAIN) if fmt == "sc16" else {}))
    assert ds.is_cuda and faded.is_cuda
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb
    lm = gfdm_amd.LinkMeter(pts)
    lm.reset()
    q = lm.match(r["frame_start"], _t(c["starts"] + c["pcp"]), 1, count=r["count"])
    assert np.array_equal(_h(q["sent_row"]), np.arange(nb)) and np.array_equal(_h(q["ref_row"])[:nb], np.arange(nb))
    t = lm.totals()
    assert (t["detections"], t["matched"], t["missed"], t["false_alarms"]) == (nb, nb, 0, 0)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    for rx in (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())):
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
        assert tuple(demod.shape) == (nb + 3, n_sym)
        got = _h(m.decode(demod, count=r["count"]))
        assert got.shape == (nb + 3, payload.shape[1]) and np.array_equal(got[:nb], payload) and not got[nb:].any()
    between, inside = Fd.loop_gain_change()
    print("|g_0| between the first and the last burst %.4f, inside one burst at most %.4f" % (between, inside))
    assert between > inside > 0
