"""GPU tests of the channel model (contract in include/gfdm_hip.h, gfdm_hip_channel_model).  The yardstick is the float64 numpy restatement
of tests/channel_model_ref.py on the same complex64 inputs, never the code under test, and the bound is the contract's error budget
    |y - y64| <= (T + 10) 2^-23 S_i + 2^-20 (s / sqrt 2) |w(a)| + 2^-23 |y64|,        S_i = sum_t |h[t]| |x[i - t]|,
derived there from the operations, not from what the kernel gives; every test prints the worst share of it that it saw.  sc16 output
equals q of the restatement except inside the guard band (within gain * budget of a step of q), where it may be one LSB off;
tests/test_channel_model.py holds that band under 1 % on the restatement alone.  Every output lies between guard words."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
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


def _model(c, **kw):
    import gfdm_amd
    return gfdm_amd.ChannelModel(kw.get("s", c["s"]), kw.get("f", c["f"]), 1.0, c["taps"], c["seed"])


def _check_c64(got, y, budget, tag):
    assert got.dtype == np.complex64 and got.shape == y.shape
    share = C.share_of_budget(got, y, budget)
    print("%s: worst error %.3f of the budget" % (tag, share))
    assert share <= 1.0, (tag, share)
    return share


def _check_sc16(got, y, budget, gain, tag):
    want, guard = C.sc16(y, budget, gain)
    assert got.dtype == np.int16 and got.shape == want.shape
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d components inside the guard band, %d of them one LSB off" % (tag, int(guard.sum()), guard.size, int(np.count_nonzero(d[guard]))))
    assert np.array_equal(got[~guard], want[~guard]), tag
    assert d.max(initial=0) <= 1, tag


@pytest.mark.parametrize("T", C.TS)
def test_every_shape(T):
    """the case table of tests/channel_model_ref.py for one T: every n from 1 to 65539, every kind of history, every f, s on and off, offsets
    of both parities up to 2^40 + 1 (one with the Philox counter's high word changing inside the call), input at both alignments, output
    at every alignment of one sample, complex64 and sc16"""
    worst = 0.0
    for idx in range(len(C.cases(T))):
        c = C.case_data(T, idx)
        sc16 = c["fmt"] == "sc16"
        tag = "T %d n %d history %d f %g s %g offset %d %s in+%d out+%d" % (T, c["n"], c["history"], c["f"], c["s"], c["offset"], c["fmt"], c["in_shift"], c["out_shift"])
        ch = _model(c)
        x = Window(c["history"] + c["n"], c["in_shift"], content=c["x"])
        w = Window(c["n"], c["out_shift"], sc16)
        res = ch.apply(x.view, c["history"], c["offset"], sc16=sc16, gain=C.sc16_gain(T) if sc16 else 1.0, out=w.view)
        assert res is w.view
        if sc16:
            _check_sc16(w.result(), c["y"], c["budget"], C.sc16_gain(T), tag)
        else:
            worst = max(worst, _check_c64(w.result(), c["y"], c["budget"], tag))
        assert np.array_equal(_bits(x.result()), _bits(c["x"]))                 # the input is left alone
    print("T %d: worst share of the budget %.3f" % (T, worst))


def test_unit_tap_is_a_bit_copy():
    """T = 1, h = 1, f = 0, s = 0: the output is the input, bit for bit -- signed zeros, infinities and denormals included"""
    import gfdm_amd
    x = C.signal(5, 4099)
    x[:8] = np.array([0, -0.0, complex(-0.0, 0.0), complex(np.inf, -1), complex(1e-42, -1e-42), complex(-np.inf, np.inf), 3e38, -1e-45], np.complex64)
    ch = gfdm_amd.ChannelModel()
    for shift in (0, 1):
        w = Window(x.size, shift)
        ch.apply(_t(x), out=w.view)
        assert np.array_equal(_bits(w.result()), _bits(x))
    w = Window(x.size - 3, 1)
    ch.apply(_t(x), history=3, offset=2 ** 40 + 1, out=w.view)                # neither history nor offset plays a part
    assert np.array_equal(_bits(w.result()), _bits(x[3:]))


@pytest.mark.parametrize("T", [2, 3, 8, 64])
def test_without_mixer_and_noise_it_is_the_fp32_fir(T):
    """s = 0, f = 0 on small-integer taps and samples: every product and partial sum is an integer below 2^24, so the fp32 FIR is exact
    in any order and with or without fused multiply-adds, and the kernel must equal it to the bit; complex taps and taps with zero
    imaginary part (the kernel leaves those products out)"""
    import gfdm_amd
    rng = np.random.default_rng(T)
    n, history = 4097, T - 1
    x = (rng.integers(-64, 65, n + history) + 1j * rng.integers(-64, 65, n + history)).astype(np.complex64)
    for real in (False, True):
        taps = (rng.integers(-8, 9, T) + (0 if real else 1j) * rng.integers(-8, 9, T)).astype(np.complex64)
        taps[0] = 1
        want, _ = C.fir(x, history, taps)
        assert np.abs(want.real).max() < 2 ** 20 and np.array_equal(want, want.astype(np.complex64))
        ch = gfdm_amd.ChannelModel(taps=taps)
        w = Window(n, 1)
        ch.apply(_t(x), history, out=w.view)
        assert np.array_equal(w.result(), want.astype(np.complex64)), (T, real)
        head = _h(ch.apply(_t(x[history:])))                                     # without history the first T - 1 outputs see zeros
        want0, _ = C.fir(x[history:], 0, taps)
        assert np.array_equal(head, want0.astype(np.complex64))


def test_noise_alone_is_w_over_sqrt_two():
    """x = 0, s = 1 over 2^20 samples from an odd offset: y = w(a) / sqrt 2 element by element, within 2^-20 |w| / sqrt 2 + 2^-23 |y| (what
    the budget leaves when S = 0); the sample statistics follow from that and from tests/test_channel_model.py"""
    import torch
    import gfdm_amd
    n, seed, offset = 1 << 20, 7, 2 ** 33 - 3
    x = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    for T in (1, 3):
        got = _h(gfdm_amd.ChannelModel(1.0, 0.0, 1.0, np.ones(T), seed).apply(x, offset=offset))
        y, budget = C.apply(np.zeros(n, np.complex64), 0, np.ones(T), 0.0, 1.0, seed, offset)
        assert np.allclose(y, C.noise(offset, n, seed) / np.sqrt(2.0), rtol=1e-14, atol=0)
        _check_c64(got, y, budget, "noise alone, T %d" % T)
    power = float(np.mean(np.abs(got.astype(np.complex128)) ** 2))
    assert abs(power - 1.0) <= 5 / np.sqrt(n)                                    # noise power = noise_voltage^2


@pytest.mark.parametrize("T,f,s", [(1, 0.0, 1.0), (3, 1.0 / 3.0, 1.0), (8, 0.002, 0.0), (64, 0.4999, 1.0)])
def test_split_invariance(T, f, s):
    """one call of 4097 samples equals, to the bit, its pieces cut at 1, 2, 255 and 1000, each with history = min(T - 1, cut) and the
    advanced offset; complex64 and sc16"""
    import gfdm_amd
    n, offset = 4097, 2 ** 31 - 1
    x = C.signal(40 + T, n)
    ch = gfdm_amd.ChannelModel(s, f, 1.0, C.taps_for(T), 3)
    dx = _t(x)
    for kw in (dict(), dict(sc16=True, gain=100.0)):
        whole = _h(ch.apply(dx, offset=offset, **kw))
        for cut in (1, 2, 255, 1000):
            hist = min(T - 1, cut)
            a = _h(ch.apply(dx[:cut], offset=offset, **kw))
            b = _h(ch.apply(dx[cut - hist:], history=hist, offset=offset + cut, **kw))
            assert np.array_equal(_bits(np.concatenate((a, b))), _bits(whole)), (T, cut, kw)


def test_sc16_truncates_and_saturates():
    """q on known values: truncation toward zero (-0.9, 0.9, +-1.5), saturation, a NaN -> 0, through T = 1, h = 1 (v = x exactly) and a gain
    that is a power of two (the product is exact), so there is no guard band"""
    import gfdm_amd
    v = np.array([32767.4, -32767.4, 32767.9, 40000.0, -40000.0, -32768.0, -32769.5, -0.9, 0.9, 1.5, -1.5, 3e38, -3e38, 12.0], np.float32)
    want = [32767, -32767, 32767, 32767, -32768, -32768, -32768, 0, 0, 1, -1, 32767, -32768, 12]
    x = np.empty(v.size + 1, np.complex64)
    x.real[:-1], x.imag[:-1] = v / 4, v[::-1] / 4
    x[-1] = complex(np.nan, 5.0)
    for shift in range(4):
        w = Window(x.size, shift, True)
        gfdm_amd.ChannelModel().apply(_t(x), sc16=True, gain=4.0, out=w.view)
        got = w.result()
        assert got[:, 0].tolist() == want + [0] and got[:, 1].tolist() == want[::-1] + [20]


@pytest.mark.parametrize("T", [1, 3, 64])
def test_a_nan_reaches_its_T_outputs_and_no_other(T):
    """a NaN in x[j] shows in outputs j .. j + T - 1 (all taps non-zero); every other output is bit-equal to the call on clean input -- also
    where j lies in the history, at a tile's edge, or in the last sample"""
    import gfdm_amd
    n, history = 4500, T + 5
    x = C.signal(60 + T, n + history)
    ch = gfdm_amd.ChannelModel(1.0, 0.002, 1.0, C.taps_for(T), 5)
    clean = _h(ch.apply(_t(x), history, offset=9))
    hit = np.zeros(n, bool)
    bad = x.copy()
    for j in (-2, 700, 2043, 2044, n - 1):                                      # sample indices relative to the first output
        bad[history + j] = complex(np.nan, 1.0)
        hit[max(j, 0):max(min(j + T, n), 0)] = True                          # (j + T <= 0: the NaN lies too far back to reach an output)
    got = _h(ch.apply(_t(bad), history, offset=9))
    assert np.all(np.isnan(got[hit].real) & np.isnan(got[hit].imag))
    assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit])) and not np.isnan(clean).any()


def test_overlapping_buffers_are_refused():
    """out anywhere inside [in - history, in + n) is EINVAL (the FIR reads neighbours: no in-place call); out right behind or in front of
    that range is fine"""
    import torch
    import gfdm_amd
    ch = gfdm_amd.ChannelModel(taps=[1, 0.5])
    buf = torch.zeros(400, dtype=torch.complex64, device="cuda:0")
    x = buf[100:200]                                                         # history 10 + n 90
    for lo in (100, 110, 50, 199, 11):
        with pytest.raises(ValueError, match="overlap"):
            ch.apply(x, history=10, out=buf[lo:lo + 90])
    as16 = buf.view(torch.float32).view(torch.int16)
    with pytest.raises(ValueError, match="overlap"):
        ch.apply(x, history=10, sc16=True, out=as16[4 * 199:4 * 199 + 180])
    ch.apply(x, history=10, out=buf[200:290])
    ch.apply(x, history=10, out=buf[10:100])
    ch.apply(x, history=10, sc16=True, out=as16[4 * 55:4 * 55 + 180])         # 90 sc16 samples end at sample 100 of the complex buffer
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,f,s", [(1, 0.0, 0.0), (3, -0.5, 1.0), (64, 0.002, 1.0)])
def test_host_flavour_equals_device_flavour(T, f, s):
    import gfdm_amd
    ch = gfdm_amd.ChannelModel(s, f, 1.0, C.taps_for(T), 21)
    x = C.signal(70 + T, 4097 + T)
    for kw in (dict(), dict(sc16=True, gain=50.0)):
        host = ch.apply(x, T, 2 ** 40 + 1, **kw)
        dev = ch.apply(_t(x), T, 2 ** 40 + 1, **kw)
        assert isinstance(host, np.ndarray) and host.shape == tuple(dev.shape) and np.array_equal(_bits(host), _bits(_h(dev)))
    out = np.zeros(4097, np.complex64)
    assert ch.apply(x, T, out=out) is out and out.any()
    assert ch.apply(x[:T], T).shape == (0,) and tuple(ch.apply(_t(x[:T]), T, sc16=True).shape) == (0, 2)      # n == 0: no launch
    with pytest.raises(TypeError):
        ch.apply(_t(x), out=out)
    with pytest.raises(ValueError, match="overlap"):
        ch.apply(x, T, out=x[T:])                                                 # in place


def test_setters_are_read_at_enqueue():
    """set_frequency_offset, set_noise_voltage and set_seed change the next call: it equals a new handle's with those values"""
    import gfdm_amd
    x = _t(C.signal(80, 1000))
    taps = C.taps_for(3)
    ch = gfdm_amd.ChannelModel(0.0, 0.0, 1.0, taps, 1)
    base = _h(ch.apply(x))
    ch.set_frequency_offset(0.25)
    ch.set_noise_voltage(0.5)
    ch.set_seed(2 ** 63 + 5)
    assert (ch.frequency_offset(), ch.noise_voltage(), ch.seed()) == (0.25, 0.5, 2 ** 63 + 5)
    got = _h(ch.apply(x, offset=3))
    fresh = _h(gfdm_amd.ChannelModel(0.5, 0.25, 1.0, taps, 2 ** 63 + 5).apply(x, offset=3))
    assert np.array_equal(_bits(got), _bits(fresh)) and not np.array_equal(_bits(got), _bits(base))
    y, budget = C.apply(_h(x), 0, taps, 0.25, 0.5, 2 ** 63 + 5, 3)
    _check_c64(got, y, budget, "after the setters")


def test_graph_replay():
    """one capture of apply (a single kernel on the capturing stream), replayed after the input changed on the device: the restatement
    each time; a setter called after the capture does not reach the replays"""
    import torch
    import gfdm_amd
    T, n, hist, offset = 8, 4097, 7, 2 ** 33 - 3
    taps = C.taps_for(T)
    ch = gfdm_amd.ChannelModel(1.0, 0.002, 1.0, taps, 9)
    x = torch.zeros(n + hist, dtype=torch.complex64, device="cuda:0")
    out = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    x.copy_(_t(C.signal(90, n + hist)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        ch.apply(x, hist, offset, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ch.apply(x, hist, offset, out=out)
    ch.set_seed(10)                                      # the graph keeps seed 9
    for seed in (91, 92):
        xs = C.signal(seed, n + hist)
        x.copy_(_t(xs))
        graph.replay()
        torch.cuda.synchronize()
        y, budget = C.apply(xs, hist, taps, 0.002, 1.0, 9, offset)
        _check_c64(_h(out), y, budget, "replay with input %d" % seed)


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_with_a_channel(fmt):
    """payload bytes -> map -> transmit -> place -> APPLY -> detect -> demodulate_bursts -> decode -> payload bytes, as
    tests/test_symbol_mapper_gpu.py::test_loop_on_the_device but through three taps, a CFO of -0.003 and noise 20 dB below the frames;
    tests/test_channel_model.py::test_loop_preconditions holds the threshold and decision margins of exactly this stream on the float64
    restatements.  The matched filter on the plain receiver and ZF + 2 IC rounds on the advanced one; nothing leaves the device in
    between."""
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
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(frames, _t(c["starts"]), c["out_len"])[0]
    ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    kw = dict(sc16=True, gain=C.LOOP_GAIN) if fmt == "sc16" else {}
    ds = ch.apply(placed, **kw)
    # the channel's output for the stream the device placed, against the restatement on that same stream
    y, budget = C.apply(_h(placed), 0, C.LOOP_TAPS, C.LOOP_F, C.LOOP_NOISE_VOLTAGE, C.LOOP_SEED, 0)
    if fmt == "sc16":
        _check_sc16(_h(ds), y, budget, C.LOOP_GAIN, "loop stream")
        assert np.abs(_h(ds).astype(np.int32)).max() < 2048
    else:
        _check_c64(_h(ds), y, budget, "loop stream")
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb and np.array_equal(_h(r["frame_start"])[:nb], c["starts"] + c["pcp"])
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    for rx in (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())):
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
        assert tuple(demod.shape) == (nb + 3, n_sym)
        got = _h(m.decode(demod, count=r["count"]))
        assert got.shape == (nb + 3, payload.shape[1]) and np.array_equal(got[:nb], payload) and not got[nb:].any()
