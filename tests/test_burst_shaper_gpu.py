"""GPU tests of the burst shaper (contract in include/gfdm_hip.h, gfdm_hip_burst_shaper).  The yardstick is the numpy restatement of
tests/burst_shaper_ref.py, never the code under test:
  complex64, scale with imaginary part 0: equal to the float32 restatement;  complex scale: within 4 * 2^-24 |scale| |x| per component
  (two products and one sum in fp32, each rounded once, fused or not);
  sc16, fixed gain: equal;  sc16 normalised, real scale: equal, the largest component compared exactly, and within 1 LSB of to_sc16.
Every output lies between guard words, at every alignment one sample allows."""
import numpy as np
import pytest

import burst_shaper_ref as S
import gfdm_ref as R
from burst_receive_cases import MARGIN, restatement, virtual_bursts
from conftest import check_err, have_gpu, rel_err

pytestmark = pytest.mark.gpu
GUARD = 8                                   # guard samples on either side of an output
TOL = 1e-5                                  # tests/test_burst_receive_gpu.py's bound for fused-versus-chain and chain-versus-float64
FRAME_LENS = (1, 3, 255, 256, 257, 721)
PADS = ((0, 0), (1, 0), (0, 1), (1, 1), (5, 0), (0, 5), (5, 1), (1, 5), (5, 5))


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


def _frames(rng, n, F):
    return (rng.standard_normal((n, F)) + 1j * rng.standard_normal((n, F))).astype(np.complex64)


class Guarded:
    """an output of n samples inside a larger buffer, `shift` samples past a 16-byte boundary, guard words on either side"""

    def __init__(self, n, sc16, shift):
        import torch
        self.lo, self.n = GUARD + shift, n
        if sc16:
            self.buf = torch.full((self.lo + n + GUARD, 2), 0x5A5A, dtype=torch.int16, device="cuda:0")
        else:
            self.buf = torch.full((self.lo + n + GUARD,), 7 + 7j, dtype=torch.complex64, device="cuda:0")
        self.out = self.buf[self.lo:self.lo + n]
        self.guard = _h(self.buf[0]).copy()
        assert self.out.is_contiguous() and (self.out.data_ptr() // (4 if sc16 else 8)) % (4 if sc16 else 2) == shift % (4 if sc16 else 2)

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.guard) and np.all(b[self.lo + self.n:] == self.guard), "guard words overwritten"
        return b[self.lo:self.lo + self.n]


def _shifts(sc16):
    return range(4 if sc16 else 2)


def _assert_c64(got, want, scale, xabs):
    """xabs: |x| of the frame sample behind every output sample (0 in the gaps)"""
    if complex(scale).imag == 0:
        assert np.array_equal(got, want)
    else:
        bound = 4 * 2.0 ** -24 * abs(scale) * xabs
        assert np.all(np.abs(got.real.astype(np.float64) - want.real) <= bound) and np.all(np.abs(got.imag.astype(np.float64) - want.imag) <= bound)


def _place_starts(F, n, lead, tail):
    """a lead-in, a back-to-back pair, a gap of 1, a gap of several frames, ..., a tail"""
    gaps = np.array((lead, 0, 1, 3 * F + 2, 2, 0, 7)[:n])
    starts = np.cumsum(gaps + np.concatenate(([0], np.full(n - 1, F)))).astype(np.int64)
    return starts, int(starts[-1] + F + tail)


@pytest.mark.parametrize("F", FRAME_LENS)
def test_shape_complex64(F):
    import gfdm_amd
    rng = np.random.default_rng(F)
    k = 0
    for scale in (0.75, 0.6 - 0.3j):
        for pre, post in PADS:
            sh = gfdm_amd.BurstShaper(F, pre, post, scale)
            for n in (1, 7):
                x = _frames(rng, n, F)
                want = S.shape_c64(x, F, pre, post, scale)
                g = Guarded(want.size, False, k % 2)
                k += 1
                res = sh.shape(_t(x), out=g.out)
                assert res is g.out
                _assert_c64(g.result(), want, scale, S.shape_c64(np.abs(x), F, pre, post, 1.0).real)
            assert tuple(sh.shape(_t(x)).shape) == (n * sh.slot_len(),)


@pytest.mark.parametrize("F", FRAME_LENS)
def test_place_complex64(F):
    import gfdm_amd
    rng = np.random.default_rng(100 + F)
    for scale in (-1.25, 0.6 - 0.3j):
        sh = gfdm_amd.BurstShaper(F, 3, 2, scale)              # the paddings play no part in place
        for n in (1, 7):
            x = _frames(rng, n, F)
            for lead, tail in ((0, 0), (4, 9), (5, 0)):        # no lead-in; an even and an odd starts[0]; with and without a tail
                starts, out_len = _place_starts(F, n, lead, tail)
                want = S.place_c64(x, F, starts, out_len, scale)
                xabs = S.place_c64(np.abs(x), F, starts, out_len, 1.0).real
                for shift in _shifts(False):
                    g = Guarded(out_len, False, shift)
                    sh.place(_t(x), _t(starts), out_len, out=g.out)
                    _assert_c64(g.result(), want, scale, xabs)


def test_many_bursts():
    """32768 + 7 bursts of 5 samples in one call: shape with paddings 1 and 5, place with gaps 0, 1, 3 and 12 in turn; both formats.  (About
    240 starts fall into 16 KiB of the complex64 stream and 480 into 16 KiB of the sc16 stream: either side of the kernel's LDS window.)"""
    import gfdm_amd
    F, n = 5, 32768 + 7
    rng = np.random.default_rng(5)
    x = _frames(rng, n, F) * np.float32(900)
    sh = gfdm_amd.BurstShaper(F, 1, 5, 2.0)
    dx = _t(x)
    assert np.array_equal(_h(sh.shape(dx)), S.shape_c64(x, F, 1, 5, 2.0))
    assert np.array_equal(_h(sh.shape(dx, sc16=True, peak=30000)), S.shape_sc16(x, F, 1, 5, 2.0, 30000))
    starts = np.cumsum(np.array((2, 0, 1, 3, 12))[np.arange(n) % 5] + np.concatenate(([0], np.full(n - 1, F)))).astype(np.int64)
    out_len = int(starts[-1] + F + 3)
    for shift in (0, 1):
        g = Guarded(out_len, False, shift)
        sh.place(dx, _t(starts), out_len, out=g.out)
        assert np.array_equal(g.result(), S.place_c64(x, F, starts, out_len, 2.0))
    g = Guarded(out_len, True, 3)
    sh.place(dx, _t(starts), out_len, sc16=True, out=g.out)
    assert np.array_equal(g.result(), S.place_sc16(x, F, starts, out_len, 2.0))
    # 5000 bursts of 3 samples, 0 to 2 samples apart: more starts in a workgroup's 16 KiB than its LDS window holds (255), in both formats
    F, n = 3, 5000
    x = _frames(rng, n, F) * np.float32(900)
    sh = gfdm_amd.BurstShaper(F, scale=2.0)
    starts = np.cumsum(np.array((1, 0, 1, 0, 2))[np.arange(n) % 5] + np.concatenate(([0], np.full(n - 1, F)))).astype(np.int64)
    out_len = int(starts[-1] + F + 1)
    for sc16 in (False, True):
        g = Guarded(out_len, sc16, 1)
        sh.place(_t(x), _t(starts), out_len, sc16=sc16, out=g.out)
        assert np.array_equal(g.result(), (S.place_sc16 if sc16 else S.place_c64)(x, F, starts, out_len, 2.0))
    assert np.array_equal(_h(sh.shape(_t(x))), S.shape_c64(x, F, 0, 0, 2.0))


@pytest.mark.parametrize("sc16", [False, True])
def test_count(sc16):
    """count of 0, 3 and n_bursts out of 7; a negative one and one above n_bursts are clamped; the spare frames never appear"""
    import torch
    import gfdm_amd
    F, n = 257, 7
    rng = np.random.default_rng(7)
    x = _frames(rng, n, F)
    sh = gfdm_amd.BurstShaper(F, scale=3.0)
    starts, out_len = _place_starts(F, n, 5, 4)
    dx, ds = _t(x), _t(starts)
    full = _h(sh.place(dx, ds, out_len, sc16=sc16))
    for cnt in (0, 3, n, -2, n + 5):
        live = min(max(cnt, 0), n)
        marked = x.copy()
        marked[live:] = 1e4 + 1e4j                                       # a spare frame in the output would show
        for count in (cnt, _t([cnt], torch.int64)):
            for peak in ((None, 2000.0) if sc16 else (None,)):
                g = Guarded(out_len, sc16, 1)
                sh.place(_t(marked), ds, out_len, count=count, sc16=sc16, peak=peak, out=g.out)
                got = g.result()
                want = (S.place_sc16(marked, F, starts, out_len, 3.0, cnt, peak or 0) if sc16 else S.place_c64(marked, F, starts, out_len, 3.0, cnt))
                assert np.array_equal(got, want), (cnt, peak)
                if peak is None:
                    end = out_len if live == n else int(starts[live])
                    assert np.array_equal(got[:end], full[:end]) and not got[end:].any()


@pytest.mark.parametrize("sc16", [False, True])
def test_cutting_rule_of_the_device_flavour(sc16):
    """starts the host flavour would refuse, defined by the contract's cutting rule and in bounds by it: a frame overlapping its successor,
    a last frame running past out_len, starts[0] = -2"""
    import gfdm_amd
    F, n = 255, 4
    rng = np.random.default_rng(11)
    x = _frames(rng, n, F) * np.float32(100)
    sh = gfdm_amd.BurstShaper(F, scale=0.5)
    starts = np.array([-2, F + 10, F + 10 + F - 31, 3 * F], np.int64)
    out_len = 3 * F + 100
    want = S.place_sc16(x, F, starts, out_len, 0.5) if sc16 else S.place_c64(x, F, starts, out_len, 0.5)
    for shift in _shifts(sc16):
        g = Guarded(out_len, sc16, shift)
        sh.place(_t(x), _t(starts), out_len, sc16=sc16, out=g.out)
        assert np.array_equal(g.result(), want)
    assert np.array_equal(want[:F - 2], S.to_sc16_out(S.scaled(x[0, 2:], 0.5), 1) if sc16 else S.scaled(x[0, 2:], 0.5))     # the part before sample 0 dropped
    for bad in (starts, [5, 5 + F - 1, 3 * F, 5 * F], [0, F, 2 * F, out_len - F + 1], [3 * F, 2 * F, F, 0]):              # ... and the host flavour refuses them
        with pytest.raises(ValueError, match="negative|runs into"):
            sh.place(x, np.array(bad, np.int64), out_len, sc16=sc16)
    # beyond count nothing is checked: those frames are not placed
    assert np.array_equal(sh.place(x, np.array([0, F, 9, -4], np.int64), out_len, count=2, sc16=sc16),
                          S.place_sc16(x, F, [0, F, 9, -4], out_len, 0.5, 2) if sc16 else S.place_c64(x, F, [0, F, 9, -4], out_len, 0.5, 2))


SPECIALS = np.array([32767.4, -32767.4, 32767.9, 32768.0, -32768.0, -32768.9, 40000.5, -40000.5, 1e9, -1e9, -0.9, 0.9, 1.9, -1.9, 0.0, 123.0], np.float32)


def test_sc16_fixed_gain():
    """equal to the restatement: truncation toward zero (-0.9, 0.9), saturation (+-32767.4, beyond +-40000), a NaN"""
    import gfdm_amd
    F, n = SPECIALS.size + 1, 3
    x = np.zeros((n, F), np.complex64)
    x.real[:, :-1], x.imag[:, :-1] = SPECIALS, SPECIALS[::-1]
    x[1] = x[1] * np.float32(0.5)
    x[:, -1] = [complex(np.nan, 5), complex(3, np.nan), complex(np.nan, np.nan)]
    for scale in (1.0, 2.0, -0.5):
        sh = gfdm_amd.BurstShaper(F, 1, 5, scale)
        want = S.shape_sc16(x, F, 1, 5, scale)
        assert want.min() == -32768 and want.max() == 32767
        starts, out_len = _place_starts(F, n, 5, 2)
        for shift in _shifts(True):
            g = Guarded(want.shape[0], True, shift)
            sh.shape(_t(x), sc16=True, out=g.out)
            assert np.array_equal(g.result(), want)
            g = Guarded(out_len, True, shift)
            sh.place(_t(x), _t(starts), out_len, sc16=True, out=g.out)
            assert np.array_equal(g.result(), S.place_sc16(x, F, starts, out_len, scale))
    one = gfdm_amd.BurstShaper(F, scale=1.0).shape(_t(x[0]), sc16=True)
    assert tuple(one.shape) == (F, 2) and _h(one)[:-1, 0].tolist() == S.q16(SPECIALS).tolist()


@pytest.mark.parametrize("F", (3, 257, 721))
def test_sc16_normalised(F):
    """real scale: equal to the restatement with the largest component compared exactly; within 1 LSB of to_sc16; zeros stay zeros"""
    import torch
    import gfdm_amd
    rng = np.random.default_rng(300 + F)
    for scale, peak, n in ((1.0, 0.9 * 2048, 7), (0.37, 32767, 1), (250.0, 100.5, 7)):
        sh = gfdm_amd.BurstShaper(F, 5, 1, scale)
        x = _frames(rng, n, F) * np.float32(3.7)
        top = S.live_top(x, F, scale)
        ws = torch.zeros(sh.workspace_bytes(n, n * sh.slot_len()), dtype=torch.uint8, device="cuda:0")
        want = S.shape_sc16(x, F, 5, 1, scale, peak)
        for shift in _shifts(True):
            g = Guarded(want.shape[0], True, shift)
            sh.shape(_t(x), sc16=True, peak=peak, out=g.out, workspace=ws)
            got = g.result()
            assert np.array_equal(got, want)
            g_dev, top_dev = _h(ws[:8].view(torch.float32))
            assert top_dev == top and g_dev == S.gain(peak, top)
        lsb = np.abs(got.astype(np.int32) - gfdm_amd.to_sc16(S.shape_c64(x, F, 5, 1, 1.0), peak).astype(np.int32))
        assert lsb.max() <= 1
        starts, out_len = _place_starts(F, n, 5, 2)
        g = Guarded(out_len, True, 2)
        sh.place(_t(x), _t(starts), out_len, sc16=True, peak=peak, out=g.out)
        got = g.result()
        assert np.array_equal(got, S.place_sc16(x, F, starts, out_len, scale, None, peak))
        assert np.abs(got.astype(np.int32) - gfdm_amd.to_sc16(S.place_c64(x, F, starts, out_len, 1.0), peak).astype(np.int32)).max() <= 1
        zeros = sh.place(_t(np.zeros_like(x)), _t(starts), out_len, sc16=True, peak=peak)
        assert tuple(zeros.shape) == (out_len, 2) and not _h(zeros).any()


def test_host_flavour_equals_device_flavour():
    import gfdm_amd
    F, n = 257, 7
    rng = np.random.default_rng(13)
    x = _frames(rng, n, F) * np.float32(50)
    sh = gfdm_amd.BurstShaper(F, 1, 5, 0.6 - 0.3j)
    starts, out_len = _place_starts(F, n, 5, 3)
    for kw in (dict(), dict(sc16=True), dict(sc16=True, peak=1843.2)):
        host = sh.shape(x, **kw)
        assert isinstance(host, np.ndarray) and host.dtype == (np.int16 if kw else np.complex64)
        assert np.array_equal(host, _h(sh.shape(_t(x), **kw)))
        for count in (None, 3):
            host = sh.place(x, starts, out_len, count=count, **kw)
            assert np.array_equal(host, _h(sh.place(_t(x), _t(starts), out_len, count=count, **kw)))
            assert host.shape == ((out_len, 2) if kw else (out_len,)) and host.any()
    # a list of ports: one call, and one normalisation, per port
    ports = sh.shape([x, 2 * x], sc16=True, peak=1000)
    assert len(ports) == 2 and np.array_equal(ports[0], ports[1]) and np.array_equal(ports[0], sh.shape(x, sc16=True, peak=1000))
    out = np.zeros((out_len, 2), np.int16)
    assert sh.place(x, starts, out_len, sc16=True, out=out) is out and out.any()
    assert sh.place(x[:0], starts[:0], 9).tolist() == [0] * 9 and sh.shape(x[:0]).size == 0


def test_graph_replay():
    """the device place, sc16 and normalised, with a device count, captured once and replayed three times on other frames and counts: each
    replay equals the eager call (a peak or a gap left over from the replay before would show)"""
    import torch
    import gfdm_amd
    F, n = 257, 7
    rng = np.random.default_rng(17)
    sh = gfdm_amd.BurstShaper(F, scale=1.5)
    starts, out_len = _place_starts(F, n, 5, 3)
    ds = _t(starts)
    frames = torch.zeros(n, F, dtype=torch.complex64, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    gout = torch.zeros(out_len, 2, dtype=torch.int16, device="cuda:0")
    ws = torch.zeros(sh.workspace_bytes(n, out_len), dtype=torch.uint8, device="cuda:0")

    def call(out, w):
        return sh.place(frames, ds, out_len, count=count, sc16=True, peak=2000.0, out=out, workspace=w)

    frames.copy_(_t(_frames(rng, n, F)))
    count.fill_(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        call(gout, ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(gout, ws)
    # amplitudes 40, 1, 5 (a stale maximum would keep 40), counts 7, 5, 2; in the last one the largest sample sits in a frame beyond count
    for amp, cnt in ((40.0, n), (1.0, 5), (5.0, 2)):
        x = _frames(rng, n, F) * np.float32(amp)
        if cnt == 2:
            x[4, 9] = 1e3
        frames.copy_(_t(x))
        count.fill_(cnt)
        graph.replay()
        torch.cuda.synchronize()
        replayed = _h(gout)
        eager = _h(call(None, None))
        assert np.array_equal(replayed, eager), (amp, cnt)
        assert np.array_equal(replayed, S.place_sc16(x, F, starts, out_len, 1.5, cnt, 2000.0))
        assert np.abs(replayed).max() in (1999, 2000)


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_back_on_the_device(fmt):
    """transmit -> BurstShaper.place at irregular starts -> BurstSync.detect -> demodulate_bursts, nothing leaving the device in between;
    through complex64 and through normalised sc16 (the int16 tensor goes into detect and the receivers as it is).
    Yardsticks: frame_start == starts + cp_len and count == n_bursts exactly; the symbols against burst_receive_cases.restatement on the host
    copy of the very stream the shaper wrote (so quantisation is in the yardstick too), with the bounds of tests/test_burst_receive_gpu.py
    (_accept: fused vs the two-step chain within TOL, the chain vs float64 within TOL, fused vs float64 within twice the chain's distance);
    the QPSK decisions equal the transmitted symbols, for ZF + 2 IC rounds on the advanced receiver and the matched filter on the plain one.
    Preconditions (decision margin, threshold margin) are asserted on the restatement here and, without a device, in
    tests/test_burst_shaper.py::test_loop_back_preconditions."""
    import gfdm_amd
    from burst_detect_ref import nms_maxima, ref_ac_ic
    c = S.loop_case()
    M, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    assert tx.output_vector_size() == c["frame_len"]
    frames = tx.transmit(_t(c["sym"]))
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < TOL           # the frames the CPU-side preconditions were checked on
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=S.LOOP_SCALE)
    dstarts = _t(c["starts"])
    kw = dict(sc16=True, peak=S.LOOP_PEAK) if fmt == "sc16" else {}
    ds = sh.place(frames, dstarts, c["out_len"], **kw)[0]
    s_host = gfdm_amd.from_sc16(_h(ds)) if fmt == "sc16" else _h(ds)
    want = (S.place_sc16 if fmt == "sc16" else S.place_c64)(_h(frames[0]), c["frame_len"], c["starts"], c["out_len"], S.LOOP_SCALE, **({"peak": S.LOOP_PEAK} if kw else {}))
    assert np.array_equal(_h(ds), want)

    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, S.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    _, ic = ref_ac_ic(s_host, K, c["pcp"])
    assert np.min(np.abs(ic[nms_maxima(ic, c["min_distance"])] - S.LOOP_THRESHOLD)) >= 1e-3          # precondition
    assert int(r["count"][0]) == nb
    assert np.array_equal(_h(r["frame_start"])[:nb], c["starts"] + c["pcp"])
    assert np.all(_h(r["frame_start"])[nb:] == -1)

    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    rxs = (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points()))
    offs, rot = r["frame_start"][:nb].contiguous(), r["sc_rot"][:nb].contiguous()
    e = virtual_bursts(s_host, _h(offs), _h(rot), 0, c["F"])
    for rx, it in zip(rxs, (None, 2)):
        tag = "loop_%s_%s" % (fmt, "ic" if it else "mf")
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        out = _h(rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"]))
        assert out.shape == (nb + 3, A * M) and not out[nb:].any()
        fused = out[:nb]
        bursts = gfdm_amd.BurstExtractor(c["F"], 0, True).extract(ds, offs, None, rot)
        a = _h(rx.demodulate_estimated(bursts, bursts.view(-1), preamble_stride=c["F"]))
        b, margin = restatement(c, e, it)
        if it is None:
            margin = float(np.min(R.decision_margin(b, R.qpsk_points(), "qpsk")))
        assert margin >= MARGIN                                                                       # precondition
        e_a, e_ab, e_fb = rel_err(fused, a), rel_err(a, b), rel_err(fused, b)
        print("%s: rel_err(fused, chain) %.3e rel_err(chain, f64) %.3e rel_err(fused, f64) %.3e margin %.3f" % (tag, e_a, e_ab, e_fb, margin))
        check_err("shaper_" + tag + "_vs_chain", e_a, TOL)
        check_err("shaper_" + tag + "_chain_vs_f64", e_ab, TOL)
        check_err("shaper_" + tag + "_vs_f64", e_fb, 2 * e_ab)
        assert np.array_equal(fused.real > 0, c["sym"].real > 0) and np.array_equal(fused.imag > 0, c["sym"].imag > 0)
