"""GPU tests of the symbol mapper (contract in include/gfdm_hip.h, gfdm_hip_symbol_mapper).  The yardstick is the numpy restatement of
tests/symbol_mapper_ref.py (float64 on the float32 inputs), never the code under test:
  map:     equal, bit for bit;
  decode:  sign rules equal everywhere (zeros, NaN, infinities included); NEAREST equal on every symbol whose float64 decision margin is at
           least 1e-5 * max(1, |x|) -- the symbols left out are counted, printed, and at most 0.1 % of a case (the CPU test checks that the
           seeded inputs stay under that cap on the restatement alone); exact ties and non-finite inputs are known answers, without a guard;
  soft:    per element |got - ref| <= 8 * 2^-24 * |s_r| * (d0 + d1), d0 and d1 the two minima of the restatement: four roundings per
           distance, one for the difference, one for the scale, with room for the second order.  No guard and no exclusion: the bound holds
           where fp32 picks another minimiser.
Every output lies between guard words, inputs and outputs at every alignment one element allows."""
import numpy as np
import pytest

import burst_shaper_ref as B
import gfdm_ref as R
import symbol_mapper_ref as S
from conftest import have_gpu, rel_err

pytestmark = pytest.mark.gpu
GUARD = 16                                  # guard elements on either side of an output: a multiple of 16 bytes for every dtype
FILL = {"uint8": 0xA5, "float32": 777.0, "complex64": 7 + 7j}
NAMES = sorted(S.constellations())


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def mappers():
    import gfdm_amd
    return {name: gfdm_amd.SymbolMapper(points) for name, (points, _) in S.constellations().items()}


class Window:
    """n elements of `dtype` inside a larger device buffer, `shift` elements past a 16-byte boundary, guard words on either side"""

    def __init__(self, dtype, n, shift, content=None):
        import torch
        name = np.dtype(dtype).name
        self.lo, self.n = GUARD + shift, n
        self.buf = torch.full((self.lo + n + GUARD,), FILL[name], dtype=getattr(torch, name), device="cuda:0")
        self.view = self.buf[self.lo:self.lo + n]
        self.fill = _h(self.buf[:1]).copy()
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * np.dtype(dtype).itemsize) % 16
        if content is not None:
            self.view.copy_(_t(np.ascontiguousarray(content).ravel()))

    def rows(self, n_rows):
        return self.view.view(n_rows, -1)

    def result(self, n_rows):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.fill) and np.all(b[self.lo + self.n:] == self.fill), "guard words overwritten"
        return b[self.lo:self.lo + self.n].reshape(n_rows, -1)


def _check_decode(c, got, x=None, count=None, tag=""):
    """got against the restatement: sign rules everywhere; NEAREST where the margin clears the guard (the rest counted and printed)"""
    x = c["x"] if x is None else x
    want, margin = S.decode(x, c["points"], c["rule"], count)
    assert got.shape == want.shape and got.dtype == np.uint8
    if c["rule"] != "nearest":
        assert np.array_equal(got, want), (c["name"], tag)
        return
    ok = S.guarded(x, margin)
    left_out = int(np.count_nonzero(~ok))
    print("%s %s%dx%d: %d of %d symbols inside the guard" % (c["name"], tag, x.shape[0], x.shape[1], left_out, x.size))
    assert left_out <= S.GUARD_CAP * x.size
    gi, wi = S.unpack(got, x.shape[1], c["k"]), S.unpack(want, x.shape[1], c["k"])
    assert np.array_equal(gi[ok], wi[ok]), (c["name"], tag)
    assert np.array_equal(got & ~S.spare_mask(x.shape[1], c["k"]), np.zeros_like(got))          # the spare bits are written as 0


def _check_soft(c, got, scale, x=None, count=None, tag=""):
    x = c["x"] if x is None else x
    want, d0, d1 = S.soft(x, c["points"], scale, count)
    assert got.shape == want.shape and got.dtype == np.float32
    err, bound = np.abs(got.astype(np.float64) - want), S.soft_bound(scale, d0, d1)
    n = S.live(count, x.shape[0])
    worst = float(np.max(err[:n] / bound[:n])) if n else 0.0
    print("%s %s%dx%d soft: worst error %.3f of the bound" % (c["name"], tag, x.shape[0], x.shape[1], worst))
    assert np.all(err[:n] <= bound[:n]), (c["name"], tag, worst)
    assert not got[n:].any()


def _run_case(m, c, k_case):
    """the three operations on one case, inputs and outputs at alignments that go round with k_case"""
    n_rows, n_sym, k = c["n_rows"], c["n_sym"], c["k"]
    rb = S.row_bytes(n_sym, k)
    s_in, s_out, b_in, b_out, f_out = k_case % 2, (k_case // 2) % 2, (k_case + 1) % 4, k_case % 4, (k_case // 3) % 4
    assert m.row_bytes(n_sym) == rb
    # map
    w = Window(np.complex64, n_rows * n_sym, s_out)
    data = Window(np.uint8, n_rows * rb, b_in, c["data"])
    res = m.map(data.rows(n_rows), n_sym, out=w.view)
    assert res is w.view
    assert np.array_equal(w.result(n_rows).view(np.uint32), c["sym"].view(np.uint32)), (c["name"], n_rows, n_sym)
    # decode
    x = Window(np.complex64, n_rows * n_sym, s_in, c["x"])
    w = Window(np.uint8, n_rows * rb, b_out)
    m.decode(x.rows(n_rows), out=w.view)
    _check_decode(c, w.result(n_rows))
    # soft, with and without a scale
    scale = c["scale"] if k_case % 2 else None
    w = Window(np.float32, n_rows * n_sym * k, f_out)
    m.soft(x.rows(n_rows), scale=None if scale is None else _t(scale), out=w.view)
    _check_soft(c, w.result(n_rows), scale)


@pytest.mark.parametrize("name", NAMES)
def test_every_shape(name, mappers):
    """n_sym 1 .. 4097 by 1 and 7 rows; buffers at every alignment of one element (symbols off by one sample, bytes by 1, 2, 3, LLRs by 1, 2, 3
    floats) in turn; decode of the mapped symbols gives the bytes back"""
    m = mappers[name]
    points, rule = S.constellations()[name]
    assert m.decision_rule() == rule and m.bits_per_symbol() == S.bits_per_symbol(points)
    assert np.array_equal(m.points().view(np.uint32), points.view(np.uint32))
    for k_case, (n_rows, n_sym) in enumerate(S.shapes()):
        _run_case(m, S.case(name, n_rows, n_sym), k_case)
    c = S.case(name, 7, 65)
    back = _h(m.decode(m.map(_t(c["data"]), 65)))
    assert np.array_equal(back, c["data"])
    one = m.decode(_t(c["sym"][0]))                                          # a 1-D input is one row
    assert tuple(one.shape) == (S.row_bytes(65, c["k"]),) and np.array_equal(_h(one), c["data"][0])
    assert tuple(m.map(_t(c["data"][0]), 65).shape) == (65,) and tuple(m.soft(_t(c["x"][0])).shape) == (65 * c["k"],)


@pytest.mark.parametrize("name", S.MANY_ROWS_NAMES)
def test_many_rows(name, mappers):
    """5000 rows of 3 symbols and 32768 + 7 rows of 5: rows are not a grid dimension, a workgroup takes a stretch of the flat output
    whatever rows lie there (several hundred of them here)"""
    for k_case, (n_rows, n_sym) in enumerate(S.MANY_ROWS):
        _run_case(mappers[name], S.case(name, n_rows, n_sym), 5 + 6 * k_case)


@pytest.mark.parametrize("name", ("gr_qpsk", "psk8", "qam64"))
def test_count(name, mappers):
    """count None, 0, 3 of 7, n_rows + 5 and -1, as an int and as a device tensor: the rows from n_live on are zeros in all three outputs
    (their input holds what would show: NaN symbols, 0xFF bytes), the others are those of the full call"""
    import torch
    m = mappers[name]
    c = S.case(name, 7, 257)
    n_rows, n_sym, k = 7, 257, c["k"]
    full = [_h(m.map(_t(c["data"]), n_sym)), _h(m.decode(_t(c["x"]))), _h(m.soft(_t(c["x"]), _t(c["scale"])))]
    for cnt in (None, 0, 3, n_rows + 5, -1):
        n = S.live(cnt, n_rows)
        x, data = c["x"].copy(), c["data"].copy()
        x[n:], data[n:] = complex(np.nan, np.nan), 0xFF
        for count in ((cnt,) if cnt is None else (cnt, _t([cnt], torch.int64))):
            outs = (Window(np.complex64, n_rows * n_sym, 1), Window(np.uint8, n_rows * S.row_bytes(n_sym, k), 3), Window(np.float32, n_rows * n_sym * k, 1))
            m.map(_t(data), n_sym, count=count, out=outs[0].view)
            m.decode(_t(x), count=count, out=outs[1].view)
            m.soft(_t(x), _t(c["scale"]), count=count, out=outs[2].view)
            for w, whole in zip(outs, full):
                got = w.result(n_rows)
                assert np.array_equal(got[:n].view(np.uint8), whole[:n].view(np.uint8)) and not got[n:].any(), (cnt, whole.dtype)
            assert np.array_equal(outs[0].result(n_rows), S.map(data, n_sym, c["points"], cnt))
            _check_decode(c, outs[1].result(n_rows), x, cnt, "count %s " % cnt)
            _check_soft(c, outs[2].result(n_rows), c["scale"], x, cnt, "count %s " % cnt)


def test_ties_and_non_finite_inputs_are_known_answers(mappers):
    """exact ties on the integer 16-QAM grid go to the first index; NaN decodes to 0 under every rule, an infinite component to 0 under
    NEAREST and by its sign under the sign tests; a zero is not '> 0'.  No guard here."""
    x, want = S.tie_inputs()
    for n_rows in (1, 3):
        rows = np.tile(x, (n_rows, 1))
        got = _h(mappers["qam16_grid"].decode(_t(rows)))
        assert np.array_equal(S.unpack(got, x.size, 4), np.tile(want, (n_rows, 1)))
    sx, qpsk, bpsk, nearest = S.special_inputs()
    assert np.array_equal(S.unpack(_h(mappers["gr_qpsk"].decode(_t(sx[None, :]))), sx.size, 2)[0], qpsk)
    assert np.array_equal(S.unpack(_h(mappers["gr_bpsk"].decode(_t(sx[None, :]))), sx.size, 1)[0], bpsk)
    for name in NAMES:
        if S.constellations()[name][1] == "nearest":
            got = _h(mappers[name].decode(_t(sx[None, :nearest.size])))
            assert np.array_equal(S.unpack(got, nearest.size, mappers[name].bits_per_symbol())[0], nearest), name


@pytest.mark.parametrize("name", ("gr_qpsk", "pygfdm_qpsk", "psk8", "grid256"))
def test_poison_stays_in_its_symbol(name, mappers):
    """one NaN symbol and one infinite symbol in a batch: the call returns 0 and every other output element -- every other symbol's bits,
    every other symbol's k soft bits -- is bit-equal to the same call without them"""
    m = mappers[name]
    c = S.case(name, 7, 65)
    k, n_sym = c["k"], 65
    x = c["x"].copy()
    x[2, 17], x[5, 64] = complex(np.nan, 0.25), complex(0.5, -np.inf)
    clean = np.ones(x.shape, bool)
    clean[2, 17] = clean[5, 64] = False
    dx, dc, ds = _t(x), _t(c["x"]), _t(c["scale"])
    got, ref = _h(m.decode(dx)), _h(m.decode(dc))
    assert np.array_equal(S.unpack(got, n_sym, k)[clean], S.unpack(ref, n_sym, k)[clean])
    got, ref = _h(m.soft(dx, ds)).view(np.uint32).reshape(7, n_sym, k), _h(m.soft(dc, ds)).view(np.uint32).reshape(7, n_sym, k)
    assert np.array_equal(got[clean], ref[clean])
    assert np.array_equal(m.decode(x), _h(m.decode(dx)))                      # ... and the host flavour returns 0 as well


@pytest.mark.parametrize("name", ("gr_qpsk", "psk8", "qam64"))
def test_split_invariance(name, mappers):
    """rows [a, b) alone are the slice of the whole call, bit for bit, in all three operations"""
    m = mappers[name]
    c = S.case(name, 7, 257)
    n_sym = 257
    dd, dx, ds = _t(c["data"]), _t(c["x"]), _t(c["scale"])
    whole = [_h(m.map(dd, n_sym)), _h(m.decode(dx)), _h(m.soft(dx, ds))]
    for a, b in ((0, 1), (1, 4), (3, 7), (6, 7)):
        part = [_h(m.map(dd[a:b], n_sym)), _h(m.decode(dx[a:b])), _h(m.soft(dx[a:b], ds[a:b]))]
        for p, w in zip(part, whole):
            assert np.array_equal(p.view(np.uint8), w[a:b].view(np.uint8)), (a, b, w.dtype)


@pytest.mark.parametrize("name", ("gr_bpsk", "gr_qpsk", "psk8", "grid256"))
def test_host_flavour_equals_device_flavour(name, mappers):
    m = mappers[name]
    c = S.case(name, 7, 63)
    for count in (None, 3):
        host = [m.map(c["data"], 63, count=count), m.decode(c["x"], count=count), m.soft(c["x"], c["scale"], count=count), m.soft(c["x"], count=count)]
        dev = [m.map(_t(c["data"]), 63, count=count), m.decode(_t(c["x"]), count=count), m.soft(_t(c["x"]), _t(c["scale"]), count=count),
               m.soft(_t(c["x"]), count=count)]
        for h, d in zip(host, dev):
            assert isinstance(h, np.ndarray) and h.shape == tuple(d.shape) and np.array_equal(h.view(np.uint8), _h(d).view(np.uint8))
    assert host[0].dtype == np.complex64 and host[1].dtype == np.uint8 and host[2].dtype == np.float32
    assert m.decode(c["x"][:0]).shape == (0, S.row_bytes(63, c["k"])) and tuple(m.decode(_t(c["x"][:0])).shape) == (0, S.row_bytes(63, c["k"]))
    out = np.zeros((7, S.row_bytes(63, c["k"])), np.uint8)
    assert m.decode(c["x"], out=out) is out and out.any()
    with pytest.raises(TypeError):
        m.decode(_t(c["x"]), out=out)
    with pytest.raises(RuntimeError):
        m.map(c["data"][:, :-1], 63)


@pytest.mark.parametrize("name", ("gr_qpsk", "qam64"))
def test_graph_replay(name, mappers):
    """one linear capture of decode (a single kernel on the capturing stream: no memset, no second branch) with a device count, replayed
    after the symbols and the count changed on the device: the restatement both times, zeros where the replay before had bytes"""
    import torch
    m = mappers[name]
    n_rows, n_sym = 7, 257
    c = S.case(name, n_rows, n_sym)
    x = torch.zeros(n_rows, n_sym, dtype=torch.complex64, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    out = torch.zeros(n_rows, S.row_bytes(n_sym, c["k"]), dtype=torch.uint8, device="cuda:0")
    x.copy_(_t(c["x"]))
    count.fill_(n_rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        m.decode(x, count=count, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.decode(x, count=count, out=out)
    for cnt, seed in ((n_rows, 0), (3, 1), (5, 2)):
        xs = S.case(name, n_rows, n_sym, seed)["x"]
        x.copy_(_t(xs))
        count.fill_(cnt)
        graph.replay()
        torch.cuda.synchronize()
        _check_decode(c, _h(out), xs, cnt, "replay count %d " % cnt)
        assert _h(out)[:cnt].any() and not _h(out)[cnt:].any()


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_on_the_device(fmt, mappers):
    """payload bytes -> map -> transmit -> place -> detect -> demodulate_bursts -> decode -> payload bytes on burst_shaper_ref.loop_case(),
    whose threshold and decision-margin preconditions tests/test_burst_shaper.py checks for exactly these symbols; complex64 and sc16
    streams, the matched filter on the plain receiver and ZF + 2 IC rounds on the advanced one.  The first nb rows are the payload, the
    max_bursts - nb spare rows zero bytes; nothing leaves the device in between."""
    import gfdm_amd
    c = B.loop_case()
    M, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym = A * M
    pts = R.qpsk_points().astype(np.complex64)
    payload = S.pack(S.indices(c["sym"], pts, "qpsk"), 2)
    assert payload.shape == (nb, S.row_bytes(n_sym, 2)) and np.array_equal(S.map(payload, n_sym, pts).view(np.uint32), c["sym"].view(np.uint32))
    m = mappers["gr_qpsk"]
    sym = m.map(_t(payload), n_sym)
    assert np.array_equal(_h(sym).view(np.uint32), c["sym"].view(np.uint32))          # to the bit: the loop case's symbols ARE the handle's points
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < 1e-5            # the frames the CPU-side preconditions were checked on
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    kw = dict(sc16=True, peak=B.LOOP_PEAK) if fmt == "sc16" else {}
    ds = sh.place(frames, _t(c["starts"]), c["out_len"], **kw)[0]
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    for rx in (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())):
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
        assert tuple(demod.shape) == (nb + 3, n_sym)
        got = _h(m.decode(demod, count=r["count"]))
        assert int(r["count"][0]) == nb
        assert got.shape == (nb + 3, payload.shape[1]) and np.array_equal(got[:nb], payload) and not got[nb:].any()
        llr = _h(m.soft(demod, count=r["count"]))
        assert np.array_equal(np.packbits(llr[:nb] < 0, axis=1), payload) and not llr[nb:].any()
