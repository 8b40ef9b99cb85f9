"""GPU tests of the sc16 capture format (int16 I/Q; contract in include/gfdm_hip.h).  Throughout q = to_sc16(stream) and f = from_sc16(q):
the same values as int16 and as complex64.
  1. the contract: every output of every call on q is bit-equal (np.array_equal) to the existing call on f -- detect, auto_correlate,
     find_frame_start(_at), extract, demodulate_bursts on every kernel family, device and host flavours;
  2. alignment: the same with the capture at sample 1 of a larger device tensor (4-byte, not 8-byte aligned);
  3. the yardsticks: detect(q) against the pygfdm fixtures, demodulate_bursts(q) against the float64 restatement on f and the transmitted
     symbols (tests/test_sc16.py holds the preconditions: the restatements stay decided under the 12-bit quantisation);
  4. detect -> demodulate_bursts on q in one captured graph, replayed on a second capture, against the eager complex64 chain."""
import functools

import numpy as np
import pytest

import gfdm_ref as R
from burst_detect_ref import detect_names, load_detect
from burst_receive_cases import CASES, MARGIN, make_case, restatement, virtual_bursts
from conftest import check_err, have_gpu, rel_err
from test_burst_detect_gpu import EDGE_STREAMS, EDGE_THRESHOLD, edge_stream
from test_burst_gpu import load_sync
from test_burst_receive_gpu import KERNEL, _detect_stream, _receivers, _same_signs

pytestmark = pytest.mark.gpu
OUT = ("frame_start", "coarse", "cfo", "metric", "sc_rot")
TOL = 1e-5                                   # tests/test_burst_receive_gpu.py's
EDGES = [e for e in EDGE_STREAMS if e[:2] in ((15, 7), (64, 256), (64, 257))]           # odd K; segment_ic; tile_ic per segment


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _bits(a):
    """bit patterns: equal NaNs compare equal, -0 and +0 do not"""
    a = np.ascontiguousarray(_h(a))
    return a.view(np.uint32) if a.dtype.kind in "fc" else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _pair(stream):
    """(q, f): the stream as sc16, shape (n, 2), and the same values as complex64"""
    import gfdm_amd
    q = gfdm_amd.to_sc16(stream)
    return q, gfdm_amd.from_sc16(q)


def _at_sample_1(q):
    """q as the slice from sample 1 of a larger device tensor: its base is 4-byte, not 8-byte aligned"""
    import torch
    big = torch.full((q.shape[0] + 1, 2), 12345, dtype=torch.int16, device="cuda:0")
    big[1:] = _t(q)
    view = big[1:]
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    return view


def _captures(q):
    """the sc16 capture in every form a call takes it: device (n, 2), device flat, device at sample 1 of a larger tensor, host (n, 2), host flat"""
    return [("device", _t(q)), ("device flat", _t(q).view(-1)), ("device at sample 1", _at_sample_1(q)), ("host", q), ("host flat", q.ravel())]


def _assert_results_equal(r, want, tag):
    assert int(_h(r["count"]).ravel()[0]) == int(_h(want["count"]).ravel()[0]), tag
    for k in OUT:
        assert _same(r[k], want[k]), (tag, k)


@functools.lru_cache(maxsize=None)
def _detect_fixture(name):
    g = load_detect(name)
    q, f = _pair(g["stream"])
    return g, q, f


def _sync(g):
    import gfdm_amd
    return gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], g["window_len"])


# ---- 1 + 2: bit-equality, aligned or not, device and host ----
@pytest.mark.parametrize("name", detect_names())
def test_detect_is_bit_equal_on_the_fixtures(name):
    g, q, f = _detect_fixture(name)
    sync = _sync(g)
    args = (g["threshold"], g["min_distance"], g["lead"])
    want = sync.detect(_t(f), *args)
    for tag, cap in _captures(q):
        _assert_results_equal(sync.detect(cap, *args), want, tag)


def test_detect_is_bit_equal_with_too_few_and_too_many_slots():
    g, q, f = _detect_fixture("k64_12b")
    sync = _sync(g)
    args = (g["threshold"], g["min_distance"], g["lead"])
    n = g["peaks"].size
    for nb in (n - 3, n + 5, 0):
        want = sync.detect(_t(f), *args, max_bursts=nb)
        assert int(want["count"][0]) == n and want["coarse"].numel() == nb
        for tag, cap in _captures(q):
            _assert_results_equal(sync.detect(cap, *args, max_bursts=nb), want, (tag, nb))
    spare = _h(sync.detect(_t(q), *args, max_bursts=n + 5)["frame_start"])
    assert np.all(spare[:n] >= 0) and np.all(spare[n:] == -1)


@pytest.mark.parametrize("K,cp,Rd,nb,n", EDGES)
def test_detect_is_bit_equal_on_the_edge_streams(K, cp, Rd, nb, n):
    import gfdm_amd
    c = edge_stream(K, cp, Rd, nb, n)
    q, f = _pair(c["stream"])
    sync = gfdm_amd.BurstSync(K, cp, c["preamble"], c["window_len"])
    for thr in (EDGE_THRESHOLD, 0.3):                        # the lower threshold: noise peaks too
        want = sync.detect(_t(f), thr, Rd, c["lead"])
        assert int(want["count"][0]) >= nb
        for tag, cap in _captures(q):
            _assert_results_equal(sync.detect(cap, thr, Rd, c["lead"]), want, (tag, thr))


def test_auto_correlate_is_bit_equal():
    import gfdm_amd
    g, q, f = _detect_fixture("k64_12b")
    e = edge_stream(*EDGES[0])
    assert EDGES[0][:2] == (15, 7)
    eq, ef = _pair(e["stream"])
    for K, cp, pre, q_, f_ in ((g["K"], g["cp_len"], g["preamble"], q, f), (15, 7, e["preamble"], eq, ef)):
        n = f_.size
        whole = gfdm_amd.BurstSync(K, cp, pre, n)                                   # the stream as one window
        grid = gfdm_amd.BurstSync(K, cp, pre, 2 * K + cp + 300)                      # windows at odd and even starts
        for sync, kw in ((whole, {}), (grid, dict(first=1, stride=333, n_windows=5))):
            ac, ic = sync.auto_correlate(_t(f_), **kw)
            assert float(ic.max()) > 0.5
            for tag, cap in _captures(q_):
                ac16, ic16 = sync.auto_correlate(cap, **kw)
                assert _same(ac16, ac) and _same(ic16, ic), (K, tag)
    # an all-zero stretch: ac = 0 there, as for complex64
    z = q.copy()
    z[1000:1000 + 4 * g["K"]] = 0
    whole = gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], z.shape[0])
    ac, ic = whole.auto_correlate(_t(z))
    assert np.all(_h(ac)[0, 1000:1000 + 2 * g["K"]] == 0) and np.all(np.isfinite(_h(ac)))
    ac32, ic32 = whole.auto_correlate(_t(gfdm_amd.from_sc16(z)))
    assert _same(ac, ac32) and _same(ic, ic32)


@pytest.mark.parametrize("name", ["k31_cp16_cfom02_20db", "k64_cp300_cfom02_26db"])
def test_find_frame_start_is_bit_equal(name):
    import gfdm_amd
    g = load_sync(name)
    q, f = _pair(g["stream"])
    sync = gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], g["window_len"])
    grid = dict(first=g["first"] - 2, stride=3, n_windows=4)                         # starts of both parities
    starts = np.array([g["first"], 0, g["first"] + 1, -5, 10 ** 9, g["first"] - 7], np.int64)    # ... and clamped ones
    want = sync.find_frame_start(_t(f), **grid)
    want_at = sync.find_frame_start_at(_t(f), _t(starts))
    assert np.all(_h(want["coarse"]) >= 0) and np.all(_h(want_at["coarse"]) >= 0)
    for tag, cap in _captures(q):
        r = sync.find_frame_start(cap, **grid)
        r_at = sync.find_frame_start_at(cap, _t(starts) if hasattr(cap, "is_cuda") else starts)
        for k in OUT:
            assert _same(r[k], want[k]) and _same(r_at[k], want_at[k]), (tag, k)


def test_extract_is_bit_equal_and_zero_outside_the_capture():
    import gfdm_amd
    c = make_case(9, 64, 2, 52, 7, 0)
    q, f = _pair(c["stream"])
    n, F, backoff = f.size, c["F"], 17
    # the first burst starts 12 samples before the capture, the last one runs 30 samples past it
    offs = np.concatenate(([5], c["starts"][1:4], c["starts"][4:6] + 1, [n - F + backoff + 30])).astype(np.int64)
    assert set(offs % 2) == {0, 1}
    rng = np.random.default_rng(3)
    scale = (0.5 + rng.random(offs.size)).astype(np.float32)
    scale[1] = 1 / 32768
    rot = np.resize(c["sc_rot"], offs.size).astype(np.complex64)
    for correct in (True, False):
        ex = gfdm_amd.BurstExtractor(F, backoff, correct)
        for sc, rt in ((None, None), (scale, None), (None, rot), (scale, rot)):
            d = lambda v: None if v is None else _t(v)
            want = ex.extract(_t(f), _t(offs), d(sc), d(rt))
            for tag, cap in _captures(q):
                dev = hasattr(cap, "is_cuda")
                got = ex.extract(cap, _t(offs) if dev else offs, d(sc) if dev else sc, d(rt) if dev else rt)
                assert _same(got, want), (tag, correct, sc is None, rt is None)
            w = _h(want)
            assert np.all(w[0, :12] == 0) and np.all(w[-1, -30:] == 0)                               # outside the capture: zeros
            if sc is None and (rt is None or not correct):                                           # ... and inside it, the samples
                assert np.array_equal(w[0, 12:], f[:F - 12]) and np.array_equal(w[-1, :-30], f[n - F + 30:])
    # unit full scale through the extractor's own scale: sample values / 32768
    ex = gfdm_amd.BurstExtractor(F, 0, False)
    unit = _h(ex.extract(_t(q), _t(offs[1:2]), _t(np.array([1 / 32768], np.float32))))
    assert np.array_equal(unit[0], (f[offs[1]:offs[1] + F] / np.float32(32768)).astype(np.complex64))
    # the capture from its sample 1 on, the offsets one lower: the same bursts (those inside the capture)
    inner = offs[1:-1]
    ex = gfdm_amd.BurstExtractor(F, backoff, True)
    want = ex.extract(_t(f), _t(inner), _t(scale[1:-1]), _t(rot[1:-1]))
    shifted = _t(q)[1:]
    assert shifted.data_ptr() % 8 == 4
    assert _same(ex.extract(shifted, _t(inner - 1), _t(scale[1:-1]), _t(rot[1:-1])), want)


def _burst_offsets(c):
    """the case's bursts, and each once more one sample late (garbage to the receiver, but a fetch at the other parity)"""
    offs = np.concatenate((c["starts"], c["starts"] + 1)).astype(np.int64)
    assert set(offs % 2) == {0, 1}
    return offs, np.concatenate((c["sc_rot"], c["sc_rot"])).astype(np.complex64)


@pytest.mark.parametrize("generic", [False, True], ids=["own_family", "generic_forced"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_demodulate_bursts_is_bit_equal(name, generic):
    M, K, L, A, nb, seed = CASES[name]
    c = make_case(M, K, L, A, nb, seed)
    q, f = _pair(c["stream"])
    offs, rot = _burst_offsets(c)
    n = offs.size
    kw = dict(preamble_offset=c["pre_off"])
    for rx in _receivers(c, generic or name == "generic_5_32"):
        assert rx.kernel_name().startswith("generic") if generic else rx.kernel_name() in KERNEL[name]
        want = rx.demodulate_bursts(_t(f), _t(offs), _t(rot), **kw)
        assert np.all(np.abs(_h(want)[:nb]).max(axis=1) > 0.1)
        cnt = np.array([n - 2], np.int64)
        want_cnt = rx.demodulate_bursts(_t(f), _t(offs), _t(rot), _t(cnt), **kw)
        assert np.all(_bits(want_cnt)[n - 2:] == 0)
        want_edge = rx.demodulate_bursts(_t(f), _t(offs + 17), None, backoff=17, cfo_correction=False, **kw)
        for tag, cap in _captures(q):
            dev = hasattr(cap, "is_cuda")
            d = (lambda v: _t(v)) if dev else (lambda v: v)
            assert _same(rx.demodulate_bursts(cap, d(offs), d(rot), **kw), want), tag                      # count None
            assert _same(rx.demodulate_bursts(cap, d(offs), d(rot), d(cnt), **kw), want_cnt), tag          # count given
            assert _same(rx.demodulate_bursts(cap, d(offs + 17), None, backoff=17, cfo_correction=False, **kw), want_edge), tag
        # the capture from its sample 1 on, the offsets one lower: the same bursts
        shifted = _t(q)[1:]
        assert shifted.data_ptr() % 8 == 4
        assert _same(rx.demodulate_bursts(shifted, _t(offs - 1), _t(rot), **kw), want)


# ---- 3: against the yardsticks, not only against itself ----
@pytest.mark.parametrize("name", detect_names())
def test_detect_on_sc16_reproduces_pygfdm(name):
    """peaks and core starts exactly; cfo within 2e-4 and metric within 1e-3 of the golden values: the bounds absorb the 12-bit
    quantisation (float64 restatement on the quantised streams, tests/test_sc16.py: cfo moves by at most 8.5e-5, metric by 1.4e-4)
    on top of the fp32 error tests/test_burst_detect_gpu.py allows (1e-4, 1e-5)"""
    g, q, _ = _detect_fixture(name)
    r = _sync(g).detect(q, g["threshold"], g["min_distance"], g["lead"])
    n = g["peaks"].size
    print(name, "count", r["count"], "of", n)
    assert r["count"] == n
    assert np.array_equal(r["frame_start"][:n], g["core_starts"])
    assert np.all(r["frame_start"][n:] == -1)
    if n:
        d_cfo, d_met = np.max(np.abs(r["cfo"][:n] - g["cfo"])), np.max(np.abs(r["metric"][:n] - g["metric"]))
        print("   cfo off the golden by %.3e, metric by %.3e, coarse off the golden peaks by %d" % (d_cfo, d_met, np.max(np.abs(r["coarse"][:n] - g["peaks"]))))
        assert d_cfo < 2e-4 and d_met < 1e-3
        assert np.max(np.abs(r["coarse"][:n] - g["peaks"])) <= 1             # as for complex64: a neighbour where the ic plateau is flat


@pytest.mark.parametrize("name", sorted(CASES))
def test_demodulate_bursts_on_sc16_agrees_with_the_restatement(name):
    M, K, L, A, nb, seed = CASES[name]
    c = make_case(M, K, L, A, nb, seed)
    q, f = _pair(c["stream"])
    e = virtual_bursts(f, c["starts"], c["sc_rot"], 0, c["F"])
    for rx, it in zip(_receivers(c, name == "generic_5_32"), (None, 2)):
        assert rx.kernel_name() in KERNEL[name]
        b, margin = restatement(c, e, it)
        assert margin > MARGIN
        got = _h(rx.demodulate_bursts(_t(q), _t(c["starts"]), _t(c["sc_rot"]), preamble_offset=c["pre_off"]))
        err = rel_err(got, b)
        print("%s %s: rel_err(sc16, restatement) %.3e margin %.3f" % (name, "ic" if it else "dem", err, margin))
        check_err("burst_rx_sc16_vs_f64_%s_%s" % (name, "ic" if it else "dem"), err, TOL)
        assert _same_signs(got, b)
        if it:                # (the plain receiver keeps the self-interference the cancellation rounds remove: its yardstick is the restatement)
            assert np.array_equal(got.real > 0, c["sym"].real > 0) and np.array_equal(got.imag > 0, c["sym"].imag > 0)


# ---- 4: the chain, captured once ----
def test_detect_then_demodulate_on_sc16_in_one_graph():
    import torch
    import gfdm_amd
    M, K, L, A, slots = 9, 64, 2, 52, 24
    a = _detect_stream(M * K + L, slots)
    b = _detect_stream(4711, slots - 9)
    F, pcp, cp, N = a["F"], a["pcp"], a["cp"], a["N"]
    sb = np.zeros_like(a["stream"])
    sb[:b["stream"].size] = b["stream"]
    (qa, fa), (qb, fb) = _pair(a["stream"]), _pair(sb)
    lead, nmax = pcp + K // 2, slots + 8
    sync = gfdm_amd.BurstSync(K, pcp, a["core"], lead + 3 * K + pcp)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, a["core"])
    adv = gfdm_amd.AdvancedReceiver(M, K, L, a["taps"], a["smap"], 2, R.qpsk_points())
    adv.configure_frames(2 * K + cp + N, 2 * K + cp, a["smap"], True)
    adv.set_channel_estimator(est)

    def chain(ds, out=None):
        r = sync.detect(ds, 0.5, F // 2, lead, max_bursts=nmax)
        return r, adv.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"], out=out)

    eager = []
    for f_, sym, cnt in ((fa, a["sym"], slots), (fb, b["sym"], slots - 9)):           # the eager complex64 chain
        r, out = chain(_t(f_))
        o = _h(out)
        assert int(r["count"][0]) == cnt
        assert np.array_equal(o[:cnt].real > 0, sym.real > 0) and np.array_equal(o[:cnt].imag > 0, sym.imag > 0) and np.all(_bits(o[cnt:]) == 0)
        eager.append((_h(r["frame_start"]), o))

    dq = _t(qa)
    gout = torch.empty(nmax, A * M, dtype=torch.complex64, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        chain(dq, gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rg, _ = chain(dq, gout)
    for q_, (fs, o), cnt in ((qa, eager[0], slots), (qb, eager[1], slots - 9)):
        dq.copy_(_t(q_))                                # the second capture goes into the same buffer
        graph.replay()
        torch.cuda.synchronize()
        assert int(rg["count"][0]) == cnt
        assert np.array_equal(_h(rg["frame_start"]), fs) and _same(gout, o)

