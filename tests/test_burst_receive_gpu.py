"""GPU tests of demodulate_bursts: the receivers that read detected bursts straight from the capture (contract in include/gfdm_hip.h).
Yardsticks, for the plain receiver and the IC receiver with 2 iterations:
  (A) the two-step path on the same inputs, BurstExtractor.extract then demodulate_estimated: within TOL = 1e-5, the project's bound for
      fused-versus-chain comparisons (both fetch through one device function and differ by the compiler's contraction only);
  (B) the float64 restatement of tests/burst_receive_cases.py: the fused path may be at most twice as far from it as (A) is (measured in
      the same test; the factor 2 covers contraction differences at the load);
  (C) precondition, asserted on (B): every decided symbol further than 0.1 from a QPSK decision boundary."""
import numpy as np
import pytest

import gfdm_ref as R
from burst_receive_cases import CASES, MARGIN, make_case, restatement, virtual_bursts
from conftest import check_err, have_gpu, rel_err
from gfdm_amd.filters import get_frequency_domain_filter

pytestmark = pytest.mark.gpu
TOL = 1e-5


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
    return np.ascontiguousarray(a).view(np.uint32)


def _receivers(c, generic=False):
    """(plain receiver, IC receiver with 2 iterations), frame layout and estimator attached"""
    import contextlib
    import gfdm_amd
    M, K, L, A = c["M"], c["K"], c["L"], c["A"]
    with (gfdm_amd.generic_family_for_testing() if generic else contextlib.nullcontext()):
        est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
        rxs = (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points()))
    for rx in rxs:
        rx.configure_frames(c["F"], c["pre_off"] + 2 * K + c["cp"], c["smap"], True)
        rx.set_channel_estimator(est)
    return rxs


def _two_step(rx, c, ds, offs, rot, backoff=0, correction=True):
    """yardstick (A)"""
    import gfdm_amd
    ex = gfdm_amd.BurstExtractor(c["F"], backoff, correction)
    bursts = ex.extract(ds, offs, None, rot)
    return rx.demodulate_estimated(bursts, bursts.view(-1)[c["pre_off"]:], preamble_stride=c["F"])


def _same_signs(got, b):
    """the symbols of (B) are recovered: every component of `got` has the sign of (B)'s, wherever (B)'s is not within 1e-3 of zero (the
    plain receiver keeps the self-interference that the cancellation rounds remove, so its yardstick is (B), not the transmitted symbols)"""
    re, im = np.abs(b.real) > 1e-3, np.abs(b.imag) > 1e-3
    return np.array_equal((got.real > 0)[re], (b.real > 0)[re]) and np.array_equal((got.imag > 0)[im], (b.imag > 0)[im])


def _accept(tag, c, rx, ic_iter, ds, offs, rot, backoff=0, with_b=True):
    """the acceptance of one call: fused vs (A), and vs (B) relative to (A)'s own distance from it"""
    fused = _h(rx.demodulate_bursts(ds, offs, rot, backoff=backoff, preamble_offset=c["pre_off"]))
    a = _h(_two_step(rx, c, ds, offs, rot, backoff))
    assert fused.shape == a.shape == (offs.numel(), c["A"] * c["M"])
    e_a = rel_err(fused, a)
    print("%s: rel_err(fused, A) %.3e" % (tag, e_a))
    check_err("burst_rx_vs_chain_" + tag, e_a, TOL)
    if with_b:
        e = virtual_bursts(_h(ds), _h(offs), _h(rot), backoff, c["F"])
        b, margin = restatement(c, e, ic_iter)
        assert margin > MARGIN                                                    # (C)
        e_ab, e_fb = rel_err(a, b), rel_err(fused, b)
        print("%s: rel_err(A, B) %.3e rel_err(fused, B) %.3e margin %.3f" % (tag, e_ab, e_fb, margin))
        check_err("burst_rx_chain_vs_f64_" + tag, e_ab, TOL)
        check_err("burst_rx_vs_f64_" + tag, e_fb, 2 * e_ab)
        assert _same_signs(fused, b)
    return fused


# (generic_rader: what a handle of the reference's QA shape reports; its estimated calls, this one among them, run on the generic kernels)
KERNEL = {"rowlane_7": ("rowlane",), "rowlane_1": ("rowlane",), "rowlane_mfma": ("rowlane",), "rowlane_jit": ("rowlane_jit",),
          "generic_127": ("generic_lds", "generic_rader"), "generic_5_32": ("generic_lds",)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bursts_from_the_capture(name):
    """cases 1-4: every kernel route, both receivers"""
    M, K, L, A, nb, seed = CASES[name]
    c = make_case(M, K, L, A, nb, seed)
    ds, offs, rot = _t(c["stream"]), _t(c["starts"]), _t(c["sc_rot"])
    generic = name == "generic_5_32"
    for rx, it in zip(_receivers(c, generic), (None, 2)):
        assert rx.kernel_name() in KERNEL[name]
        fused = _accept("%s_%s" % (name, "ic" if it else "dem"), c, rx, it, ds, offs, rot)
        if it:
            assert np.array_equal(fused.real > 0, c["sym"].real > 0) and np.array_equal(fused.imag > 0, c["sym"].imag > 0)
    if generic:                                        # the row-lane kernels of the same shape, same call
        for rg, rr in zip(_receivers(c, True), _receivers(c)):
            assert rr.kernel_name() == "rowlane"
            e = rel_err(_h(rg.demodulate_bursts(ds, offs, rot)), _h(rr.demodulate_bursts(ds, offs, rot)))
            check_err("burst_rx_generic_vs_rowlane", e, TOL)


@pytest.mark.parametrize("backoff,pre_off", [(0, 0), (17, 0), (0, 21), (17, 21)])
def test_edges_of_the_fetch(backoff, pre_off):
    """case 5: bursts cut by either end of the capture (compared with (A) only, bit patterns of non-finite values included), two bursts at
    one offset, offsets in descending order, with and without backoff, preamble at the burst start and behind junk"""
    c = make_case(9, 64, 2, 52, 7, 1, pre_off)
    s, F = c["stream"], c["F"]
    st = c["starts"]
    # descending; 3 twice; one burst starting before sample 0, one running past the end (the capture is cut there)
    cut_lo, cut_hi = int(st[0]) + 40, int(st[6]) + F - 55
    s = s[cut_lo:cut_hi]
    order = [6, 5, 3, 3, 2, 1, 0]
    offs = st[order] - cut_lo + backoff
    ds, doffs, rot = _t(s), _t(offs), _t(c["sc_rot"][order])
    for rx, it in zip(_receivers(c), (None, 2)):
        tag = "edges_%d_%d_%s" % (backoff, pre_off, "ic" if it else "dem")
        fused = _h(rx.demodulate_bursts(ds, doffs, rot, backoff=backoff, preamble_offset=pre_off))
        a = _h(_two_step(rx, c, ds, doffs, rot, backoff))
        assert np.array_equal(_bits(fused[2]), _bits(fused[3]))                       # same offset: bit-equal rows
        for row in (0, 6):                                                            # cut by the capture's ends
            fin = np.isfinite(fused[row]) & np.isfinite(a[row])
            assert np.array_equal(_bits(fused[row])[~np.repeat(fin, 2)], _bits(a[row])[~np.repeat(fin, 2)])
            if fin.any():
                check_err("burst_rx_vs_chain_%s_cut%d" % (tag, row), rel_err(fused[row][fin], a[row][fin]), TOL)
        inner = slice(1, 6)
        _accept(tag, c, rx, it, ds, doffs[inner].contiguous(), rot[inner].contiguous(), backoff)
        assert np.array_equal(_bits(_h(rx.demodulate_bursts(ds, doffs[inner].contiguous(), rot[inner].contiguous(), backoff=backoff, preamble_offset=pre_off))),
                              _bits(fused[inner]))                                    # a row does not depend on its neighbours


def test_rotation_switches():
    """case 6: sc_rot None, cfo_correction False and r_b = 0 each equal the extractor with correction off, bit for bit; with a CFO of 0.25
    the symbols are recovered with the correction and not without it"""
    import torch
    c = make_case(9, 64, 2, 52, 5, 2, 0, 0.25)
    cfo = np.full(5, 0.25)
    # the same frames with a CFO of exactly +-0.25 on every burst: rotate the capture burst by burst
    s = c["stream"].astype(np.complex128)
    for b, st in enumerate(c["starts"]):
        n = np.arange(c["F"])
        s[st:st + c["F"]] *= np.exp(2j * np.pi * (cfo[b] - c["cfo"][b]) / c["K"] * n)
    ds, offs = _t(s.astype(np.complex64)), _t(c["starts"])
    rot = _t(np.exp(2j * np.pi * cfo / c["K"]).astype(np.complex64))
    for rx, it in zip(_receivers(c), (None, 2)):
        off = _h(_two_step(rx, c, ds, offs, rot, 0, correction=False))
        for kw in (dict(sc_rot=None), dict(sc_rot=rot, cfo_correction=False), dict(sc_rot=torch.zeros_like(rot))):
            got = _h(rx.demodulate_bursts(ds, offs, **kw))
            assert np.array_equal(_bits(got), _bits(off)), kw
        on = _h(rx.demodulate_bursts(ds, offs, rot))
        b_on, _ = restatement(c, virtual_bursts(_h(ds), _h(offs), _h(rot), 0, c["F"]), it)
        assert _same_signs(on, b_on)                             # recovered with the correction: what (B) recovers, both receivers
        bad = lambda o: float(np.mean(((o.real > 0) != (c["sym"].real > 0)) | ((o.imag > 0) != (c["sym"].imag > 0))))
        print("symbols with a sign error: %.4f with the correction, %.4f without" % (bad(on), bad(off)))
        assert bad(on) == 0                                      # ... and the transmitted symbols, with either receiver
        assert bad(off) > bad(on) + 0.1


def test_count():
    """case 7: rows from clamp(count, 0, n) on are zeros, the rows below bit-equal to the call without count"""
    import torch
    c = make_case(9, 64, 2, 52, 7, 0)
    ds, offs, rot = _t(c["stream"]), _t(c["starts"]), _t(c["sc_rot"])
    n = 7
    for rx in _receivers(c):
        full = _h(rx.demodulate_bursts(ds, offs, rot, count=None))
        assert np.all(np.abs(full).max(axis=1) > 0.1)
        for cnt in (0, 3, n, n + 5, -2):
            live = min(max(cnt, 0), n)
            out = torch.full((n, full.shape[1]), 7 + 7j, dtype=torch.complex64, device="cuda:0")
            got = _h(rx.demodulate_bursts(ds, offs, rot, count=_t([cnt], torch.int64), out=out))
            assert np.array_equal(_bits(got[:live]), _bits(full[:live])), cnt
            assert np.all(_bits(got[live:]) == 0), cnt


def test_long_capture():
    """case 8: a zero capture of 2^29 samples with three bursts: just below sample 2^28, just above it (byte offsets on either side of
    2^31) and ending at the last sample (past 2^32); bit-equal to the same bursts in a short capture"""
    import torch
    c = make_case(9, 64, 2, 52, 7, 0)
    F, n_long = c["F"], 1 << 29
    pos_long = np.array([(1 << 28) - 100, (1 << 28) - 100 + F + 3, n_long - F], np.int64)       # (the first straddles sample 2^28, the second lies behind it)
    pos_short = np.array([50, 50 + F + 9, 2 * (50 + F + 9)], np.int64)
    segs = [c["stream"][st:st + F] for st in c["starts"][:3]]
    short = np.zeros(int(pos_short[-1]) + F, np.complex64)
    for p, seg in zip(pos_short, segs):
        short[p:p + F] = seg
    big = torch.zeros(n_long, dtype=torch.complex64, device="cuda:0")
    for p, seg in zip(pos_long, segs):
        big[int(p):int(p) + F] = _t(seg)
    rot = _t(c["sc_rot"][:3])
    for rx in _receivers(c):
        want = _h(rx.demodulate_bursts(_t(short), _t(pos_short), rot))
        got = _h(rx.demodulate_bursts(big, _t(pos_long), rot))
        assert np.all(np.abs(want).max(axis=1) > 0.1)
        assert np.array_equal(_bits(got), _bits(want))
    del big


def _detect_stream(seed, slots, M=9, K=64, L=2, A=52):
    """the stream of tests/test_burst_detect_gpu.py::test_detect_extract_receive_on_device (seed M K + L: that very stream; another seed:
    other symbols, offsets, CFOs and noise behind the same preamble)"""
    import gfdm_amd
    rng = np.random.default_rng(seed)
    N, pcp, cp = M * K, K // 2, K // 2
    smap = np.concatenate((np.arange(1, A // 2 + 1), np.arange(K - A // 2, K)))
    spec = np.zeros(K, complex)
    spec[smap] = np.exp(1j * np.pi / 2 * (rng if seed == M * K + L else np.random.default_rng(M * K + L)).integers(0, 4, A)) * np.sqrt(K / A)
    core = np.tile(np.fft.ifft(spec) * np.sqrt(A), 2) / np.sqrt(K)
    full = np.concatenate((core[-pcp:], core))
    taps = get_frequency_domain_filter("rrc", 0.2, M, K, L)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, smap, True, L, taps, np.zeros(0, complex), [0], [full])
    F = tx.output_vector_size()
    bits = rng.integers(0, 2, (slots, A * M, 2))
    sym = ((1 - 2 * bits[..., 0]) + 1j * (1 - 2 * bits[..., 1])) / np.sqrt(2)
    frames = tx.transmit(_t(sym.astype(np.complex64)))[0].cpu().numpy()
    S = 2 * F
    offs = rng.integers(K, S - F - K, slots)
    cfo = rng.uniform(-0.25, 0.25, slots)
    sigma = np.sqrt(np.mean(np.abs(frames) ** 2) / 10 ** 2.5 / 2)
    s = sigma * (rng.standard_normal(slots * S) + 1j * rng.standard_normal(slots * S))
    for b in range(slots):
        rot = (0.8 + 0.45 * rng.random()) * np.exp(1j * (2 * np.pi * rng.random() + 2 * np.pi * cfo[b] / K * np.arange(F)))
        s[b * S + offs[b]:b * S + offs[b] + F] += frames[b] * rot
    return dict(stream=s.astype(np.complex64), sym=sym, core=core, taps=taps, smap=smap, F=F, pcp=pcp, cp=cp, N=N, slot_len=S)


def test_detect_then_demodulate_and_graph():
    """case 9: detect(max_bursts = slots + 8) -> demodulate_bursts(count = detect's): every sign recovered, the spare rows zero; the same
    two calls captured in one graph and replayed on another capture with another number of bursts equal the eager calls on it"""
    import torch
    import gfdm_amd
    M, K, L, A, slots = 9, 64, 2, 52, 64
    a = _detect_stream(M * K + L, slots)
    b = _detect_stream(4711, slots - 23)
    F, pcp, cp, N = a["F"], a["pcp"], a["cp"], a["N"]
    sb = np.zeros_like(a["stream"])
    sb[:b["stream"].size] = b["stream"]                                  # the shorter capture in the same buffer, silence behind it
    lead, nmax = pcp + K // 2, slots + 8
    sync = gfdm_amd.BurstSync(K, pcp, a["core"], lead + 3 * K + pcp)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, a["core"])
    adv = gfdm_amd.AdvancedReceiver(M, K, L, a["taps"], a["smap"], 2, R.qpsk_points())
    adv.configure_frames(2 * K + cp + N, 2 * K + cp, a["smap"], True)
    adv.set_channel_estimator(est)
    ds = _t(a["stream"])

    def chain(out=None):
        r = sync.detect(ds, 0.5, F // 2, lead, max_bursts=nmax)
        return r, adv.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"], out=out)

    def signs_ok(o, sym):
        return np.array_equal(o.real > 0, sym.real > 0) and np.array_equal(o.imag > 0, sym.imag > 0)

    r, out = chain()
    eager_a = _h(out)
    assert int(r["count"][0]) == slots
    assert signs_ok(eager_a[:slots], a["sym"]) and np.all(_bits(eager_a[slots:]) == 0)
    ds.copy_(_t(sb))
    r, out = chain()
    eager_b = _h(out)
    assert int(r["count"][0]) == slots - 23
    assert signs_ok(eager_b[:slots - 23], b["sym"]) and np.all(_bits(eager_b[slots - 23:]) == 0)

    ds.copy_(_t(a["stream"]))
    gout = torch.empty(nmax, A * M, dtype=torch.complex64, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        chain(gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rg, _ = chain(gout)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_h(gout)), _bits(eager_a))
    ds.copy_(_t(sb))                                    # another capture, another number of bursts, same buffers
    graph.replay()
    torch.cuda.synchronize()
    assert int(rg["count"][0]) == slots - 23
    assert np.array_equal(_bits(_h(gout)), _bits(eager_b))


def test_host_flavour_equals_device_flavour():
    """case 10: numpy arrays in -> the host entry point; bit-equal to the device one"""
    c = make_case(9, 64, 2, 52, 7, 0, 21)
    for rx in _receivers(c):
        kw = dict(backoff=17, preamble_offset=21)
        offs = c["starts"] + 17
        dev = _h(rx.demodulate_bursts(_t(c["stream"]), _t(offs), _t(c["sc_rot"]), _t([5], None), **kw))
        host = rx.demodulate_bursts(c["stream"], offs, c["sc_rot"], np.array([5], np.int64), **kw)
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(dev))
        assert np.all(_bits(host[5:]) == 0) and np.all(np.abs(host[:5]).max(axis=1) > 0.1)
        assert np.array_equal(_bits(rx.demodulate_bursts(c["stream"], offs, None, None, **kw)),
                              _bits(_h(rx.demodulate_bursts(_t(c["stream"]), _t(offs), None, None, **kw))))


def test_argument_errors():
    """case 11: every EINVAL of the contract with its message; no bursts -> an empty result"""
    import gfdm_amd
    c = make_case(9, 64, 2, 52, 7, 0)
    M, K, L, A, F = c["M"], c["K"], c["L"], c["A"], c["F"]
    s, offs = c["stream"], c["starts"]
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    for make in (lambda: gfdm_amd.Demodulator(M, K, L, c["taps"]), lambda: gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())):
        rx = make()
        with pytest.raises(ValueError, match="set_channel_estimator"):
            rx.demodulate_bursts(s, offs)
        rx.set_channel_estimator(est)
        with pytest.raises(ValueError, match="configure_frames"):
            rx.demodulate_bursts(s, offs)
        with pytest.raises(ValueError, match="configure_frames"):
            rx.demodulate_bursts(_t(s), _t(offs))
        rx = make()
        rx.configure_frames(F, 2 * K + c["cp"], c["smap"], True)
        rx._estimator = est                                     # past the Python-side check: the library refuses the missing estimator itself
        with pytest.raises(ValueError, match="set_channel_estimator"):
            rx.demodulate_bursts(s, offs)
        rx.set_channel_estimator(est)
        for kw, match in ((dict(preamble_offset=-1), "preamble_offset"), (dict(preamble_offset=F - 2 * K + 1), "preamble_offset"),
                          (dict(backoff=-1), "backoff"), (dict(noutput_size=A * M + 1), "MUST not exceed")):
            with pytest.raises(ValueError, match=match):
                rx.demodulate_bursts(s, offs, **kw)
            with pytest.raises(ValueError, match=match):
                rx.demodulate_bursts(_t(s), _t(offs), **kw)
        L_ = gfdm_amd.lib()
        fn = getattr(L_, rx._bursts_prefix + "_host")
        out = np.zeros((7, A * M), np.complex64)
        for stream_len, n, match in ((-1, 7, "stream_len"), (s.size, -1, "n_bursts")):
            assert fn(rx._h, out.ctypes.data, s.ctypes.data, stream_len, offs.ctypes.data, None, None, 0, 0, 1, -1, n) == gfdm_amd.capi.EINVAL
            assert match in L_.gfdm_hip_last_error().decode()
        assert rx.demodulate_bursts(s, offs[:0]).shape == (0, A * M)
        assert tuple(rx.demodulate_bursts(_t(s), _t(offs[:0])).shape) == (0, A * M)
        assert rx.demodulate_bursts(s, offs, noutput_size=100).shape == (7, 100)
