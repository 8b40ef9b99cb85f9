"""GPU tests of the spectrum meter (contract in include/gfdm_hip.h, gfdm_hip_spectrum_meter) against the numpy restatement of
tests/spectrum_meter_ref.py.  Two yardsticks for psd_sum, neither the code under test:
  the derived budget of the header, per bin (it catches wrong indices and twiddles), and
  the project's rule for its transforms: ||got - ref||_2 over the bins against the same error of numpy's own complex64 pipeline on the
  same input, floored at 2^-24 ||ref||_2, held to 3 (it catches lost bits).
The integer totals (segments, bad_segments, samples, bad_samples, peak_bits, hist) are exact; power_sum is held to (tiles + 32) 2^-53.
Every case prints its figures ("spectrum accuracy: ...") before it asserts; profiles/r22/spectrum_accuracy.json is made of those lines."""
import numpy as np
import pytest

import burst_shaper_ref as B
import spectrum_meter_ref as R
from conftest import have_gpu
from spectrum_gpu_common import INT, Guarded
from spectrum_gpu_common import check_psd as _check_psd
from spectrum_gpu_common import same_totals as _same_totals
from spectrum_gpu_common import to_device as _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _psd_ref(x, sm, origins=None):
    x = R.widen(x) if np.asarray(x).dtype == np.int16 else np.asarray(x, np.complex64)
    nfft, hop = sm.nfft(), sm.hop()
    return R.psd(x, sm.window(), R.stream_origins(nfft, hop, x.size) if origins is None else origins)


@pytest.mark.parametrize("nfft", R.NFFTS)
def test_every_size_three_segments_hann(nfft):
    import gfdm_amd
    sm = gfdm_amd.SpectrumMeter(nfft)
    assert (sm.nfft(), sm.hop()) == (nfft, nfft // 2) and np.array_equal(sm.window(), R.hann(nfft))
    x = R.gaussian_with_tone(2 * nfft, nfft, nfft)
    assert sm.plan(x.size) == (3, 3 * (nfft // 2))
    assert sm.update(_t(x)) == 3 * (nfft // 2)
    t = sm.read()
    _check_psd(t, _psd_ref(x, sm), "nfft %d, 3 segments, hann" % nfft)
    assert t["samples"] == t["bad_samples"] == t["peak_bits"] == 0 and t["power_sum"] == 0.0 and not t["hist"].any()
    # the host flavour is the device flavour behind an upload
    host = gfdm_amd.SpectrumMeter(nfft)
    host.update(x)
    assert _same_totals(host.read(), t)
    # psd(): the bins of a stationary input add up to its mean power (Parseval: exactly the windowed segments' mean power)
    f = x[R.stream_origins(nfft, nfft // 2, x.size)[:, None] + np.arange(nfft)].astype(np.complex128) * R.hann(nfft).astype(np.float64)
    assert sm.psd().sum() == pytest.approx((np.abs(f) ** 2).sum() / (3 * float((R.hann(nfft).astype(np.float64) ** 2).sum())), rel=1e-6)
    assert np.array_equal(sm.psd(shift=True), np.fft.fftshift(sm.psd()))
    assert sm.band_power(-2, 3) == pytest.approx(sm.psd()[[-2, -1, 0, 1, 2]].sum(), rel=1e-12)


@pytest.mark.parametrize("nfft", (16, 64))
def test_hops_and_lengths(nfft):
    import gfdm_amd
    for hop in (1, 3, nfft // 2, nfft - 1, nfft):
        sm = gfdm_amd.SpectrumMeter(nfft, hop=hop)
        x = R.gaussian_with_tone(nfft + 6 * hop + hop - 1, 100 * nfft + hop, nfft)
        sm.update(_t(x))
        t = sm.read()
        assert t["segments"] == 7
        _check_psd(t, _psd_ref(x, sm), "nfft %d hop %d, 7 segments" % (nfft, hop))
        # n = nfft - 1: no segment, no launch, the totals untouched; n = nfft: one; n = nfft + hop - 1: still one
        assert sm.update(_t(x[:nfft - 1])) == 0 and _same_totals(sm.read(), t)
        for n in (nfft, nfft + hop - 1):
            one = gfdm_amd.SpectrumMeter(nfft, hop=hop)
            assert one.update(_t(x[:n])) == hop
            _check_psd(one.read(), _psd_ref(x[:nfft], one), "nfft %d hop %d n %d" % (nfft, hop, n))
        assert one.update(_t(x[:0])) == 0


@pytest.mark.parametrize("nfft", (16, 256, 4096))
def test_alignment_sc16_repeats_and_canaries(nfft):
    import gfdm_amd
    hop = nfft // 2
    x = R.gaussian_with_tone(3 * nfft + 5, 7 * nfft, nfft, scale=300.0)
    iq = R.sc16_capture(3 * nfft + 5, 7 * nfft, nfft)
    first = None
    for shift in (0, 1):                                                           # both 8-byte alignments of complex64
        g = Guarded(x, shift)
        sm = gfdm_amd.SpectrumMeter(nfft)
        sm.update(g.view)
        sm.power(g.view)
        t = sm.read()
        assert g.unchanged()
        if first is None:
            first = t
            _check_psd(t, _psd_ref(x, sm), "nfft %d, complex64 at scale 300" % nfft)
        assert _same_totals(t, first), "the totals depend on the alignment of the input"
    widened = gfdm_amd.SpectrumMeter(nfft)
    widened.update(_t(R.widen(iq)))
    widened.power(_t(R.widen(iq)))
    want = widened.read()
    _check_psd(want, _psd_ref(iq, widened), "nfft %d, widened sc16" % nfft)
    for shift in (0, 1, 2, 3):                                                     # all four 4-byte alignments of sc16
        g = Guarded(iq, shift)
        sm = gfdm_amd.SpectrumMeter(nfft)
        assert sm.update(g.view) == sm.plan(iq.shape[0])[1]
        sm.power(g.view)
        assert g.unchanged()
        assert _same_totals(sm.read(), want), "sc16 is not bit-equal to the widened call (shift %d)" % shift
    flat = gfdm_amd.SpectrumMeter(nfft)
    flat.update(_t(iq.reshape(-1)))                                                # (2n,) is (n, 2)
    flat.power(iq.reshape(-1))                                                     # ... and on the host path
    assert _same_totals(flat.read(), want)
    # two calls on the same input: bit-equal totals, and twice one call's integers
    a, b = gfdm_amd.SpectrumMeter(nfft), gfdm_amd.SpectrumMeter(nfft)
    for sm in (a, b):
        for _ in range(2):
            sm.update(_t(x))
            sm.power(_t(x))
    ta = a.read()
    assert _same_totals(ta, b.read()) and ta["segments"] == 2 * first["segments"] and ta["samples"] == 2 * first["samples"]
    assert np.array_equal(ta["hist"], 2 * first["hist"]) and ta["peak_bits"] == first["peak_bits"]
    assert np.allclose(ta["psd_sum"], 2 * first["psd_sum"], rtol=2.0 ** -40, atol=0)
    # reset
    a.reset()
    z = a.read()
    assert all(z[k] == 0 for k in INT) and z["power_sum"] == 0.0 and not z["psd_sum"].any() and not z["hist"].any()
    a.update(_t(x))
    a.power(_t(x))
    assert _same_totals(a.read(), first)
    assert hop == a.hop()


@pytest.mark.parametrize("nfft,hop", ((16, 3), (64, 32), (1024, 1024), (4096, 1000)))
def test_cut_stream(nfft, hop):
    import gfdm_amd
    x = R.gaussian_with_tone(nfft + 40 * hop + 2, nfft + hop, nfft)
    whole, cut = gfdm_amd.SpectrumMeter(nfft, hop=hop), gfdm_amd.SpectrumMeter(nfft, hop=hop)
    xd = _t(x)
    assert whole.update(xd) == 41 * hop
    start = 0
    for end in (x.size // 3, 2 * x.size // 3, x.size):
        start += cut.update(xd[start:end])
    assert start == 41 * hop
    a, b = whole.read(), cut.read()
    assert all(a[k] == b[k] for k in INT) and a["segments"] == 41
    assert np.all(np.abs(a["psd_sum"] - b["psd_sum"]) <= 2.0 ** -40 * a["psd_sum"])
    _check_psd(b, _psd_ref(x, cut), "nfft %d hop %d, a stream cut into three calls" % (nfft, hop))


@pytest.mark.parametrize("nfft", (16, 128, 2048))
def test_a_non_finite_sample_stays_in_its_segment(nfft):
    import gfdm_amd
    for bad in (np.nan, np.inf, complex(0, -np.inf)):
        x = R.gaussian_with_tone(5 * nfft, 3 * nfft, nfft)
        x[2 * nfft + nfft // 3] = bad
        sm = gfdm_amd.SpectrumMeter(nfft, hop=nfft)
        sm.update(_t(x))
        t = sm.read()
        assert (t["segments"], t["bad_segments"]) == (4, 1)
        _check_psd(t, _psd_ref(x, sm), "nfft %d, one segment of five with %r" % (nfft, bad))
    # overlapping segments: the sample spoils every segment it lies in and no other
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.update(_t(x))
    t = sm.read()
    assert (t["segments"], t["bad_segments"]) == (7, 2)
    _check_psd(t, _psd_ref(x, sm), "nfft %d, overlapping segments, two of nine bad" % nfft)


def test_a_product_that_overflows_spoils_its_segment():
    """finite samples times a finite window value beyond fp32: the segment counts in bad_segments and psd_sum stays finite"""
    import gfdm_amd
    nfft = 64
    w = R.hann(nfft)
    w[5] = 3e38
    x = R.gaussian_with_tone(3 * nfft, 77, nfft)
    for data in (x, R.sc16_capture(3 * nfft, 77, nfft)):
        data[5] = data[2 * nfft + 5] = 1000                                        # 1000 * 3e38 overflows
        data[nfft + 5] = 0                                                         # the middle segment's product at w[5] is 0: it alone survives
        sm = gfdm_amd.SpectrumMeter(nfft, window=w, hop=nfft)
        sm.update(_t(data))
        t = sm.read()
        assert (t["segments"], t["bad_segments"]) == (1, 2) and np.isfinite(t["psd_sum"]).all()
        _check_psd(t, _psd_ref(data, sm), "nfft 64, a window value of 3e38", yardstick=False)


@pytest.mark.parametrize("nfft", (1024, 4096))
def test_a_dominant_tone_stays_inside_its_bin_s_bound(nfft):
    """a tone that carries the whole norm (amplitude 4 in unit noise): the yardstick would be one draw of one bin's rounding error there
    (tests/spectrum_meter_ref.py, tone_amplitude), so that bin is held to a bound of its own, coherent_bin_bound, and the figure is printed"""
    import gfdm_amd
    x = R.gaussian_with_tone(3 * nfft + 5, 7 * nfft, nfft, scale=300.0, amp=4.0)
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.update(_t(x))
    t = sm.read()
    r = _psd_ref(x, sm)
    k = int(np.argmax(r["psd_sum"]))
    assert r["psd_sum"][k] > 0.5 * r["psd_sum"].sum()
    rel = abs(t["psd_sum"][k] - r["psd_sum"][k]) / r["psd_sum"][k]
    print("spectrum accuracy: dominant tone, nfft %d: bin %d off by %.2f x 2^-24 of itself, bound %.0f x 2^-24; yardstick ratio %.3f (not asserted)"
          % (nfft, k, rel * 2.0 ** 24, R.coherent_bin_bound(nfft) * 2.0 ** 24, R.yardstick_ratio(t["psd_sum"], r)))
    assert rel <= R.coherent_bin_bound(nfft)
    assert R.budget_share(t["psd_sum"], r) <= 1.0


@pytest.mark.parametrize("nfft,sc16", ((64, False), (256, True), (1024, False)))
def test_update_at(nfft, sc16):
    import gfdm_amd
    hop, spb, first = nfft // 2, 3, -5
    span = first + (spb - 1) * hop + nfft
    stream_len = 9 * span + 77
    x = R.sc16_capture(stream_len, 5 * nfft, nfft) if sc16 else R.gaussian_with_tone(stream_len, 5 * nfft, nfft)
    # permuted, a -1, a burst whose first segment starts in front of the stream (2 + first < 0), one whose last segment reaches past stream_len
    starts = np.array([4 * span, 17, -1, 7 * span + 3, 2, stream_len - span + 9, 2 * span + 1, 17], np.int64)
    xd, sd = _t(x), _t(starts)
    for count in (None, -2, 0, 3, len(starts), len(starts) + 5):
        sm = gfdm_amd.SpectrumMeter(nfft)
        sm.update_at(xd, sd, spb, first, count=count)
        o = R.burst_origins(starts, count, first, spb, hop, nfft, stream_len)
        t = sm.read()
        assert t["segments"] == len(o) and t["bad_segments"] == 0
        if count is None:
            assert len(o) == 3 * 5 + 2 + 2                                     # five whole bursts (17 twice), two segments each of the two at the edges
        _check_psd(t, _psd_ref(x, sm, o), "update_at nfft %d %s count %r" % (nfft, "sc16" if sc16 else "c64", count), yardstick=len(o) > 0)
        if count in (3, None):                                                 # count as detect writes it, and the host flavour
            dev = gfdm_amd.SpectrumMeter(nfft)
            dev.update_at(xd, sd, spb, first, count=None if count is None else _t(np.array([count], np.int64)))
            host = gfdm_amd.SpectrumMeter(nfft)
            host.update_at(x, starts, spb, first, count=count)
            assert _same_totals(dev.read(), t) and _same_totals(host.read(), t)
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.update_at(xd, sd[:0], spb, first)
    sm.update_at(xd, sd, 0, first)
    assert sm.read()["segments"] == 0
    with pytest.raises(ValueError):
        sm.update_at(xd, sd, -1, first)


def test_power_exact_over_eighty_octaves():
    import gfdm_amd
    n = 100003
    for name, x in (("complex64", R.wide_range_powers(n, 9)), ("sc16", R.wide_range_sc16(n, 9))):
        r = R.power(R.widen(x) if name == "sc16" else x)
        if name == "complex64":
            assert r["bad_samples"] == 3 and r["hist"][0] > 1000 and r["hist"][511] > 1000 and np.count_nonzero(r["hist"]) == 512
        for shift in (0, 1):
            g = Guarded(x, shift)
            sm = gfdm_amd.SpectrumMeter(64)
            sm.power(g.view)
            t = sm.read()
            assert g.unchanged()
            assert [t[k] for k in INT] == [0, 0, r["samples"], r["bad_samples"], r["peak_bits"]], name
            assert np.array_equal(t["hist"], r["hist"]), name
            err, bound = abs(t["power_sum"] - r["power_sum"]), R.power_bound(r["tiles"], r["power_sum"])
            print("spectrum accuracy: power_sum %s shift %d: |got - ref| = %.3g, bound %.3g" % (name, shift, err, bound))
            assert err <= bound, name
            assert not t["psd_sum"].any()
        host = gfdm_amd.SpectrumMeter(64)
        host.power(x)
        assert _same_totals(host.read(), t)
        assert sm.mean_power() == t["power_sum"] / t["samples"]
        peak = float(np.array([r["peak_bits"]], np.uint32).view(np.float32)[0])
        assert sm.peak_power() == peak and sm.papr_db() == pytest.approx(10 * np.log10(peak / (r["power_sum"] / r["samples"])), abs=1e-9)
        edges, tail = sm.ccdf()
        assert tail[0] == r["samples"] and np.array_equal(tail, np.cumsum(r["hist"][::-1])[::-1])
        assert np.allclose(edges * sm.mean_power(), R.hist_edges(), rtol=1e-14, atol=0)
    empty = gfdm_amd.SpectrumMeter(64)
    empty.power(_t(np.zeros(0, np.complex64)))
    assert empty.read()["samples"] == 0 and np.isnan(empty.papr_db()) and np.isnan(empty.mean_power())


def test_graph_replay():
    """reset + accumulate + power captured once and replayed: a linear graph, the totals of the eager calls"""
    import torch
    import gfdm_amd
    nfft = 256
    x = R.gaussian_with_tone(20 * nfft + 9, 41, nfft)
    xd = _t(x)
    eager = gfdm_amd.SpectrumMeter(nfft)
    eager.update(xd)
    eager.power(xd)
    want = eager.read()
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.update(xd)                                                                  # something for the captured reset to clear
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                  # the current stream inside is the capturing one
        sm.reset()
        sm.update(xd)
        sm.power(xd)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _same_totals(sm.read(), want)
    _check_psd(want, _psd_ref(x, sm), "graph replay, nfft 256")


def test_end_to_end_received_bursts():
    """frames at K = 64, M = 9 with 52 active subcarriers: transmit -> place with gaps -> ChannelModel.apply at 30 dB -> detect ->
    update_at(detect's starts, nfft 256).  Asserted: the PSD of the received bursts is the restatement's on the downloaded capture.
    Printed, not asserted: the out-of-band ratio and the PAPR (nobody has measured them before)."""
    import gfdm_amd
    c = B.loop_case()
    M_, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    assert (K, M_, A) == (64, 9, 52)
    nfft = 256
    tx = gfdm_amd.Transmitter(M_, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(_t(c["sym"]))                                             # one tensor per cyclic shift: one
    assert len(frames) == 1
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(frames, _t(c["starts"]), c["out_len"])[0]
    signal = float((frames[0].abs().double() ** 2).mean()) * B.LOOP_SCALE ** 2    # the mean power of a placed frame
    ch = gfdm_amd.ChannelModel((signal / 10.0 ** 3.0) ** 0.5, 0.0, 1.0, (1,), 5)  # noise power 30 dB below it
    rx = ch.apply(placed)
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(rx, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb
    first = 2 * K + cp                                                             # behind the preamble: the payload and its prefix
    spb = (N - nfft) // (nfft // 2) + 1
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.update_at(rx, r["frame_start"], spb, first, count=r["count"])
    sm.power(frames[0])
    t = sm.read()
    cap = rx.cpu().numpy()
    o = R.burst_origins(r["frame_start"].cpu().numpy(), int(r["count"][0]), first, spb, nfft // 2, nfft, cap.size)
    assert t["segments"] == nb * spb == len(o)
    _check_psd(t, R.psd(cap, sm.window(), o), "end to end, received payloads at 30 dB, nfft 256")
    P = sm.psd()
    assert P.sum() == pytest.approx(float(np.mean(np.abs(cap[o[:, None] + np.arange(nfft)]) ** 2)), rel=0.3)
    print("spectrum meter, K 64 M 9, 52 active subcarriers, rrc 0.1, payload of %d received bursts at 30 dB, hann 256: out-of-band ratio %.2f dB; "
          "PAPR of the transmitted frames %.2f dB" % (nb, gfdm_amd.oob_ratio_db(P, K, c["smap"]), sm.papr_db()))
