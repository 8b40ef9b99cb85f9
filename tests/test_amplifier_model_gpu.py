"""GPU tests of the amplifier model (contract in include/gfdm_hip.h, gfdm_hip_amplifier_model).  The yardstick is the float64 numpy
restatement of tests/amplifier_model_ref.py on the same complex64 inputs, never the code under test, and the bounds are the contract's:
    POLY          |y - y64| <= (4 K + Q + 8) 2^-23 S_i,        S_i = sum_q sum_k |c[q][k]| |u[i - q]|^(2 k + 1)
    closed forms  |y - y64| <= B 2^-23 |y64|,  B the larger of the derived floor (8 CLIP and RAPP, 16 SALEH) and twice what the ref file's
                  float32 numpy evaluation needs on the same inputs
counted from the roundings, not from what the kernel gives; every test prints the worst share that it saw (with GFDM_AMPLIFIER_ACCURACY=
<file> the shares of the accuracy test are also written there as JSON: profiles/r23/amplifier_accuracy.json).  sc16 output equals q of the
restatement except inside the guard band (within gain * budget of a step of q), where it may be one LSB off.  Every output lies between
guard words.  What the kernel promises about bits -- a sample does not depend on the alignment of either buffer or on where a stream is
cut into calls -- is tested bit for bit."""
import json
import os

import numpy as np
import pytest

import amplifier_model_ref as Am
import burst_shaper_ref as B
import channel_model_ref as C
import gfdm_ref as R
import spectrum_meter_ref as Sp
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


def _model(sp, drive=1.0):
    import gfdm_amd
    return gfdm_amd.AmplifierModel(sp["kind"], tuple(sp["p"]), sp["c"], drive=drive)


def _check_c64(got, y, budget, tag, quiet=False):
    assert got.dtype == np.complex64 and got.shape == y.shape
    share = Am.share_of_budget(got, y, budget)
    if not quiet:
        print("%s: worst error %.3f of the budget" % (tag, share))
    assert share <= 1.0, (tag, share)
    return share


def _check_sc16(got, y, budget, gain, tag):
    want, guard = Am.sc16(y, budget, gain)
    assert got.dtype == np.int16 and got.shape == want.shape
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert guard.sum() <= max(1, Am.GUARD_CAP * guard.size), tag
    assert np.array_equal(got[~guard], want[~guard]), tag
    assert d.max(initial=0) <= 1, tag
    return int(guard.sum()), int(np.count_nonzero(d[guard]))


N_ACC = 2 * Am.K_TILE + 5


# ---- 1. accuracy of every kind ----
def test_accuracy_of_every_kind():
    """n = 2 tile + 5 samples whose amplitudes spread over e^-6 .. e^3 times a unit Gaussian, through every closed form (CLIP; RAPP at p =
    0.5, 1, 2, 3, 10; the classic Saleh curves and one whose phase reaches pi) and POLY at (Q, K) = (1, 1), (1, 2), (3, 3), (4, 5), (16, 5)"""
    shares = {}
    for i, sp in enumerate(Am.closed_forms()):
        x = Am.wide_signal(i, N_ACC)
        y, floor = Am.apply(x, 0, sp)
        Bf = Am.closed_form_B(x, sp)
        got = _h(_model(sp).apply(_t(x)))
        need = Am.need_of(got, y)
        shares[Am.tag(sp)] = dict(B=Bf, needs_units_of_2_23_y=round(need, 3), share=round(need / Bf, 4))
        print("%s: the kernel needs %.2f * 2^-23 |y| of B = %.1f: share %.3f" % (Am.tag(sp), need, Bf, need / Bf))
        assert _check_c64(got, y, floor * (Bf / Am.floor_of(sp["kind"])), Am.tag(sp), quiet=True) <= 1.0
    for i, sp in enumerate(Am.polys()):
        Q = Am.delays(sp)
        x = Am.wide_signal(100 + i, N_ACC + Q - 1)
        y, budget = Am.apply(x, Q - 1, sp)
        got = _h(_model(sp).apply(_t(x), Q - 1))
        shares[Am.tag(sp)] = dict(share=round(_check_c64(got, y, budget, Am.tag(sp)), 4))
    path = os.environ.get("GFDM_AMPLIFIER_ACCURACY")
    if path:
        with open(path, "w") as f:
            json.dump(shares, f, indent=1)


# ---- 2. RAPP at p = 16 with large inputs ----
def test_rapp_at_p_16_with_large_inputs():
    """amplitudes from A / 4 up to 2^60 A: the float32 formula written naively returns 0 there; the kernel stays on the curve"""
    A = 1.5
    sp = Am.spec("rapp", 2.0, A, 16.0)
    rng = np.random.default_rng(2302)
    n = Am.K_TILE + 77
    amp = A * np.exp2(rng.uniform(-2, 60, n))
    amp[:3] = A * 2.0 ** 60, A * 2.0 ** 59.5, A * 0.75
    x = (amp * np.exp(2j * np.pi * rng.random(n))).astype(np.complex64)
    got = _h(_model(sp).apply(_t(x)))
    mod = np.abs(got.astype(np.complex128))
    assert np.all(np.isfinite(mod)) and np.all(mod > 0) and np.all(mod <= A * (1 + 2.0 ** -21))
    y, floor = Am.apply(x, 0, sp)
    _check_c64(got, y, floor, "rapp p 16, amplitudes up to 2^60 A")
    assert np.count_nonzero(Am.rapp32_naive(x, sp) == 0) > n // 2


# ---- 3. CLIP exactness ----
@pytest.mark.parametrize("drive", [1.0, 0.37])
def test_clip_exactness(drive):
    A = 0.8
    sp = Am.spec("clip", A)
    x = Am.wide_signal(31, Am.K_TILE + 9)
    x[5] = x[Am.K_TILE] = 0
    x[6] = complex(0.0, -0.0)
    d = np.float32(drive)
    u = np.empty_like(x)
    u.real, u.imag = d * x.real, d * x.imag                                            # the fp32 product of each component (signs of zeros kept)
    assert (d * x.real).dtype == np.float32
    r = np.abs(u.astype(np.complex128)) ** 2
    A32 = float(np.float32(A))
    below, above = r <= A32 * A32 * (1 - 2.0 ** -20), r >= A32 * A32 * (1 + 2.0 ** -20)           # (a sample within rounding of the knee may take either branch)
    assert below.sum() > 100 and above.sum() > 100
    got = _h(_model(sp, drive).apply(_t(x)))
    assert np.array_equal(_bits(got[below]), _bits(u[below]))
    mod = np.abs(got.astype(np.complex128))
    assert np.all(mod[~below] <= A32 * (1 + 2.0 ** -21)) and np.all(mod[above] >= A32 * (1 - 2.0 ** -21))     # either branch of the band keeps the bound
    for i in (5, 6, Am.K_TILE):
        assert got[i] == 0 and np.array_equal(_bits(got[i:i + 1]), _bits(u[i:i + 1]))


# ---- 4. geometry ----
@pytest.mark.parametrize("ki", range(len(Am.geometry_kinds())), ids=[Am.tag(sp) for sp in Am.geometry_kinds()])
def test_geometry(ki):
    """n in 1, 2, 3, tile - 1, tile, tile + 1; history 0, Q - 1 and Q + 4; `in` at both alignments, `out` at every alignment of one sample,
    complex64 and sc16; canaries on both sides of every buffer; every alignment gives the bits of the first, and so do three pieces"""
    sp = Am.geometry_kinds()[ki]
    am = _model(sp)
    gain = Am.sc16_gain(sp)
    worst, in_guard, off = 0.0, 0, 0
    for c in Am.geometry_cases(ki):
        n, hist = c["n"], c["history"]
        xs = Am.geometry_signal(c["seed"], hist + n)
        y, budget = Am.apply(xs, hist, sp)
        first = {}
        for fmt, i_shift, o_shift in c["aligns"]:
            sc16 = fmt == "sc16"
            tag = "%s n %d history %d %s in+%d out+%d" % (Am.tag(sp), n, hist, fmt, i_shift, o_shift)
            x = Window(hist + n, i_shift, content=xs)
            w = Window(n, o_shift, sc16)
            res = am.apply(x.view, hist, out=w.view, gain=gain if sc16 else 1.0)
            assert res is w.view
            got = w.result()
            if sc16:
                g, o = _check_sc16(got, y, budget, gain, tag)
                in_guard, off = in_guard + g, off + o
            else:
                worst = max(worst, _check_c64(got, y, budget, tag, quiet=True))
            assert np.array_equal(_bits(x.result()), _bits(xs)), tag                   # the input is left alone
            if fmt not in first:
                first[fmt] = got.copy()
                # the same stream in three pieces (those of n < 3 that are empty are left out)
                p = Window(n, 1 - o_shift, sc16)
                for a, b, h in Am.pieces_with_history(sp, n, hist):
                    if b > a:
                        am.apply(x.view[hist + a - h:hist + b], h, out=p.view[a * p.per:b * p.per], gain=gain if sc16 else 1.0)
                assert np.array_equal(_bits(p.result()), _bits(got)), tag + ": three pieces"
            else:
                assert np.array_equal(_bits(got), _bits(first[fmt])), tag + ": another alignment, other bits"
    print("%s: worst share of the budget %.3f; sc16: %d components inside the guard band, %d of them one LSB off" % (Am.tag(sp), worst, in_guard, off))


def test_host_flavour_equals_device_flavour():
    for sp in Am.geometry_kinds():
        am = _model(sp, 0.9)
        Q = Am.delays(sp)
        xs = Am.geometry_signal(2390, Q - 1 + 777)
        dev = _h(am.apply(_t(xs), Q - 1))
        host = am.apply(xs, Q - 1)
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(dev))
        dev16 = _h(am.apply(_t(xs), Q - 1, sc16=True, gain=Am.sc16_gain(sp)))
        host16 = am.apply(xs, Q - 1, sc16=True, gain=Am.sc16_gain(sp))
        assert host16.dtype == np.int16 and host16.shape == (777, 2) and np.array_equal(host16, dev16)
        assert am.apply(np.zeros(0, np.complex64)).size == 0 and am.apply(_t(np.zeros(0, np.complex64))).numel() == 0
    with pytest.raises(ValueError, match="overlap"):
        x = _t(xs)
        am.apply(x[8:], 0, out=x[:x.numel() - 8])


# ---- 5. non-finite samples ----
@pytest.mark.parametrize("ki", range(len(Am.geometry_kinds())), ids=[Am.tag(sp) for sp in Am.geometry_kinds()])
def test_non_finite_samples_stay_where_they_are(ki):
    """one NaN sample (in the last samples of the first tile: POLY's outputs that read it lie in two tiles) and one Inf sample spoil their
    own 1 (POLY: Q) outputs; every other output keeps its bits"""
    sp = Am.geometry_kinds()[ki]
    am = _model(sp)
    Q = Am.delays(sp)
    n = Am.K_TILE + 300
    xs = Am.geometry_signal(2395 + ki, n)
    bad = xs.copy()
    at_nan, at_inf = Am.K_TILE - 2, 100
    bad[at_nan] = complex(np.nan, 0.25)
    bad[at_inf] = complex(0.25, -np.inf)
    for o_shift in (0, 1):
        clean = Window(n, o_shift)
        dirty = Window(n, o_shift)
        am.apply(_t(xs), out=clean.view)
        am.apply(_t(bad), out=dirty.view)
        a, b = clean.result(), dirty.result()
        spoiled = np.zeros(n, bool)
        spoiled[at_nan:at_nan + Q] = spoiled[at_inf:at_inf + Q] = True
        assert np.array_equal(_bits(a).reshape(n, 2)[~spoiled], _bits(b).reshape(n, 2)[~spoiled])
        assert not np.isfinite(b[spoiled]).any() and np.isfinite(a).all()


# ---- 6. two tones, a known answer ----
def test_two_tones_through_a_third_order_polynomial():
    """tones of amplitude a on the bins k1, k2 of nfft = 1024 through POLY(Q = 1, K = 2), c = [1, c3]: a rect-window SpectrumMeter shows the
    third-order products 2 k1 - k2, 2 k2 - k1 at |c3|^2 a^6 and the fundamentals at |1 + 3 c3 a^2|^2 a^2, within the meter's own
    coherent-bin bound plus what the budget of POLY(1, 2) and the rounding of the tones to complex64 can move a bin by"""
    import gfdm_amd
    am = gfdm_amd.AmplifierModel.poly([1, Am.TONE_C3])
    y = am.apply(_t(Am.two_tones()))
    sm = gfdm_amd.SpectrumMeter(Am.TONE_NFFT, "rect", hop=Am.TONE_NFFT)
    sm.update(y)
    assert sm.read()["segments"] == Am.TONE_SEGMENTS
    P = sm.psd()
    slack = Am.two_tone_slack()
    for k, want in sorted(Am.two_tone_answer().items()):
        bound = 2 * np.sqrt(want) * slack + slack ** 2 + Sp.coherent_bin_bound(Am.TONE_NFFT) * want
        print("bin %d: power %.9e, expected %.9e, difference %.3f of the bound" % (k, P[k], want, abs(P[k] - want) / bound))
        assert abs(P[k] - want) <= bound


# ---- 7. the linear case ----
@pytest.mark.parametrize("T", [1, 3, 16])
def test_linear_case_against_the_channel_model(T):
    """POLY(Q = T, K = 1) is an FIR: against ChannelModel(taps = c[:, 0], f = 0, noise = 0) on the same stream, each within its own budget
    of the shared restatement"""
    import gfdm_amd
    taps = C.taps_for(T)
    n, hist = Am.K_TILE + 321, T - 1
    xs = C.signal(2400 + T, hist + n)
    y, bc = C.apply(xs, hist, taps, 0.0, 0.0, 0, 0)
    ya, ba = Am.apply(xs, hist, Am.spec("poly", c=taps[:, None]))
    assert np.max(np.abs(y - ya)) <= 1e-14 * np.max(np.abs(y))
    got_a = _h(gfdm_amd.AmplifierModel.poly(taps[:, None]).apply(_t(xs), hist))
    got_c = _h(gfdm_amd.ChannelModel(0.0, 0.0, 1.0, taps).apply(_t(xs), hist))
    _check_c64(got_a, y, ba, "POLY(%d, 1)" % T)
    _check_c64(got_c, y, bc, "ChannelModel, %d taps" % T)


# ---- 8. set_drive and graph replay ----
def test_set_drive_is_read_at_enqueue_and_a_graph_replays():
    import torch
    sp = Am.spec("saleh", *Am.SALEH_CLASSIC)
    am = _model(sp, 0.5)
    n = 4097
    xs = Am.geometry_signal(2410, n)
    for drive in (0.5, 2.0, 0.0, 1.25):
        am.drive = drive
        assert am.drive == drive
        y, budget = Am.apply(xs, 0, sp, drive)
        _check_c64(_h(am.apply(_t(xs))), y, budget, "saleh at drive %g" % drive)
    x = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    out = torch.zeros(n, dtype=torch.complex64, device="cuda:0")
    x.copy_(_t(xs))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        am.apply(x, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        am.apply(x, out=out)
    am.drive = 3.0                                      # the graph keeps 1.25
    for seed in (2411, 2412):
        xn = Am.geometry_signal(seed, n)
        x.copy_(_t(xn))
        graph.replay()
        torch.cuda.synchronize()
        got = _h(out).copy()
        am.drive = 1.25
        assert np.array_equal(_bits(got), _bits(_h(am.apply(_t(xn)))))
        am.drive = 3.0
        y, budget = Am.apply(xn, 0, sp, 1.25)
        _check_c64(got, y, budget, "replay with input %d" % seed)


# ---- 9. end to end ----
def _oob(P, c):
    import gfdm_amd
    return gfdm_amd.oob_ratio_db(P, c["K"], c["smap"])


def test_end_to_end():
    """payload bytes -> map -> transmit -> place -> power (mean) -> AMPLIFY (RAPP p = 2, drive from amplifier_drive) -> apply (tap 1 / d,
    the channel loop's CFO and noise) -> detect -> match -> demodulate_bursts -> measure / decode, on the setup of
    tests/test_spectrum_meter_gpu.py::test_end_to_end_received_bursts.  The back-off is the smallest of the ladder 12, 9, 6, 4, 3 dB at
    which tests/test_amplifier_model.py::test_loop_preconditions shows the margins to hold on the restatements: 6 dB.  Asserted: every
    burst detected, matched and decoded right on both receivers; oob_ratio_db of the device chain within 0.01 dB of the host restatement's
    on the downloaded placed stream; after CLIP(A) the meter's exact peak_power() <= A^2 (1 + 2^-21).  Printed, not asserted: OOB, PAPR
    and EVM before and after the amplifier at every rung of the ladder."""
    import gfdm_amd
    c = B.loop_case()
    M, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym = A * M
    nfft = 256
    pts = R.qpsk_points().astype(np.complex64)
    payload = S.pack(S.indices(c["sym"], pts, "qpsk"), 2)
    m = gfdm_amd.SymbolMapper(pts)
    sym = m.map(_t(payload), n_sym)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < 1e-5            # the frames the CPU-side preconditions were checked on
    placed = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE).place(frames, _t(c["starts"]), c["out_len"])[0]
    sm = gfdm_amd.SpectrumMeter(nfft)
    sm.power(placed)
    mean = sm.mean_power()
    assert mean == pytest.approx(float(np.mean(np.abs(C.loop_stream()[0].astype(np.complex128)) ** 2)), rel=1e-4)

    sp = Am.loop_spec()
    am = _model(sp)
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    lm = gfdm_amd.LinkMeter(pts)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    receivers = (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points()))
    for rx in receivers:
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
    placed_h = _h(placed)

    def spectrum(stream):
        """(oob dB, papr dB) of a device stream: Hann 256, every segment of the stream"""
        s = gfdm_amd.SpectrumMeter(nfft)
        s.update(stream)
        s.power(stream)
        return _oob(s.psd(), c), s.papr_db()

    def chain(backoff, check):
        d = gfdm_amd.amplifier_drive(mean, backoff, 1.0)
        am.drive = d
        amplified = am.apply(placed)
        ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, [np.float32(1.0 / d)], C.LOOP_SEED)
        ds = ch.apply(amplified)
        r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
        evm = []
        if check:
            assert int(r["count"][0]) == nb
            lm.reset()
            q = lm.match(r["frame_start"], _t(c["starts"] + c["pcp"]), 1, count=r["count"])
            assert np.array_equal(_h(q["sent_row"]), np.arange(nb)) and np.array_equal(_h(q["ref_row"])[:nb], np.arange(nb))
            t = lm.totals()
            assert (t["detections"], t["matched"], t["missed"], t["false_alarms"]) == (nb, nb, 0, 0)
        for rx in receivers:
            demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
            if check:
                got = _h(m.decode(demod, count=r["count"]))
                assert got.shape == (nb + 3, payload.shape[1]) and np.array_equal(got[:nb], payload) and not got[nb:].any()
            if int(r["count"][0]) == nb:
                e = lm.measure(demod, _t(payload), count=r["count"])
                ep, rp = _h(e["err_power"])[:nb].astype(np.float64), _h(e["ref_power"])[:nb].astype(np.float64)
                evm.append(100.0 * float(np.sqrt(ep.sum() / rp.sum())))
        return d, amplified, evm

    # the chosen back-off: asserted
    d, amplified, evm = chain(Am.LOOP_BACKOFF, True)
    z, zbudget = Am.apply(placed_h, 0, sp, d)                                          # the restatement on the stream the device placed
    _check_c64(_h(amplified), z, zbudget, "amplified loop stream at %g dB" % Am.LOOP_BACKOFF)
    s = gfdm_amd.SpectrumMeter(nfft)
    s.update(amplified)
    o = Sp.stream_origins(nfft, nfft // 2, placed_h.size)
    ref = Sp.psd(z.astype(np.complex64), s.window(), o)
    oob_dev, oob_ref = _oob(s.psd(), c), _oob(ref["psd_sum"], c)
    print("out-of-band ratio at %g dB: device chain %.4f dB, host restatement %.4f dB" % (Am.LOOP_BACKOFF, oob_dev, oob_ref))
    assert abs(oob_dev - oob_ref) <= 0.01
    # a clipper in front of the meter's exact peak
    A_clip = 0.75 * float(np.sqrt(sm.peak_power()))
    clip = gfdm_amd.AmplifierModel.clip(A_clip)
    s = gfdm_amd.SpectrumMeter(nfft)
    s.power(clip.apply(placed))
    A32 = float(np.float32(A_clip))
    print("CLIP(%.4f): peak power %.9e, A^2 %.9e" % (A_clip, s.peak_power(), A32 * A32))
    assert 0 < s.peak_power() <= A32 * A32 * (1 + 2.0 ** -21) and sm.peak_power() > A32 * A32
    # the ladder: printed
    oob0, papr0 = spectrum(placed)
    print("before the amplifier: out-of-band ratio %.2f dB, PAPR %.2f dB" % (oob0, papr0))
    for backoff in Am.LOOP_BACKOFF_LADDER:
        d, amplified, evm = chain(backoff, False)
        oob, papr = spectrum(amplified)
        print("back-off %4.1f dB (drive %.4f): out-of-band ratio %.2f dB, PAPR %.2f dB, EVM %s %% (MF, ZF + IC2)" %
              (backoff, d, oob, papr, " / ".join("%.2f" % v for v in evm) or "not all bursts found"))
