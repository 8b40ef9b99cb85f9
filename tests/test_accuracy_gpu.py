"""GPU accuracy tests: every kernel route held to the float32 reference's own error budget, and to exact power-of-two homogeneity
(tests/accuracy_cases.py: ROUTES, figures, bounds; the method is pinned on the CPU by tests/test_accuracy.py).

  budget       On every route, with RRC and with `rand` taps, every entry point of the modulator, the receiver and the advanced receiver
               (2 rounds, MF and ZF input, guarded blocks; vector-ALU rounds, matrix-core rounds on the *_ic_mx routes) is compared with
               the float64 oracle by three figures -- l2, peak, pos -- and each figure is bounded by 2 (peak: 3) times the figure the
               plain-C float32 oracle reaches on the same call, computed here next to the GPU's.  Every comparison goes through check_err
               with a tag acc_<route>_<taps>_<entry>_<figure> (accref_...: the C oracle's figure, against TOL), so GFDM_ERRLOG
               collects figure, bound and reference (profiles/r03/accuracy_budget_table.md).  Transmitter.transmit against COracleTx on three routes.
  homogeneity  Scaling by a power of two commutes with every float32 rounding while nothing over- or underflows, so a linear kernel must
               return the scaled BITS: no reference, no tolerance.  One launch per entry point whose block b is multiplied by 2^k, k
               cycling through (0, -40, +15, +40) -- neighbours of wildly different magnitude share wavefronts on the 2-per-wave and
               K = 4 routes -- must equal 2^k times the unscaled launch, block by block.  x and f_eq (block and rx preamble) scaled
               together must leave the equalised (self-estimating) calls bit-identical.  The cancellation rounds subtract unit symbols and
               are not homogeneous: the advanced receiver is covered at ic_iter = 0.

Measured on an MI355X (1272 comparisons): l2 0.26 to 1.19, pos 0.22 to 1.45 and peak 0.27 to 2.06 times the C oracle's figure, medians
0.9; no route needs a margin above 2 (peak: 3), and every entry point, divisions by f_eq included, is bit-homogeneous on every route
(transmitter, estimator and self-estimating receiver on the deep and the four-subcarrier routes too).  The matrix-core rounds differ
from the vector-ALU rounds in bits and by 5e-8 to 6e-8 in L2.  With the device
tap table cut to 18 mantissa bits every budget test fails and every homogeneity test still passes (a cut table is still linear)."""
import contextlib

import numpy as np
import pytest

import accuracy_cases as A
import c_oracle
import gfdm_ref as R
import poison_cases as P
from conftest import check_err, have_gpu, rel_err
from test_poison_gpu import _setting

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@contextlib.contextmanager
def _creating(route, routes=A.ROUTES, **override):
    """the context in which the handles of a route are created (as tests/test_poison_gpu.py, on the routes of accuracy_cases)"""
    import gfdm_amd
    r = dict(routes[route], **override)
    with contextlib.ExitStack() as es:
        if r.get("generic"):
            es.enter_context(gfdm_amd.generic_family_for_testing())
        es.enter_context(_setting(gfdm_amd.set_ic_matrix_cores, r.get("ic_mx")))
        es.enter_context(_setting(gfdm_amd.set_dft_matrix_cores, r.get("dft_mx")))
        yield


def _handles(route, c, ic_iter=A.IC_ITER, routes=A.ROUTES, **override):
    """Modulator, Demodulator and AdvancedReceiver of a route behind the calls of accuracy_cases.Handles, kernel_name() asserted: a route
    cannot silently change.  A route of another list (routes) that says adv=False gets no AdvancedReceiver."""
    import gfdm_amd
    M, K, L = c["M"], c["K"], c["L"]
    with _creating(route, routes, **override):
        mod, dem = gfdm_amd.Modulator(M, K, L, c["taps"]), gfdm_amd.Demodulator(M, K, L, c["taps"])
        adv = gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], ic_iter, R.qpsk_points()) if routes[route].get("adv", True) else None
    assert (mod.kernel_name(), dem.kernel_name()) == (routes[route]["kernel"],) * 2
    if adv is not None:
        assert adv.kernel_name() == routes[route]["kernel"]
        assert adv.decision_rule() == "qpsk" and adv.get_phase_compensation() == 0 and adv.get_ic() == ic_iter
    return A.Handles(mod, dem, adv)


class _Findings:
    """collects every failed comparison of a test, so that one run shows all of a route's figures"""

    def __init__(self):
        self.lines = []

    def check(self, tag, err, bound, where=""):
        try:
            check_err(tag, err, bound)
        except AssertionError as e:
            self.lines.append("%s  [%s]" % (e, where))

    def same_bits(self, what, got, want):
        got, want = np.asarray(got).reshape(np.asarray(want).shape), np.asarray(want)
        if np.array_equal(P.bits(got), P.bits(want)):
            return
        bad = (P.bits(got) != P.bits(want)).reshape(want.shape[0], -1)
        blocks = np.flatnonzero(bad.any(axis=1))
        with np.errstate(all="ignore"):
            rel = np.abs(got - want)[blocks].max(axis=-1) / np.abs(want)[blocks].max(axis=-1)
        self.lines.append("%s: %d words differ in blocks %s (k = %s), largest difference %.2e of the block's peak"
                          % (what, int(bad.sum()), blocks[:8].tolist(), [A.SCALES[b % len(A.SCALES)] for b in blocks[:8]], float(np.nanmax(rel))))

    def done(self):
        assert not self.lines, "\n".join(self.lines)


def _tx_kernels(route):
    """(the Rader kernels serve plain blocks; the transmitter of that shape may stay on the generic kernels)"""
    k = A.ROUTES[route]["kernel"]
    return (k, "generic_lds") if k == "generic_rader" else (k,)


# ---------------------------------------------------------------- budget

def _budget(found, tag, kind, c, ref, h, entries, margin):
    """every entry against its bound: check_err tags acc_<tag>_<taps>_<entry>_<figure>, accref_... the C oracle's figure, accmargin_... the margin"""
    for e in entries:
        assert 2 * A.keep(c, e).sum() >= c["B"]                          # as tests/test_accuracy.py
        assert 0 < ref[e]["l2"] < A.REF_L2_CAP
        bound = A.bounds(ref[e], margin)
        figs, got, want = h.figures(e, c)
        print("%s %s %-20s " % (tag, kind, e) + "  ".join("%s %.2e / %.2e (ref %.2e)" % (f, figs[f], bound[f], ref[e][f]) for f in A.FIGURES))
        for f in A.FIGURES:
            found.check("accref_%s_%s_%s_%s" % (tag, kind, e, f), ref[e][f], A.TOL)            # the C oracle's figure, for the ratio table
            found.check("accmargin_%s_%s_%s_%s" % (tag, kind, e, f), margin[f], 4.0 + 1e-9)         # the cap of every margin
            found.check("acc_%s_%s_%s_%s" % (tag, kind, e, f), figs[f], bound[f], A.where(got, want))


@pytest.mark.parametrize("route,kind", A.CASES)
def test_every_entry_point_within_the_float32_budget(route, kind):
    c = A.make_case(route, kind)
    ref = A.reference_figures(route, kind)
    h = _handles(route, c)
    found = _Findings()
    _budget(found, route, kind, c, ref, h, A.ROUTES[route]["entries"], A.ROUTES[route]["margin"])
    if A.ROUTES[route]["ic_mx"] == 2:
        # kernel_name() is the same for both forms of the rounds.  That this route runs another one than the vector-ALU routes shows in
        # the result: the same sums in another order (f16 operand terms, f32 sums) agree to rounding and differ in some bits.
        va = _handles(route, c, ic_mx=0)
        for e in A.IC:
            a, b = h.run(e, c), va.run(e, c)
            assert not np.array_equal(P.bits(a), P.bits(b)), "%s %s: bit-identical to the vector-ALU rounds, the matrix-core form is not in use" % (route, e)
            k = A.keep(c, e)
            check_err("acc_%s_%s_%s_mx_vs_valu" % (route, kind, e), rel_err(a[k], b[k]), 2e-6)          # two forms of the same sum (tap_cases.CROSS)
    found.done()


@pytest.mark.parametrize("route", A.TX_ROUTES)
def test_transmitter_within_the_float32_budget(route):
    """Transmitter.transmit against COracleTx: a partial map, cyclic prefix 5, suffix 3, ramp 2, cyclic shifts 0 and 2, a preamble; the
    frames behind the preamble are compared, the preamble itself is a copy"""
    import gfdm_amd
    c = A.make_tx_case(route)
    with _creating(route):
        tx = gfdm_amd.Transmitter(*A.tx_args(c))
    assert tx.kernel_name() == A.ROUTES[route]["kernel"]
    otx = c_oracle.COracleTx(*A.tx_args(c))
    frames = tx.transmit(c["sym"])
    found = _Findings()
    for port in range(len(A.TX_SHIFTS)):
        want = c["refs"][port][:, A.TX_PRE:]
        ref = A.figures(otx.work(c["sym"], port)[:, A.TX_PRE:], want)
        assert 0 < ref["l2"] < A.REF_L2_CAP
        assert np.array_equal(P.bits(frames[port][:, :A.TX_PRE]), P.bits(np.broadcast_to(c["pre"][port].astype(np.complex64), (c["B"], A.TX_PRE))))
        got = frames[port][:, A.TX_PRE:]
        figs, bound = A.figures(got, want), A.bounds(ref, A.ROUTES[route]["margin"])
        print("%s port %d " % (route, port) + "  ".join("%s %.2e / %.2e (ref %.2e)" % (f, figs[f], bound[f], ref[f]) for f in A.FIGURES))
        for f in A.FIGURES:
            found.check("accref_%s_rand_transmit%d_%s" % (route, port, f), ref[f], A.TOL)
            found.check("accmargin_%s_rand_transmit%d_%s" % (route, port, f), A.ROUTES[route]["margin"][f], 4.0 + 1e-9)
            found.check("acc_%s_rand_transmit%d_%s" % (route, port, f), figs[f], bound[f], A.where(got, want))
    found.done()


# ---------------------------------------------------------------- exact power-of-two homogeneity

HOMOGENEOUS = [(r, k) for r, k in A.CASES if A.ROUTES[r]["entries"] == A.PLAIN + A.IC]


@pytest.mark.parametrize("route,kind", HOMOGENEOUS)
def test_power_of_two_scaling_returns_the_scaled_bits(route, kind):
    """modulate, fft_[equalize_]filter_downsample, demodulate[_equalize] (x scaled, f_eq fixed), transform_subcarriers_to_td,
    cancel_sc_interference (td and fd scaled together), the advanced receiver at ic_iter = 0; x and f_eq scaled together."""
    c = A.make_case(route, kind)
    B = c["B"]
    s = A.block_scales(B)
    found = _Findings()
    for what, h, entries in (("", _handles(route, c), A.PLAIN), ("ic_iter=0 ", _handles(route, c, ic_iter=0), A.IC)):
        for e in entries:
            plain, scaled = h.run(e, c), h.run(e, c, sx=s)
            assert np.isfinite(plain).all() and np.isfinite(scaled).all(), e
            found.same_bits("%s %s %s%s" % (route, kind, what, e), scaled, A.times(plain, s))
            if e in ("fdeq", "demodulate_equalize", "ic_zf"):
                for k in A.JOINT:
                    both = np.full(B, 2.0 ** k)
                    found.same_bits("%s %s %s%s, x and f_eq times 2^%d" % (route, kind, what, e, k), h.run(e, c, sx=both, sf=both), plain)
    found.done()


@pytest.mark.parametrize("route", sorted(r for r, k in HOMOGENEOUS if k == "rand"))
def test_power_of_two_scaling_of_transmitter_and_estimator(route):
    """Transmitter.transmit (the data part of every frame scales, the preamble samples stay), ChannelEstimator.estimate_frame (rx preamble
    scaled), and demodulate_estimated with block and rx preamble scaled together (bit-identical output); every route, the four-subcarrier ones (two active subcarriers) included."""
    import gfdm_amd
    c = A.make_tx_case(route)
    M, K, L, B = c["M"], c["K"], c["L"], c["B"]
    s = A.block_scales(B)
    found = _Findings()
    with _creating(route):
        tx = gfdm_amd.Transmitter(*A.tx_args(c))
    assert tx.kernel_name() in _tx_kernels(route)
    plain, scaled = tx.transmit(c["sym"]), tx.transmit(c["sym"] * s[:, None])
    for port in range(len(A.TX_SHIFTS)):
        assert np.isfinite(scaled[port]).all()
        found.same_bits("%s transmit port %d, preamble" % (route, port), scaled[port][:, :A.TX_PRE], plain[port][:, :A.TX_PRE])
        found.same_bits("%s transmit port %d" % (route, port), scaled[port][:, A.TX_PRE:], A.times(plain[port][:, A.TX_PRE:], s))
    Act, smap = A.active(K)
    pre, rx = A.estimator_inputs(K, B)
    cc = A.make_case(route, "rand")
    with _creating(route):
        est = gfdm_amd.ChannelEstimator(M, K, Act, True, 1, pre)
        dem = gfdm_amd.Demodulator(M, K, L, cc["taps"])
    assert dem.kernel_name() == A.ROUTES[route]["kernel"]
    e0, e1 = est.estimate_frame(rx), est.estimate_frame(rx * s[:, None])
    assert np.isfinite(e0).all() and np.isfinite(e1).all()
    found.same_bits("%s estimate_frame [%s]" % (route, est.kernel_name()), e1, A.times(e0, s))
    dem.set_channel_estimator(est)
    d0 = dem.demodulate_estimated(cc["xe"], rx)
    assert np.isfinite(d0).all()
    for k in A.JOINT:
        found.same_bits("%s demodulate_estimated, block and rx preamble times 2^%d" % (route, k), dem.demodulate_estimated(cc["xe"] * 2.0 ** k, rx * 2.0 ** k), d0)
    dem.set_channel_estimator(None)
    found.done()
