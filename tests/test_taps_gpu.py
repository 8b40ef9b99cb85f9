"""GPU tap tests: every kernel family with complex, asymmetric, full-band taps (tests/tap_cases.py: families, ROUTES).

The other parity tests use root-raised-cosine taps, on which a kernel that conjugates the taps, reads a part back to front, swaps the
cross terms of the complex product or (at overlap 4) drops the outer parts computes the same thing; tests/test_taps.py asserts that, and
that on the inputs used here every such mistake is at least 0.1 away.  Bounds are the project's own: TOL = 1e-5 per-block relative L2
against the float64 oracle, 2e-6 between two forms of the same sum.  Every comparison goes through check_err with a tag
taps_<route>_<family>_<entry>, so GFDM_ERRLOG collects the measured errors (profiles/r03/tap_error_table.md).

  a. every route x {rand, real_asym, cplx_icsym}: every entry point of the modulator, the receiver and the advanced receiver;
  b. the flag cross: a complex filter in front of the real-symmetric and the matrix-core cancellation rounds (cplx_icsym); the other
     combination, a real filter in front of the general rounds, is real_asym in (a);
  c. known answers that need no oracle: f(1j t) = 1j f(t); imaginary parts below the host's real-taps threshold change no bit; one above it
     changes nothing beyond 2e-6;
  d. the fused parts: transmitter (mapped, framed), frames in, estimator in front, bursts from a capture;
  e. the pybind11 modulator on the rxl_ctaps_* fixtures."""
import contextlib

import numpy as np
import pytest

import c_oracle
import gfdm_ref as R
import tap_cases as T
from burst_receive_cases import CASES as BURST_CASES, make_case as make_burst_case
from conftest import assert_places, check_err, have_gpu, load_rx_overlap_golden, rel_err
from test_taps import CTAPS

pytestmark = pytest.mark.gpu
TOL, CROSS = T.TOL, T.CROSS


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@contextlib.contextmanager
def _setting(setter, mode):
    """a process-wide creation-time switch (set_ic_matrix_cores / set_dft_matrix_cores), restored afterwards; None: untouched"""
    if mode is None:
        yield
        return
    prev = setter(mode)
    try:
        yield
    finally:
        setter(prev)


@contextlib.contextmanager
def _creating(route, generic=None, ic_mx=None):
    """the context in which the handles of a route are created"""
    import gfdm_amd
    r = T.ROUTES[route]
    with contextlib.ExitStack() as es:
        if r.get("generic") if generic is None else generic:
            es.enter_context(gfdm_amd.generic_family_for_testing())
        es.enter_context(_setting(gfdm_amd.set_ic_matrix_cores, ic_mx))
        es.enter_context(_setting(gfdm_amd.set_dft_matrix_cores, r.get("dft_mx")))
        yield


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pair(route, taps):
    """(Modulator, Demodulator) of a route with the given taps, kernel_name() asserted: a route cannot silently change"""
    import gfdm_amd
    M, K, L = T.ROUTES[route]["shape"]
    with _creating(route):
        mod, dem = gfdm_amd.Modulator(M, K, L, taps), gfdm_amd.Demodulator(M, K, L, taps)
    assert (mod.kernel_name(), dem.kernel_name()) == (T.ROUTES[route]["kernel"],) * 2
    return mod, dem


def _advanced(route, c, decision, pts, **how):
    import gfdm_amd
    with _creating(route, **how):
        return gfdm_amd.AdvancedReceiver(c["M"], c["K"], c["L"], c["taps"], c["smap"], T.IC_ITER, pts, decision=decision)


def _ic_inputs(c):
    return (("mf", c["x"], None), ("zf", c["xe"], c["feq"]))


def _ic_run(adv, x, feq):
    return adv.demodulate(x) if feq is None else adv.demodulate_equalize(x, feq)


# ---------------------------------------------------------------- a. every route, every family, every entry point

@pytest.mark.parametrize("kind", T.FAMILIES)
@pytest.mark.parametrize("route", sorted(T.ROUTES))
def test_every_entry_point_with_asymmetric_taps(route, kind):
    c = T.make_case(route, kind)
    M, K, L, nt, ic = c["M"], c["K"], c["L"], c["nt"], c["ic"]
    sym, gauss, x, xe, feq = c["sym"], c["gauss"], c["x"], c["xe"], c["feq"]
    mod, dem = _pair(route, c["taps"])

    def err(entry, got, ref, tol=TOL):
        check_err("taps_%s_%s_%s" % (route, kind, entry), rel_err(got, ref), tol)
    err("filter_taps_mod", mod.filter_taps(), nt, 1e-6)
    err("filter_taps", dem.filter_taps(), nt, 1e-6)
    err("ic_filter_taps", dem.ic_filter_taps(), ic, 1e-6)
    err("modulate", mod.modulate(sym), x)
    err("modulate_gauss", mod.modulate(gauss), R.modulate(gauss, nt, M, K, L))
    S = R.fft_filter_downsample(x, nt, M, K, L)
    err("fd", dem.fft_filter_downsample(x), S)
    err("fd_gauss", dem.fft_filter_downsample(gauss), R.fft_filter_downsample(gauss, nt, M, K, L))
    err("fdeq", dem.fft_equalize_filter_downsample(xe, feq), R.fft_filter_downsample(xe, nt, M, K, L, feq))
    err("demodulate", dem.demodulate(x), R.demodulate(x, nt, M, K, L))
    err("demodulate_gauss", dem.demodulate(gauss), R.demodulate(gauss, nt, M, K, L))
    zf = dem.demodulate_equalize(xe, feq)
    err("demodulate_equalize", zf, R.demodulate(xe, nt, M, K, L, feq))
    err("demodulate_equalize_gauss", dem.demodulate_equalize(gauss, feq), R.demodulate(gauss, nt, M, K, L, feq))
    err("to_td", dem.transform_subcarriers_to_td(S), R.transform_subcarriers_to_td(S, M, K))
    err("cancel", dem.cancel_sc_interference(sym, S), R.cancel_sc_interference(sym, S, ic, M, K))
    # and the plain-C float32 oracle agrees with the GPU to float32 noise as well
    err("c_oracle", zf, c_oracle.COracle(M, K, L, c["taps"]).demodulate(xe, feq))

    # the advanced receiver: IC_ITER rounds, MF and ZF input, a partial subcarrier map, both decision rules; guarded blocks only
    ci = T.make_ic_case(route, kind)
    for rule, decision, pts in T.RULES:
        adv = _advanced(route, ci, decision, pts)
        assert adv.kernel_name() == T.ROUTES[route]["kernel"] and adv.decision_rule() == rule
        for inp, src, eq in _ic_inputs(ci):
            keep = ci["keep_%s_%s" % (inp, rule)]
            assert 2 * keep.sum() >= T.IC_BLOCKS                      # as tests/test_taps.py
            err("ic_%s_%s" % (inp, rule), _ic_run(adv, src, eq)[keep], ci["ref_%s_%s" % (inp, rule)][keep])


# ---------------------------------------------------------------- b. complex filter, real-symmetric / matrix-core cancellation rounds

@pytest.mark.parametrize("route", ["rowlane_wave", "rowlane_multiwave", "rowlane_jit_l4"])
def test_complex_filter_with_real_symmetric_cancellation_kernel(route):
    """cplx_icsym: handles created under set_ic_matrix_cores(2) (matrix-core rounds wherever the form applies) and (0) (vector ALU): each
    against the oracle, against each other, and against the same handle kind of the generic family"""
    ci = T.make_ic_case(route, "cplx_icsym")
    pts = R.qpsk_points()
    mx, va = _advanced(route, ci, "auto", pts, ic_mx=2), _advanced(route, ci, "auto", pts, ic_mx=0)
    gen = _advanced(route, ci, "auto", pts, generic=True)
    assert (mx.kernel_name(), va.kernel_name(), gen.kernel_name()) == (T.ROUTES[route]["kernel"],) * 2 + ("generic_lds",)
    for inp, src, eq in _ic_inputs(ci):
        keep, ref = ci["keep_%s_qpsk" % inp], ci["ref_%s_qpsk" % inp]
        assert 2 * keep.sum() >= T.IC_BLOCKS
        a, b, g = (_ic_run(h, src, eq)[keep] for h in (mx, va, gen))
        tag = "taps_%s_cplx_icsym_cross_%s_" % (route, inp)
        check_err(tag + "mx", rel_err(a, ref[keep]), TOL)
        check_err(tag + "valu", rel_err(b, ref[keep]), TOL)
        check_err(tag + "generic", rel_err(g, ref[keep]), TOL)
        check_err(tag + "mx_vs_valu", rel_err(a, b), CROSS)
        check_err(tag + "mx_vs_generic", rel_err(a, g), CROSS)
        check_err(tag + "valu_vs_generic", rel_err(b, g), CROSS)


# ---------------------------------------------------------------- c. known answers

@pytest.mark.parametrize("route", ["rowlane_wave", "rowlane_multiwave", "generic_lds_12", "rader_l4"])
def test_known_answer_relations_of_the_taps(route):
    c = T.make_case(route, "rrc")
    M, K, L = c["M"], c["K"], c["L"]
    sym, x = c["sym"], c["x"]
    rrc = c["taps"]
    tmax = np.abs(rrc).max()

    def run(taps):
        mod, dem = _pair(route, taps)
        return dict(modulate=mod.modulate(sym), demodulate=dem.demodulate(x), fd=dem.fft_filter_downsample(x)), dem.filter_taps()
    real, _ = run(rrc)
    # every entry point is linear in the taps: f(1j t) = 1j f(t)
    imag, _ = run(T.make_taps("imag", M, K, L))
    for k in real:
        check_err("taps_%s_imag_%s" % (route, k), rel_err(imag[k], 1j * real[k]), CROSS)
    # imaginary parts below the real-taps threshold: the same bits as with none, and filter_taps() still returns the taps as given
    below, ft = run(rrc + 1e-14j * tmax)
    for k in real:
        assert np.array_equal(_bits(below[k]), _bits(real[k])), k
    want = R.normalize_taps(rrc + 1e-14j * tmax, M)
    assert np.all(ft.imag > 0) and np.abs(ft.imag / want.imag - 1).max() < 1e-6 and rel_err(ft, want) < 1e-6
    # one imaginary part above it: the complex filter, the same result to rounding
    t = rrc.copy()
    t[int(np.argmax(np.abs(rrc)))] += 1e-9j * tmax
    above, _ = run(t)
    for k in real:
        check_err("taps_%s_above_%s" % (route, k), rel_err(above[k], real[k]), CROSS)


# ---------------------------------------------------------------- d. the fused parts

@pytest.mark.parametrize("generic", [False, True])
def test_transmitter_with_asymmetric_taps(generic):
    """the three variants of the modulator kernel: plain (Modulator), mapper in front (Transmitter.modulate) and mapper + cyclic prefix / suffix, ramp and preamble behind (transmit), arguments of
    tests/test_transmitter_gpu.py::test_transmitter_generic_family_and_validation"""
    import gfdm_amd
    M, K, L = 5, 32, 2
    rng = np.random.default_rng(532)
    taps = T.make_taps("rand", M, K, L)
    nt = R.normalize_taps(taps, M)
    smap = np.concatenate((np.arange(1, 13), np.arange(20, 32)))
    A, cp, cs, ramp = len(smap), 5, 3, 2
    window = np.concatenate((np.linspace(0.1, 0.9, ramp), np.ones(M * K + cp + cs - 2 * ramp), np.linspace(0.9, 0.1, ramp))).astype(complex)
    pre = [T._gauss(rng, 11) for _ in range(2)]
    for per_ts in (True, False):
        with (gfdm_amd.generic_family_for_testing() if generic else contextlib.nullcontext()):
            tx = gfdm_amd.Transmitter(M, K, A, cp, cs, ramp, smap[::-1], per_ts, L, taps, window, [0, 2], pre)
            mod = gfdm_amd.Modulator(M, K, L, taps)
        assert tx.kernel_name() == mod.kernel_name() == ("generic_lds" if generic else "rowlane")
        tag = "taps_tx_%s_rand_%s_" % ("generic" if generic else "rowlane", "ts" if per_ts else "sc")
        grid = T.qpsk(rng, (19, M * K))
        check_err(tag + "plain", rel_err(mod.modulate(grid), R.modulate(grid, nt, M, K, L)), TOL)
        sym = T.qpsk(rng, (19, A * M - 3))                      # fewer symbols than slots: the rest is zero
        check_err(tag + "mapped", rel_err(tx.modulate(sym, A * M - 3), R.modulate(R.map_to_resources(sym, M, K, smap, per_ts), nt, M, K, L)), TOL)
        frames = tx.transmit(sym, ninput_size=A * M - 3)
        for port, s in enumerate((0, 2)):
            check_err(tag + "framed%d" % port, rel_err(frames[port], R.transmit(sym, nt, M, K, L, smap, per_ts, cp, cs, ramp, window, s, pre[port])), TOL)


@pytest.mark.parametrize("route", ["rowlane_wave", "rowlane_jit_mixed"])
def test_frames_in_with_asymmetric_taps(route):
    import gfdm_amd
    c = T.make_case(route, "rand")
    M, K, L, N, nt = c["M"], c["K"], c["L"], c["N"], c["nt"]
    smap = T.subcarrier_map(K, M)
    framed = lambda a: np.concatenate((a[:, -6:], a, a[:, :3]), axis=1)
    for per_ts in (True, False):
        with _creating(route):
            dem = gfdm_amd.Demodulator(M, K, L, c["taps"])
        assert dem.kernel_name() == T.ROUTES[route]["kernel"]
        dem.configure_frames(N + 9, 6, smap, per_ts)
        tag = "taps_%s_rand_frames_%s" % (route, "ts" if per_ts else "sc")
        check_err(tag, rel_err(dem.demodulate_frames(framed(c["x"])), R.demap_from_resources(R.demodulate(c["x"], nt, M, K, L), M, K, smap, per_ts)), TOL)
        check_err(tag + "_eq", rel_err(dem.demodulate_frames(framed(c["xe"]), c["feq"]),
                                       R.demap_from_resources(R.demodulate(c["xe"], nt, M, K, L, c["feq"]), M, K, smap, per_ts)), TOL)


@pytest.mark.parametrize("name", ["rowlane_7", "rowlane_jit", "generic_5_32"])
def test_estimated_and_burst_receivers_with_asymmetric_taps(name):
    """demodulate_estimated (estimator in front) and demodulate_bursts (bursts straight from the capture), plain demodulation, `rand` taps:
    the acceptance tests/test_burst_receive_gpu.py applies to the same routes (fused against the two-step path, and both against the
    float64 restatement)"""
    from test_burst_receive_gpu import KERNEL, _accept, _receivers, _t
    c = make_burst_case(*BURST_CASES[name], taps_kind="rand")
    ds, offs, rot = _t(c["stream"]), _t(c["starts"]), _t(c["sc_rot"])
    rx = _receivers(c, name == "generic_5_32")[0]
    assert rx.kernel_name() in KERNEL[name]
    _accept("taps_%s_rand_dem" % name, c, rx, None, ds, offs, rot)


# ---------------------------------------------------------------- e. pybind11

@pytest.mark.parametrize("name", CTAPS)
def test_pybind_modulator_on_the_tap_fixtures(name):
    """(the Demodulator side of the same files: tests/test_parity_gpu.py::test_golden_demodulator_any_overlap)"""
    import gfdm_python
    g = load_rx_overlap_golden(name)
    mod = gfdm_python.Modulator(g["M"], g["K"], g["L"], g["taps"])
    for which, sym, ref in (("qpsk", g["symbols"], g["pygfdm_modulate"]), ("gauss", g["gauss_symbols"], g["pygfdm_modulate_gauss"])):
        for b in range(sym.shape[0]):
            check_err("taps_pybind_%s_%s" % (name, which), rel_err(mod.modulate(sym[b]), ref[b]), TOL)
    assert_places(mod.modulate(g["symbols"][0]), g["pygfdm_modulate"][0], 5)
