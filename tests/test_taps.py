"""CPU side of the tap tests (no GPU): the oracles are pinned with complex, asymmetric, full-band taps, and the inputs of
tests/test_taps_gpu.py meet the conditions that make its comparisons mean something.

  * fixture pin: both oracles' modulate against pygfdm on the rxl_ctaps_* fixtures (tests/golden/make_golden_taps.py); the receiver side of
    the same files runs through tests/test_oracle.py::test_receiver_oracles_match_pygfdm_at_any_overlap, unchanged;
  * odd overlap, which pygfdm cannot pin (it is a different model there): the two independently written restatements of the C++ lines, numpy
    float64 and plain C float32, against each other on every stage and every tap family;
  * the cases discriminate: on the inputs of every route, every wrong tap handling of tap_cases.mutations moves the float64 result by at
    least 0.1 -- and with root-raised-cosine taps it does not, which is why the families exist;
  * the decision guard keeps at least half of the blocks of every cancellation case."""
import glob
import os

import numpy as np
import pytest

import c_oracle
import gfdm_ref as R
import tap_cases as T
from conftest import GOLDEN_DIR, load_rx_overlap_golden, rel_err

CTAPS = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "rxl_ctaps_*.npz")))


def test_the_tap_fixtures_are_there():
    assert len(CTAPS) == 10 and {load_rx_overlap_golden(n)["L"] % 2 for n in CTAPS} == {0}


@pytest.mark.parametrize("name", CTAPS)
def test_oracles_modulate_matches_pygfdm_with_complex_taps(name):
    """bounds of tests/test_oracle.py for the same comparison: 1e-12 numpy oracle (float64 both), 1e-6 C oracle (float32)"""
    g = load_rx_overlap_golden(name)
    M, K, L = g["M"], g["K"], g["L"]
    nt = R.normalize_taps(g["taps"], M)
    assert np.abs(nt.imag).max() > 0.1 * np.abs(nt).max()                  # complex taps
    co = c_oracle.COracle(M, K, L, g["taps"])
    for sym, ref in ((g["symbols"], g["pygfdm_modulate"]), (g["gauss_symbols"], g["pygfdm_modulate_gauss"])):
        assert rel_err(R.modulate(sym, nt, M, K, L), ref) < 1e-12
        assert rel_err(co.modulate(sym), ref) < 1e-6
    assert np.array_equal(g["frames"], g["pygfdm_modulate"].astype(np.complex64))


@pytest.mark.parametrize("name", CTAPS)
def test_the_fixtures_tell_wrong_tap_handling_apart(name):
    """what the RRC fixtures cannot: every mutation of the taps is at least 0.1 away from the stored model outputs"""
    g = load_rx_overlap_golden(name)
    M, K, L = g["M"], g["K"], g["L"]
    nt = R.normalize_taps(g["taps"], M)
    for mname, mt in T.mutations(nt, M, L):
        assert T.per_block_rel(R.modulate(g["gauss_symbols"], mt, M, K, L), g["pygfdm_modulate_gauss"]).min() > 0.1, mname
        assert T.per_block_rel(R.demodulate(g["gauss"], mt, M, K, L), g["pygfdm_demodulate_fft_loop_gauss"]).min() > 0.1, mname


@pytest.mark.parametrize("M,K,L", T.ODD_SHAPES)
@pytest.mark.parametrize("kind", T.FAMILIES + ("rrc",))
def test_c_oracle_matches_numpy_oracle_at_odd_overlap(M, K, L, kind):
    """every stage, bounds of tests/test_oracle.py::test_c_oracle_matches_numpy_oracle_all_stages"""
    c = T.make_shape_case(M, K, L, 3, kind)
    nt, x, feq, sym = c["nt"], c["xe"], c["feq"], c["sym"]
    o = c_oracle.COracle(M, K, L, c["taps"])
    assert rel_err(o.filter_taps(), nt) < 1e-6
    assert rel_err(o.ic_filter_taps(), R.ic_filter_taps(nt, M, L)) < 1e-6
    assert rel_err(o.modulate(sym), c["x"]) < 1e-5
    assert rel_err(o.modulate(c["gauss"]), R.modulate(c["gauss"], nt, M, K, L)) < 1e-5
    S = R.fft_filter_downsample(x, nt, M, K, L, feq)
    assert rel_err(o.fft_filter_downsample(x, feq), S) < 1e-5
    assert rel_err(o.fft_filter_downsample(c["gauss"]), R.fft_filter_downsample(c["gauss"], nt, M, K, L)) < 1e-5
    assert rel_err(o.transform_subcarriers_to_td(S), R.transform_subcarriers_to_td(S, M, K)) < 1e-5
    assert rel_err(o.cancel_sc_interference(sym, S), R.cancel_sc_interference(sym, S, R.ic_filter_taps(nt, M, L), M, K)) < 1e-5
    assert rel_err(o.demodulate(x, feq), R.demodulate(x, nt, M, K, L, feq)) < 1e-5
    smap = T.subcarrier_map(K, M)
    for pc in (0, 1):
        ref, st = R.advanced_receive(x, nt, M, K, L, smap, R.qpsk_points(), 2, f_eq=feq, kind="qpsk", do_phase_compensation=pc, return_stages=True)
        keep = st["dec_margin"] > T.DECISION_GUARD              # (random taps leave decisions near zero; a float32 decision there may flip)
        assert keep.any()
        assert rel_err(o.advanced_receive(x, smap, R.qpsk_points(), 2, f_eq=feq, kind="qpsk", do_phase_compensation=pc)[keep], ref[keep]) < 1e-5
        assert rel_err(o.advanced_receive(x, smap, R.qpsk_points(), 2, f_eq=feq, kind="nearest", do_phase_compensation=pc)[keep], ref[keep]) < 1e-5


def test_tap_families_are_what_they_say():
    for M, K, L in sorted({r["shape"] for r in T.ROUTES.values()}):
        n = M * L
        mirror = (n - np.arange(n)) % n
        t = T.make_taps("rand", M, K, L)
        assert np.abs(t.imag).min() > 0 and np.abs(t - t[mirror]).max() > 0.1 and np.abs(t).min() > 1e-4
        t = T.make_taps("real_asym", M, K, L)
        assert np.all(t.imag == 0) and np.abs(t - t[mirror]).max() > 0.1
        # cplx_icsym: in float32, as a handle holds them, the products of the two main parts are exactly real and exactly even in m
        t = R.normalize_taps(T.make_taps("cplx_icsym", M, K, L), M).astype(np.complex64)
        assert np.all((t[:M].real == 0) | (t[:M].imag == 0)) and np.abs(t.imag).max() > 0.1
        a, b = t[:M], t[(L - 1) * M:]
        ic = (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)         # float32 arithmetic
        assert ic.dtype == np.complex64 and np.all(ic.imag == 0) and np.array_equal(ic.real, ic.real[(M - np.arange(M)) % M])
        g = np.fft.ifft(ic.astype(complex)) / M
        assert np.abs(g.imag).max() < 1e-15 * np.abs(g).max() and np.abs(g - g[(M - np.arange(M)) % M]).max() < 1e-15 * np.abs(g).max()
        t = T.make_taps("imag", M, K, L)
        assert np.all(t.real == 0) and np.array_equal(t.imag, T.make_taps("rrc", M, K, L).real)


@pytest.mark.parametrize("route", sorted(T.ROUTES))
def test_every_mutation_moves_the_result_on_the_routes_inputs(route):
    """A condition on the inputs, checked with the reference alone: with `rand` taps every wrong tap handling changes R.modulate and
    R.demodulate of the route's own blocks by at least 0.1 relative (every block), four orders of magnitude above TOL."""
    c = T.make_case(route, "rand")
    M, K, L, nt = c["M"], c["K"], c["L"], c["nt"]
    names = []
    for mname, mt in T.mutations(nt, M, L):
        names.append(mname)
        for sym in (c["sym"], c["gauss"]):
            assert T.per_block_rel(R.modulate(sym, mt, M, K, L), R.modulate(sym, nt, M, K, L)).min() > 0.1, mname
        for x in (c["x"], c["gauss"]):
            assert T.per_block_rel(R.demodulate(x, mt, M, K, L), R.demodulate(x, nt, M, K, L)).min() > 0.1, mname
        assert T.per_block_rel(R.demodulate(c["xe"], mt, M, K, L, c["feq"]), R.demodulate(c["xe"], nt, M, K, L, c["feq"])).min() > 0.1, mname
    assert names == ["conj", "mirror", "swap_main", "shift1"] + (["swap_outer", "zero_outer"] if L >= 4 else [])


def test_rrc_taps_are_blind_to_the_same_mutations():
    """the blindness that motivates the families: with RRC taps conj and mirror are the same function, and at the reference's overlap-4 QA
    shape a kernel may drop the outer tap parts and stay inside TOL"""
    for route, blind, bound in (("rowlane_wave", ("conj", "mirror"), 1e-12), ("rader_l4", ("conj", "mirror"), 1e-12), ("rader_l4", ("zero_outer",), T.TOL)):
        c = T.make_case(route, "rrc")
        M, K, L, nt = c["M"], c["K"], c["L"], c["nt"]
        muts = dict(T.mutations(nt, M, L))
        for mname in blind:
            assert rel_err(R.modulate(c["sym"], muts[mname], M, K, L), c["x"]) < bound, mname
            assert rel_err(R.demodulate(c["x"], muts[mname], M, K, L), R.demodulate(c["x"], nt, M, K, L)) < bound, mname
            assert rel_err(R.demodulate(c["gauss"], muts[mname], M, K, L), R.demodulate(c["gauss"], nt, M, K, L)) < bound, mname


@pytest.mark.parametrize("route", sorted(T.ROUTES))
@pytest.mark.parametrize("kind", T.FAMILIES)
def test_decision_guard_keeps_at_least_half_of_the_blocks(route, kind):
    """a condition, not a measurement: the oracle alone keeps at least half of the IC_BLOCKS blocks of every cancellation case (the GPU test
    asserts the same count before it compares)"""
    c = T.make_ic_case(route, kind)
    for rule, _, _ in T.RULES:
        for inp in ("mf", "zf"):
            keep = c["keep_%s_%s" % (inp, rule)]
            print(route, kind, inp, rule, int(keep.sum()))
            assert 2 * keep.sum() >= T.IC_BLOCKS, (inp, rule, int(keep.sum()))


@pytest.mark.parametrize("name", ["rowlane_7", "rowlane_jit", "generic_5_32"])
def test_burst_restatement_with_random_taps_discriminates(name):
    """the burst cases test_taps_gpu.py runs with taps_kind="rand" (plain demodulation): the default argument leaves the existing cases as
    they were, and the float64 restatement moves by at least 0.1 under every wrong tap handling"""
    from burst_receive_cases import CASES, make_case, restatement, virtual_bursts
    base, same = make_case(*CASES[name]), make_case(*CASES[name], taps_kind="rrc")
    assert all(np.array_equal(base[k], same[k]) for k in base)
    c = dict(make_case(*CASES[name], taps_kind="rand"))
    assert np.array_equal(c["taps"], T.make_taps("rand", c["M"], c["K"], c["L"]))
    e = virtual_bursts(c["stream"], c["starts"], c["sc_rot"], 0, c["F"])
    ref, _ = restatement(c, e, None)
    assert np.isfinite(ref).all()
    for mname, mt in T.mutations(c["nt"], c["M"], c["L"]):
        got, _ = restatement(dict(c, nt=mt), e, None)
        assert T.per_block_rel(got, ref).min() > 0.1, mname
