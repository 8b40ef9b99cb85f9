"""CPU side of the accuracy tests (no GPU): the method of tests/test_accuracy_gpu.py is pinned with the two oracles alone.

tests/accuracy_cases.py bounds every error figure of a kernel route by a small multiple of the figure the plain-C float32 oracle reaches
on the same inputs.  Here the C oracle stands in for a kernel:

  * reference figures: on every route's inputs its worst per-block L2 error stays below 5e-7, so no l2 bound rises above 1e-6, and two
    seeds give the same l2 to a few percent (median below 5%; every case within 20%, within sqrt 2 where blocks are shorter than 100 samples);
  * mutations: three defects the project's TOL = 1e-5 lets through are caught by the bounds on every route -- except where arithmetic
    rules it out, each exception asserted: the tap cut stays inside the bounds of one case (accuracy_cases.CUT_STAYS_INSIDE), a 1e-6
    position error is only held to the bound where the reference's own per-position figure is below 4.5e-7 (the plain timeslot
    transforms on every route), and a 1e-4 element error passes TOL only from N = 101 on;
  * no false alarm: the unmutated C oracle on a second seed passes against the first seed's bounds;
  * the decision guard keeps at least half of the blocks of every cancellation case;
  * the C oracle is exactly homogeneous under powers of two, the property the GPU tests ask of the kernels without any tolerance."""
import numpy as np
import pytest

import accuracy_cases as A
import poison_cases as P
from conftest import rel_err

TOL = A.TOL


def test_the_routes_are_the_ones_the_method_is_about():
    import tap_cases as T
    assert set(T.ROUTES) < set(A.ROUTES) and len(T.ROUTES) == 15
    assert {"rowlane_2_per_wave_ic_mx", "rowlane_wave_ic_mx"} < set(A.ROUTES)
    deep = {A.ROUTES[r]["shape"]: A.ROUTES[r] for r in A.ROUTES if r.startswith("deep_")}
    assert set(deep) == {(9, 200, 2), (9, 31, 2), (37, 32, 2), (15, 1024, 2)} and all(d["kernel"] == "rowlane_jit" for d in deep.values())
    assert deep[(15, 1024, 2)]["B"] == 4 and A.ROUTES["generic_global"]["B"] == 8
    for r in A.ROUTES.values():
        M, K, _ = r["shape"]
        assert r["B"] >= 64 or M * K > 1024
        # margins: 2 (l2, pos) and 3 (peak); an exception needs a written count of roundings and stays at or below 4
        assert r["margin"] == A.MARGIN or (max(r["margin"].values()) <= 4.0 and r.get("roundings"))
    assert A.MARGIN == {"l2": 2.0, "pos": 2.0, "peak": 3.0}


def test_the_figures_are_what_they_say():
    rng = np.random.default_rng(0)
    b = rng.standard_normal((5, 12)) + 1j * rng.standard_normal((5, 12))
    a = b.copy()
    a[3, 7] += 0.5
    a[:, 2] += 0.01
    rms = np.sqrt(np.mean(np.abs(b) ** 2, axis=-1))
    f = A.figures(a, b)
    assert abs(f["l2"] - rel_err(a, b)) < 1e-15
    assert abs(f["peak"] - 0.5 / rms[3]) < 1e-12
    assert abs(f["pos"] - np.sqrt(np.mean(np.array([0.5 / rms[3] if i == 3 else 0.0 for i in range(5)]) ** 2))) < 1e-12       # position 7
    assert A.bounds(dict(l2=1e-7, peak=1e-6, pos=1e-5)) == dict(l2=2e-7, peak=3e-6, pos=TOL)


@pytest.mark.parametrize("route,kind", A.CASES)
def test_reference_figures_stay_under_the_cap(route, kind):
    """the C oracle's own figures on the route's inputs; a second seed agrees"""
    for e, f in A.reference_figures(route, kind).items():
        g = A.reference_figures(route, kind, 1)[e]
        print("%s %s %-20s l2 %.2e peak %.2e pos %.2e   seed 1: %.2e %.2e %.2e" % (route, kind, e, f["l2"], f["peak"], f["pos"], g["l2"], g["peak"], g["pos"]))
        assert 0 < f["l2"] < A.REF_L2_CAP and A.bounds(f)["l2"] < 1e-6
        if route in A.SHORT_BLOCKS:                                  # (40% seen at N = 32: still inside sqrt 2, half the margin)
            assert 2 ** -0.5 < g["l2"] / f["l2"] < 2 ** 0.5
        else:                                                        # (16% seen at N = 279, below 10% elsewhere)
            assert abs(g["l2"] / f["l2"] - 1) < 0.2


def test_two_seeds_agree_to_a_few_percent():
    """over all routes, tap families and entry points the l2 of the second seed is within 5% of the first's in the median, and within
    10% on nine cases out of ten"""
    dev = sorted(abs(A.reference_figures(r, k, 1)[e]["l2"] / f["l2"] - 1) for r, k in A.CASES for e, f in A.reference_figures(r, k).items())
    print("median %.3f, 90th percentile %.3f, largest %.3f of %d" % (dev[len(dev) // 2], dev[9 * len(dev) // 10], dev[-1], len(dev)))
    assert dev[len(dev) // 2] < 0.05 and dev[9 * len(dev) // 10] < 0.10


@pytest.mark.parametrize("route,kind", A.CASES)
def test_second_seed_passes_against_the_first_seeds_bounds(route, kind):
    """no false alarm: the margins do not fire on the scatter of the figures"""
    for e in A.ROUTES[route]["entries"]:
        bound = A.bounds(A.reference_figures(route, kind)[e], A.ROUTES[route]["margin"])
        got = A.reference_figures(route, kind, 1)[e]
        for f in A.FIGURES:
            assert got[f] < bound[f], (e, f, got[f], bound[f])


def _tap_entries(route):
    return [e for e in ("modulate", "fd", "demodulate", "ic_mf") if e in A.ROUTES[route]["entries"]]


@pytest.mark.parametrize("route,kind", A.CASES)
def test_taps_with_18_mantissa_bits_pass_tol_and_exceed_the_budget(route, kind):
    """A tap table stored or split too coarsely: l2 and pos.  The NORMALISED float32 taps are cut, as a kernel's table would be (the RRC
    design values themselves are mostly 1 and 0, which no cut changes); the C oracle's constructor normalises them once more, which takes
    the common scale error of a cut out again and leaves the tap-to-tap part."""
    c = A.make_case(route, kind)
    h = A.oracle_handles(c, taps=A.chop_mantissa(c["nt"], 18))
    moved = rel_err(h.dem.o.filter_taps(), A.oracle_handles(c).dem.o.filter_taps())
    print("%s %s taps moved by %.2e" % (route, kind, moved))
    for e in _tap_entries(route):
        bound = A.bounds(A.reference_figures(route, kind)[e], A.ROUTES[route]["margin"])
        got = h.figures(e, c)[0]
        print("%s %s %-20s l2 %.2e (bound %.2e) pos %.2e (bound %.2e)" % (route, kind, e, got["l2"], bound["l2"], got["pos"], bound["pos"]))
        assert got["l2"] < TOL
        if (route, kind) in A.CUT_STAYS_INSIDE:
            assert got["l2"] < bound["l2"], ("the exception no longer holds", e, got, bound)     # (l2 at 0.7 of its bound; pos within 5% of its own, either side)
        else:
            assert got["l2"] > bound["l2"] and got["pos"] > bound["pos"], (e, got, bound)


@pytest.mark.parametrize("route,kind", A.CASES)
def test_one_wrong_element_passes_tol_and_exceeds_the_budget(route, kind):
    """the last element of the last block off by 1e-4 of the block's RMS: peak.  Its l2 is 1e-4 / sqrt N, inside TOL from N = 101 on."""
    c = A.make_case(route, kind)
    h = A.oracle_handles(c)
    for e in A.ROUTES[route]["entries"]:
        bound = A.bounds(A.reference_figures(route, kind)[e], A.ROUTES[route]["margin"])
        _, got, ref = h.figures(e, c)
        f = A.figures(A.off_one_element(got, ref), ref)
        if c["N"] > 100:
            assert f["l2"] < TOL, (e, f)
        assert f["peak"] > 10 * bound["peak"], (e, f, bound)
        assert f["pos"] > bound["pos"]                          # (seen by pos as well: 1e-4 / sqrt B at that position)


@pytest.mark.parametrize("route,kind", A.CASES)
def test_one_wrong_position_passes_tol_and_exceeds_the_budget(route, kind):
    """One output position off by 1e-6 of the block's RMS in every block (one wrong twiddle literal, one lane on a cheaper path): 1e-6 / sqrt N
    in a block's l2, caught by pos.  An extra error of 1e-6 can only stand out where the reference's own per-position figure is below
    5e-7 (the bound is twice that figure); it is asserted on every entry point where that holds with a little room (4.5e-7), and on every
    route that is at least the plain timeslot transforms (the cancellation rounds on the two routes that have nothing else)."""
    c = A.make_case(route, kind)
    h = A.oracle_handles(c)
    caught = []
    for e in A.ROUTES[route]["entries"]:
        ref_f = A.reference_figures(route, kind)[e]
        bound = A.bounds(ref_f, A.ROUTES[route]["margin"])
        _, got, ref = h.figures(e, c)
        f = A.figures(A.off_one_position(got, ref), ref)
        assert f["l2"] < TOL, (e, f)
        if ref_f["pos"] < 4.5e-7:
            assert f["pos"] > bound["pos"], (e, f, bound)
            caught.append(e)
    assert ("to_td" if "to_td" in A.ROUTES[route]["entries"] else "ic_mf") in caught, caught


@pytest.mark.parametrize("route,kind", A.CASES)
def test_decision_guard_keeps_at_least_half_of_the_blocks(route, kind):
    """a condition, not a measurement: checked with the float64 oracle alone (the GPU test asserts the same count before it compares)"""
    c = A.make_case(route, kind)
    for inp in ("mf", "zf"):
        k = c["keep_ic_" + inp]
        print(route, kind, inp, int(k.sum()), "of", c["B"])
        assert 2 * k.sum() >= c["B"], (inp, int(k.sum()))


@pytest.mark.parametrize("route", sorted(r for r in A.ROUTES if A.ROUTES[r]["entries"] == A.PLAIN + A.IC))
def test_c_oracle_is_exactly_homogeneous_under_powers_of_two(route):
    """Scaling by a power of two commutes with every float32 rounding while nothing over- or underflows: modulate(2^20 x) is
    2^20 modulate(x) bit for bit, and so is every other linear entry point under the per-block scales of the GPU test; x and f_eq scaled
    together leave the equalised calls unchanged."""
    c = A.make_case(route, "rand")
    h = A.oracle_handles(c)
    B = c["B"]
    assert np.array_equal(P.bits(h.run("modulate", c, sx=np.full(B, 2.0 ** 20))), P.bits(A.times(h.run("modulate", c), np.full(B, 2.0 ** 20))))
    s = A.block_scales(B)
    assert set(np.log2(s[:4]).astype(int)) == set(A.SCALES)
    for e in A.PLAIN:
        plain = np.asarray(h.run(e, c)).reshape(B, -1)
        scaled = np.asarray(h.run(e, c, sx=s)).reshape(B, -1)
        assert np.isfinite(scaled).all() and np.array_equal(P.bits(scaled), P.bits(A.times(plain, s))), e
    for e in ("fdeq", "demodulate_equalize"):
        for k in A.JOINT:
            both = np.full(B, 2.0 ** k)
            assert np.array_equal(P.bits(h.run(e, c, sx=both, sf=both)), P.bits(h.run(e, c))), (e, k)


@pytest.mark.parametrize("route", A.TX_ROUTES)
def test_transmitter_oracle_figures(route):
    """COracleTx on the transmitter case: the frames behind the preamble, every port, under the same cap"""
    import c_oracle
    c = A.make_tx_case(route)
    tx = c_oracle.COracleTx(*A.tx_args(c))
    for port in range(len(A.TX_SHIFTS)):
        got = tx.work(c["sym"], port)
        assert np.array_equal(got[:, :A.TX_PRE], np.broadcast_to(c["pre"][port].astype(np.complex64), (c["B"], A.TX_PRE)))
        f = A.figures(got[:, A.TX_PRE:], c["refs"][port][:, A.TX_PRE:])
        print(route, port, f)
        assert 0 < f["l2"] < A.REF_L2_CAP
