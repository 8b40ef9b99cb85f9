"""GPU parity of the IC receiver's decisions beyond QPSK, on every kernel family.

Each family states the decision rule on its own (decide_point in gfdm_rowlane_impl.h for the compiled and the run-time
instantiated row-lane kernels, decide in gfdm_generic.hip, rader_decide in gfdm_rader.hip) and sums the phase offset on its
own.  Here BPSK (sign test and nearest point), pygfdm's point orders, scaled BPSK, 8-PSK, 16- / 64-QAM, a single point and
4096 points run through each of them against the float64 oracle (lib/advanced_receiver_kernel_cc.cc:56-123), with known
answers for exact ties, zero under the sign test and the multiplicity of a subcarrier in the map.

IC outputs are compared on the blocks whose oracle decision margin (gfdm_ref.decision_margin: distance to the nearest
boundary of the decision region, and with phase compensation to arg's branch cut) exceeds DECISION_GUARD; every test
asserts a floor on the number of blocks it compares.
"""
import contextlib

import numpy as np
import pytest

import gfdm_ref as R
from conftest import rel_err
from gfdm_amd.filters import get_frequency_domain_filter
from test_decisions import CONSTELLATIONS, draw, qam_points

pytestmark = pytest.mark.gpu

TOL = 1e-5
DECISION_GUARD = 1e-4

# (M, K, L, alpha, family the IC handle must run on)
FAMILY_SHAPES = [
    (9, 64, 2, 0.2, "rowlane"),             # the block is the wavefront: neighbours by DPP rotates
    (15, 128, 4, 0.2, "rowlane"),           # two wavefronts per block, LDS exchange; QPSK would take the matrix-core rounds
    (5, 32, 2, 0.5, "rowlane"),             # two blocks per wavefront
    (7, 16, 2, 0.3, "rowlane_jit"),         # instantiated at run time (hiprtc)
    (7, 12, 2, 0.3, "generic_lds"),
    (21, 37, 2, 0.35, "generic_lds"),
    (64, 8, 2, 0.3, "generic_lds"),         # timeslot transforms on the matrix cores (M >= 32)
    (127, 16, 2, 0.5, "generic_rader"),     # Rader timeslot transforms
    (15, 1040, 2, 0.3, "generic_lds"),      # block larger than the LDS: tiles in global scratch
]
SHAPE_IDS = ["%d_%d_%d" % s[:3] for s in FAMILY_SHAPES]

# the rule requested at creation: the pygfdm tables ask for the sign tests and must fall back to the nearest-point rule
REQUEST = {"bpsk_pygfdm": "bpsk", "qpsk_pygfdm": "qpsk", "bpsk_x2": "bpsk"}
# points on the real axis: the data turned by half a radian, so that every symbol of the negative point lies below arg's cut
PHASE = {"bpsk_gr": 0.5, "bpsk_pygfdm": 0.5, "bpsk_x2": 0.5}
SMALL = {(5, 32, 2), (7, 16, 2), (7, 12, 2), (127, 16, 2)}      # the shapes the 64-QAM and 4096-point cases run on
# the self-interference of a roll-off above 0.1 puts some of a big block's 8-PSK / QAM symbols within fp32 noise of a decision
# boundary (every block would be dropped): these run at roll-off 0.1
DENSE = {"8psk", "16qam", "16qam_perm", "64qam"}


def margin_keep(stages):
    """blocks whose every decision (every round) and, with phase compensation, every round-0 symbol's arg is clear of fp32 noise"""
    return stages["dec_margin"] > DECISION_GUARD


def family_context(family, M):
    """handles of the generic_lds shapes are created on the generic family (a power-of-two K would otherwise be instantiated at run
    time); from 32 timeslots on with the timeslot transforms on the matrix cores"""
    import gfdm_amd
    if family not in ("generic_lds",):
        return contextlib.nullcontext()           # (the Rader kernels serve M = 127 on their own; forcing the generic family would bypass them)
    stack = contextlib.ExitStack()
    stack.enter_context(gfdm_amd.generic_family_for_testing())
    if M >= 32:
        prev = gfdm_amd.set_dft_matrix_cores(2)
        stack.callback(gfdm_amd.set_dft_matrix_cores, prev)
    return stack


def make_adv(shape, smap, ic_iter, points, pc=0, decision="auto", taps=None):
    import gfdm_amd
    M, K, L, alpha, family = shape
    taps = get_frequency_domain_filter("rrc", alpha, M, K, L) if taps is None else taps
    with family_context(family, M):
        adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, np.asarray(smap), ic_iter, points, do_phase_compensation=pc, decision=decision)
    assert adv.kernel_name() == family, (shape, adv.kernel_name())
    return adv


def partial_map(K):
    return np.arange(K) if K < 8 else np.concatenate((np.arange(1, K // 2 - 1), np.arange(K // 2 + 2, K)))


def signal(shape, name, smap, B, seed):
    """(MF input, ZF input, f_eq): symbols of `name` on the map's subcarriers, modulated, through a frequency-selective channel"""
    M, K, L, alpha, _ = shape
    N = M * K
    rng = np.random.default_rng(seed)
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = draw(rng, name, (B, len(smap), M), PHASE.get(name, 0.0))
    x = R.modulate(d.reshape(B, N), nt, M, K, L)
    feq = np.fft.fft(np.array([1, .5, .1j, .1 + .05j]), N)[None, :] * np.exp(0.01j * np.arange(B))[:, None]
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    return x, xe, feq


def run_cases(shape, name, combos, B, seed):
    """every (map, ic_iter, pc) of `combos`, MF and ZF input, against the oracle on the blocks the margin keeps; returns (kept, compared)"""
    M, K, L, alpha, _ = shape
    pts, kind, _ = CONSTELLATIONS[name]
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    kept = total = 0
    maps = {"full": np.arange(K), "partial": partial_map(K)}
    sig = {m: signal(shape, name, maps[m], B, seed + i) for i, m in enumerate(maps)}
    for mname, ic_iter, pc in combos:
        smap = maps[mname]
        x, xe, feq = sig[mname]
        adv = make_adv(shape, smap, ic_iter, pts, pc, REQUEST.get(name, "auto"))
        assert adv.decision_rule() == kind, (name, adv.decision_rule())
        for inp, eq in ((x, None), (xe, feq)):
            ref, st = R.advanced_receive(inp, nt, M, K, L, smap, pts, ic_iter, f_eq=eq, do_phase_compensation=pc, kind=kind, return_stages=True)
            keep = margin_keep(st)
            got = adv.demodulate(inp) if eq is None else adv.demodulate_equalize(inp, eq)
            assert np.all(np.isfinite(got))
            if keep.any():
                err = rel_err(got[keep], ref[keep])
                assert err < TOL, (name, shape[:3], mname, ic_iter, pc, "zf" if eq is not None else "mf", err)
            kept += int(keep.sum())
            total += B
    return kept, total


ALL_COMBOS = [(m, ic, pc) for m in ("full", "partial") for ic in (1, 2, 5) for pc in (0, 1)]
BASIC = ["bpsk_gr", "bpsk_pygfdm", "qpsk_pygfdm", "bpsk_x2", "8psk", "16qam", "16qam_perm", "single"]


PARITY_CASES = [(s, n) for s in FAMILY_SHAPES for n in BASIC + (["64qam"] if s[:3] in SMALL else [])]


@pytest.mark.parametrize("shape,name", PARITY_CASES, ids=["%d_%d_%d-%s" % (s[:3] + (n,)) for s, n in PARITY_CASES])
def test_constellation_matches_oracle_on_every_family(shape, name):
    """MF and ZF input, 1 / 2 / 5 rounds, phase compensation off and on, full and partial map; the rule the handle reports is
    the one the oracle runs (GNU Radio's BPSK: the sign test; pygfdm's point orders and scaled BPSK: nearest point, also when the
    sign test was asked for)."""
    big = shape[0] * shape[1] > 4000
    combos = ALL_COMBOS if not big else [c for c in ALL_COMBOS if c[1] != 2]
    B = 4 if big else 8
    if name in DENSE:
        shape = shape[:3] + (0.1,) + shape[4:]
    kept, total = run_cases(shape, name, combos, B, seed=97 * shape[0] + shape[1] + len(name))
    assert kept >= total // 5, (kept, total)      # (64-QAM on the M = 127 shape keeps the fewest: 48 of 192)


def test_4096_points_reach_the_end_of_the_list():
    """4092 decoys at distance >= 10 from every symbol and the four true points (QPSK turned by 0.1 rad) at indices 4092..4095: the
    nearest-point loop must run over the API's whole range (1..4096 points) on every family; 4097 points are refused."""
    import gfdm_amd
    pts = CONSTELLATIONS["4096"][0]
    assert pts.size == 4096 and np.min(np.abs(pts[:4092])) > 11.99
    for shape in FAMILY_SHAPES:
        if shape[:3] in SMALL:
            rader = shape[4] == "generic_rader"          # (the float64 nearest-point search over 4096 points is what costs here)
            combos = [("partial", 2, 1)] if rader else [("full", 1, 0), ("partial", 2, 1)]
            kept, total = run_cases(shape, "4096", combos, 3 if rader else 6, seed=shape[1])
            assert kept >= total // 2, (shape, kept, total)
    M, K, L = 9, 64, 2
    taps = get_frequency_domain_filter("rrc", 0.2, M, K, L)
    with pytest.raises(ValueError):
        gfdm_amd.AdvancedReceiver(M, K, L, taps, np.arange(K), 2, np.concatenate((pts, [5j])), decision="nearest")


@pytest.mark.parametrize("shape", FAMILY_SHAPES, ids=SHAPE_IDS)
def test_single_point_decides_that_point(shape):
    """n_points = 1: every decision is that point, so a round is S' = S - ic (.) DFT_M(2 p) on the map's neighbours -- the same in every
    round (known answer, without the oracle's decide)."""
    M, K, L, alpha, _ = shape
    p = CONSTELLATIONS["single"][0]
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    x, _, _ = signal(shape, "16qam", np.arange(K), 3, seed=M)
    S = R.fft_filter_downsample(x, nt, M, K, L)
    want = R.transform_subcarriers_to_td(R.cancel_sc_interference(np.full(x.shape, p[0]), S, R.ic_filter_taps(nt, M, L), M, K), M, K)
    for ic_iter in (1, 3):
        got = make_adv(shape, np.arange(K), ic_iter, p).demodulate(x)
        assert rel_err(got, want) < TOL


def zero_input(N):
    z = np.zeros((2, N), np.complex64)
    z[1] = -0.0 - 0.0j
    return z


def zero_case_taps(shape):
    """RRC taps plus a complex perturbation.  With d0 = 0 every decision is the same point, constant over the timeslots, so a round
    leaves only -ic[0] x (the neighbours' decisions); for a plain RRC prototype ic[0] = t[0] t[(L-1) M] is ~1e-3 and the output a
    residue of larger float32 terms, too small for a relative comparison.  The perturbation makes ic[0] O(0.1)."""
    M, K, L, alpha, _ = shape
    rng = np.random.default_rng(M * L)
    return get_frequency_domain_filter("rrc", alpha, M, K, L) + 0.3 * (rng.standard_normal(M * L) + 1j * rng.standard_normal(M * L))


@pytest.mark.parametrize("shape", FAMILY_SHAPES, ids=SHAPE_IDS)
def test_exact_ties_go_to_the_first_listed_point(shape):
    """All-zero input (and its negative-zero copy): d0 = 0 exactly, and the four inner 16-QAM points are exactly equally distant from it.
    Every decision is the first of them in the list; reordering the list changes the output, and every order equals the oracle."""
    M, K, L, alpha, _ = shape
    taps = zero_case_taps(shape)
    nt = R.normalize_taps(taps, M)
    q = qam_points(16)
    inner = np.flatnonzero(np.abs(q) < 0.5)
    assert inner.size == 4 and np.ptp(np.abs(q[inner])) == 0
    z = zero_input(M * K)
    outer = np.setdiff1d(np.arange(16), inner)
    outs = []
    for first in inner:
        order = np.concatenate((outer[:6], [first], outer[6:], np.setdiff1d(inner, [first])))     # `first` is listed before the other three
        p = q[order]
        ref = R.advanced_receive(z.astype(complex), nt, M, K, L, np.arange(K), p, 1, kind="nearest")
        assert np.allclose(ref, R.advanced_receive(z.astype(complex), nt, M, K, L, np.arange(K), q[first:first + 1], 1))
        assert np.abs(ref).max() > 1e-2
        got = make_adv(shape, np.arange(K), 1, p, decision="nearest", taps=taps).demodulate(z)
        assert rel_err(got, ref) < TOL and np.all(np.isfinite(got))
        outs.append(got[0])
    for i in range(4):
        for j in range(i):
            assert rel_err(outs[i], outs[j]) > 0.5


@pytest.mark.parametrize("shape", FAMILY_SHAPES, ids=SHAPE_IDS)
def test_bpsk_sign_test_sends_zero_to_the_negative_point(shape):
    """GNU Radio's BPSK (sign test): an exactly-zero component (+0 and -0) decides -1, on every family."""
    M, K, L, alpha, _ = shape
    taps = zero_case_taps(shape)
    nt = R.normalize_taps(taps, M)
    b = CONSTELLATIONS["bpsk_gr"][0]
    adv = make_adv(shape, np.arange(K), 1, b, taps=taps)
    assert adv.decision_rule() == "bpsk"
    z = zero_input(M * K)
    ref = R.advanced_receive(z.astype(complex), nt, M, K, L, np.arange(K), b, 1, kind="bpsk")
    assert np.allclose(ref, R.advanced_receive(z.astype(complex), nt, M, K, L, np.arange(K), b[:1], 1))
    assert np.abs(ref).max() > 1e-2
    assert rel_err(adv.demodulate(z), ref) < TOL


@pytest.mark.parametrize("shape", [s for s in FAMILY_SHAPES if s[:3] in {(9, 64, 2), (15, 128, 4), (7, 16, 2), (7, 12, 2), (127, 16, 2)}],
                         ids=lambda s: "%d_%d_%d" % s[:3])
def test_subcarrier_listed_300_times_weighs_300_times_in_the_phase_mean(shape):
    """The duplicate-map known answer (tests/test_parity_gpu.py::test_duplicate_subcarrier_map_entry_counts_twice_in_the_phase_mean) past
    255 copies: phi([k1] * 300 + [k2]) = (300 phi[k1] + phi[k2]) / 301 -- the multiplicity a handle keeps per subcarrier must not saturate."""
    M, K, L, alpha, _ = shape
    rng = np.random.default_rng(7 * M + K)
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    N, B, k1, k2 = M * K, 4, 3, 7
    q = R.qpsk_points()
    d = np.zeros((B, K, M), complex)
    d[:, k1, :] = q[rng.integers(0, 4, (B, M))] * np.exp(-0.02j)
    d[:, k2, :] = q[rng.integers(0, 4, (B, M))] * np.exp(0.08j)
    x = R.modulate(d.reshape(B, N), nt, M, K, L)
    d0 = R.demodulate(x, nt, M, K, L)

    def run(smap, pc):
        return make_adv(shape, smap, 1, q, pc).demodulate(x)

    def phi(smap):
        diff = run(smap, 1).astype(np.complex128) - run(smap, 0)
        return np.angle(1.0 + np.sum(np.conj(d0) * diff, axis=-1) / np.sum(np.abs(d0) ** 2, axis=-1))

    p1, p2 = phi([k1]), phi([k2])
    assert np.min(np.abs(p1 - p2)) > 0.05
    big = [k1] * 300 + [k2]
    assert np.max(np.abs(phi(big) - (300 * p1 + p2) / 301)) < 2e-5
    ref = R.advanced_receive(x, nt, M, K, L, big, q, 1, do_phase_compensation=1, kind="qpsk")
    assert rel_err(run(big, 1), ref) < TOL


def test_setters_after_creation_switch_the_rounds():
    """A QPSK handle at (15, 128, 4) runs its rounds on the matrix cores; set_phase_compensation(1) must take its launches off that form (it has
    no phase sum), set_phase_compensation(0) back onto it, set_ic(n) change the number of rounds -- each against the oracle, and each equal to
    a handle created with that configuration."""
    shape = (15, 128, 4, 0.2, "rowlane")
    M, K, L, alpha, _ = shape
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    q = R.qpsk_points()
    smap = partial_map(K)
    x, xe, feq = signal(shape, "qpsk_pygfdm", smap, 8, seed=15)
    # qpsk_pygfdm has the same points as GNU Radio's QPSK: the data are plain QPSK symbols
    adv = make_adv(shape, smap, 2, q)
    assert adv.decision_rule() == "qpsk"
    kept = 0
    for step, (ic_iter, pc) in enumerate(((2, 0), (2, 1), (2, 0), (5, 0), (5, 1), (1, 1))):
        if step:
            if pc != adv.get_phase_compensation():
                adv.set_phase_compensation(pc)
            if ic_iter != adv.get_ic():
                adv.set_ic(ic_iter)
        assert (adv.get_ic(), adv.get_phase_compensation()) == (ic_iter, pc)
        fresh = make_adv(shape, smap, ic_iter, q, pc)
        ref, st = R.advanced_receive(xe, nt, M, K, L, smap, q, ic_iter, f_eq=feq, do_phase_compensation=pc, kind="qpsk", return_stages=True)
        keep = margin_keep(st)
        got = adv.demodulate_equalize(xe, feq)
        assert np.array_equal(got, fresh.demodulate_equalize(xe, feq))
        if keep.any():
            assert rel_err(got[keep], ref[keep]) < TOL, (ic_iter, pc)
        kept += int(keep.sum())
    assert kept >= 3 * 8


@pytest.mark.parametrize("shape", [FAMILY_SHAPES[0], FAMILY_SHAPES[4]], ids=lambda s: "%d_%d_%d" % s[:3])
def test_16qam_frames_in_demapped_symbols_out(shape):
    """demodulate_frames after configure_frames (load offset + demapping store) with 16-QAM decisions"""
    M, K, L, alpha, _ = shape
    N, B = M * K, 8
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    pts = CONSTELLATIONS["16qam"][0]
    smap = partial_map(K)
    _, xe, feq = signal(shape, "16qam", smap, B, seed=3 * K)
    rng = np.random.default_rng(K)
    kept = 0
    for pc in (0, 1):
        adv = make_adv(shape, smap, 2, pts, pc)
        ref, st = R.advanced_receive(xe, nt, M, K, L, smap, pts, 2, f_eq=feq, do_phase_compensation=pc, kind="nearest", return_stages=True)
        keep = margin_keep(st)
        for per_timeslot in (True, False):
            adv.configure_frames(N + 11, 6, smap, per_timeslot)
            frames = rng.standard_normal((B, N + 11)) + 1j * rng.standard_normal((B, N + 11))
            frames[:, 6:6 + N] = xe
            got = adv.demodulate_frames(frames, feq)
            want = R.demap_from_resources(ref, M, K, smap, per_timeslot)
            assert got.shape == want.shape
            if keep.any():
                assert rel_err(got[keep], want[keep]) < TOL
        kept += int(keep.sum())
    assert kept >= B


def test_16qam_device_pointer_entry_point():
    """gfdm_hip_advanced_receiver_work_device (torch tensors on the GPU) with 16-QAM decisions, equal to the host entry point"""
    import torch
    shape = FAMILY_SHAPES[0]
    M, K, L, alpha, _ = shape
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", alpha, M, K, L), M)
    pts = CONSTELLATIONS["16qam"][0]
    smap = partial_map(K)
    _, xe, feq = signal(shape, "16qam", smap, 12, seed=64)
    dev = torch.device("cuda:0")
    for pc in (0, 1):
        adv = make_adv(shape, smap, 3, pts, pc)
        ref, st = R.advanced_receive(xe, nt, M, K, L, smap, pts, 3, f_eq=feq, do_phase_compensation=pc, kind="nearest", return_stages=True)
        keep = margin_keep(st)
        assert keep.sum() >= 4
        t_x = torch.from_numpy(xe.astype(np.complex64)).to(dev)
        t_e = torch.from_numpy(feq.astype(np.complex64)).to(dev)
        got = adv.demodulate_equalize(t_x, t_e)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert rel_err(got[keep], ref[keep]) < TOL
        assert np.array_equal(got, adv.demodulate_equalize(xe, feq))


def test_16qam_through_the_pybind11_advanced_receiver():
    """gfdm_python.AdvancedReceiver with gfdm_python.Constellation(points): the reference's constructor surface with a 16-QAM object"""
    import gfdm_python
    M, K, L, alpha = 9, 64, 2, 0.2
    shape = (M, K, L, alpha, "rowlane")
    taps = get_frequency_domain_filter("rrc", alpha, M, K, L)
    nt = R.normalize_taps(taps, M)
    pts = CONSTELLATIONS["16qam_perm"][0]
    smap = partial_map(K)
    x, xe, feq = signal(shape, "16qam_perm", smap, 8, seed=9)
    c = gfdm_python.Constellation(list(pts.astype(np.complex64)))
    kept = 0
    for pc in (0, 1):
        adv = gfdm_python.AdvancedReceiver(M, K, L, list(taps.astype(np.complex64)), list(smap), 2, c, pc)
        assert adv.kernel_name() == "rowlane"
        ref, st = R.advanced_receive(xe, nt, M, K, L, smap, pts, 2, f_eq=feq, do_phase_compensation=pc, kind="nearest", return_stages=True)
        keep = margin_keep(st)
        got = np.stack([adv.demodulate_equalize(xe[b].astype(np.complex64), feq[b].astype(np.complex64)) for b in range(8)])
        if keep.any():
            assert rel_err(got[keep], ref[keep]) < TOL
        kept += int(keep.sum())
    assert kept >= 8
