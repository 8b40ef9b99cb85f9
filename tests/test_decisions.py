"""Decision rules of the IC receiver beyond QPSK, on the CPU: the oracle's decision margin, the three host-side
statements of the rule (gfdm_ref.decide, the C oracle's decide, gr::gfdm::constellation::decision_maker), and the C
oracle's IC receiver against the float64 one for constellations other than QPSK.

The constellations here are shared with tests/test_constellations_gpu.py.  The reference decides with whatever
gr::digital::constellation it is given (lib/advanced_receiver_kernel_cc.cc:109-123); pygfdm lists its BPSK / QPSK points
in another order than GNU Radio (python/pygfdm/symbolmapping.py:20-21), so those tables take the nearest-point rule.
"""
import numpy as np
import pytest

import c_oracle
import gfdm_ref as R
from conftest import rel_err
from gfdm_amd.filters import get_frequency_domain_filter

TOL_F32 = 1e-5
DECISION_GUARD = 1e-4


def qam_points(n):
    """square n-QAM, unit average power, row by row from the most negative corner"""
    side = int(round(np.sqrt(n)))
    lv = np.arange(-(side - 1), side, 2, dtype=np.float64)
    p = (lv[None, :] + 1j * lv[:, None]).ravel()
    return p / np.sqrt(np.mean(np.abs(p) ** 2))


def decoy_points(n, radius=12.0):
    """n points on rings of radius >= `radius`: at distance >= radius - |x| from any sample x near the unit circle"""
    i = np.arange(n)
    return (radius + 0.5 * (i // 64)) * np.exp(2j * np.pi * ((i % 64) + 0.5 * (i // 64 % 2)) / 64)


_S = np.sqrt(0.5)
_ROTQ = R.qpsk_points() * np.exp(0.1j)

# name -> (points, the rule the handle reports and the oracle runs, points the data are drawn from)
CONSTELLATIONS = {
    "bpsk_gr": (np.array([-1, 1], complex), "bpsk", None),                          # gr::digital::constellation_bpsk: sign test
    "bpsk_pygfdm": (np.array([1, -1], complex), "nearest", None),                   # pygfdm's table: same points, other order
    "qpsk_pygfdm": (np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]) * _S, "nearest", None),
    "bpsk_x2": (np.array([-2, 2], complex), "nearest", None),
    "8psk": (np.exp(1j * np.pi * np.arange(8) / 4), "nearest", None),              # point 4 lies on arg's branch cut
    "16qam": (qam_points(16), "nearest", None),
    "16qam_perm": (qam_points(16)[np.random.default_rng(16).permutation(16)], "nearest", None),
    "64qam": (qam_points(64), "nearest", None),
    "single": (np.array([0.6 - 0.8j]), "nearest", np.array([0.6 - 0.8j, -0.8 - 0.6j])),   # n_points = 1: every decision is that point
    "4096": (np.concatenate((decoy_points(4092), _ROTQ)), "nearest", _ROTQ),      # the true points at indices 4092..4095
}


def data_points(name):
    pts, _, data = CONSTELLATIONS[name]
    return pts if data is None else data


def draw(rng, name, shape, phase=0.0):
    """uniform symbols of a constellation (its data points), turned by a common phase"""
    p = data_points(name)
    return p[rng.integers(0, p.size, shape)] * np.exp(1j * phase)


def _samples(rng, pts, n):
    """points plus complex noise of about the point spacing, and a few far outliers"""
    spread = 0.5 * np.min([np.abs(a - b) for i, a in enumerate(pts) for b in pts[i + 1:]] or [1.0])
    x = pts[rng.integers(0, pts.size, n)] + spread * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x[:8] *= 5
    return x


def _cases():
    out = [(name, pts, kind) for name, (pts, kind, _) in CONSTELLATIONS.items()]
    return out + [("qpsk_gr", R.qpsk_points(), "qpsk"), ("qpsk_gr_nearest", R.qpsk_points(), "nearest"),
                  ("bpsk_gr_nearest", np.array([-1, 1], complex), "nearest")]


@pytest.mark.parametrize("name,pts,kind", _cases(), ids=[c[0] for c in _cases()])
def test_decision_margin_bounds_the_decision_region(name, pts, kind):
    """A sample moved by less than its margin, in any direction, keeps its decision; moved just past the nearest boundary
    (the bisector towards the point that sets the margin, or the axis of the sign test) it takes another one."""
    rng = np.random.default_rng(len(pts) + len(kind))
    x = _samples(rng, pts, 4000)
    m = R.decision_margin(x, pts, kind)
    dec = R.decide(x, pts, kind)
    assert m.shape == x.shape and np.all(m >= 0)
    if pts.size == 1 and kind == "nearest":
        assert np.all(np.isinf(m)) and np.all(dec == pts[0])
        return
    assert np.all(np.isfinite(m))
    for _ in range(4):
        u = np.exp(2j * np.pi * rng.random(x.size))
        assert np.array_equal(R.decide(x + 0.999 * m * u, pts, kind), dec)
    if kind == "qpsk":
        re = np.abs(x.real) <= np.abs(x.imag)
        step = np.where(re, -np.sign(x.real), -1j * np.sign(x.imag))
    elif kind == "bpsk":
        step = -np.sign(x.real).astype(complex)
    else:
        i = np.argmin(np.abs(x[:, None] - pts) ** 2, axis=-1)
        d = np.abs(x[:, None] - pts) ** 2
        sep = np.abs(pts[None, :] - pts[i][:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.where(sep > 0, (d - d[np.arange(x.size), i][:, None]) / (2 * sep), np.inf)
        j = np.argmin(b, axis=-1)
        assert np.allclose(b[np.arange(x.size), j], m)
        step = (pts[j] - pts[i]) / np.abs(pts[j] - pts[i])        # the normal of the bisector, towards p_j
    moved = R.decide(x + (m + 1e-7) * step, pts, kind)
    assert np.all(moved != dec)


def test_decision_margin_known_values():
    q = R.qpsk_points()
    assert np.allclose(R.decision_margin(np.array([0.3 - 0.1j, -2 + 5j]), q, "qpsk"), [0.1, 2])
    assert np.allclose(R.decision_margin(np.array([-0.25 + 7j]), q, "bpsk"), [0.25])
    qam = np.array([-3, -1, 1, 3], complex)
    # 0.4 is nearest to 1 (index 2): bisector with -1 at 0 -> 0.4, with 3 at 2 -> 1.6
    assert np.allclose(R.decision_margin(np.array([0.4, 2.0, 0.0]), qam, "nearest"), [0.4, 0.0, 0.0])
    assert np.allclose(R.decision_margin(np.array([0.3 + 0.5j]), qam, "nearest"), [0.3])
    assert np.array_equal(R.phase_cut_margin(np.array([-1 + 0.2j, -1 - 0.3j, 1 + 0j, 0j, -0.0 + 0j])), [0.2, 0.3, np.inf, np.inf, np.inf])


def test_dec_margin_stage_is_the_minimum_over_rounds_and_the_branch_cut():
    """advanced_receive(return_stages=True)['dec_margin']: per block, the smallest margin of any decided component in any
    round, and with phase compensation also of the round-0 symbols from arg's cut."""
    M, K, L = 5, 16, 2
    rng = np.random.default_rng(3)
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", 0.4, M, K, L), M)
    smap = np.arange(2, K - 3)
    pts = CONSTELLATIONS["8psk"][0]
    d = np.zeros((6, K, M), complex)
    d[:, smap, :] = draw(rng, "8psk", (6, smap.size, M))
    x = R.modulate(d.reshape(6, -1), nt, M, K, L)
    for pc in (0, 1):
        _, st = R.advanced_receive(x, nt, M, K, L, smap, pts, 3, do_phase_compensation=pc, return_stages=True)
        act = lambda v: v.reshape(6, K, M)[:, smap, :].reshape(6, -1)
        want = np.full(6, np.inf)
        for v in [st["d0"]] + st["iters"][:-1]:
            want = np.minimum(want, R.decision_margin(act(v), pts).min(axis=1))
        if pc:
            want = np.minimum(want, R.phase_cut_margin(act(st["d0"])).min(axis=1))
        assert st["dec_margin"].shape == (6,) and np.array_equal(st["dec_margin"], want)
    _, st = R.advanced_receive(x, nt, M, K, L, smap, pts, 0, return_stages=True)
    assert np.all(np.isinf(st["dec_margin"]))


def _cpp_decide(pts, xs):
    import gfdm_python
    c = gfdm_python.Constellation(list(np.asarray(pts, np.complex64)))
    return np.array([c.decision_maker(complex(v)) for v in np.asarray(xs, np.complex64)])


def _index(x, pts, kind):
    return np.array([int(np.flatnonzero(pts == v)[0]) for v in R.decide(x, pts, kind)])


@pytest.mark.parametrize("name", [n for n in CONSTELLATIONS if CONSTELLATIONS[n][1] == "nearest"])
def test_nearest_point_rules_agree_on_random_samples(name):
    """gfdm_ref.decide, the C oracle's decide (through its IC receiver) and constellation::decision_maker (the rule a
    points-only constellation runs on the host) pick the same points wherever the float32 distances cannot tie."""
    pts = CONSTELLATIONS[name][0]
    rng = np.random.default_rng(11)
    x = _samples(rng, data_points(name), 600).astype(np.complex64).astype(complex)
    far = R.decision_margin(x, pts) > 1e-5
    assert far.sum() > 500
    assert np.array_equal(_cpp_decide(pts, x[far]), _index(x[far], pts, "nearest"))
    # the C oracle decides on its own demodulated symbols: its IC output equals the float64 one on blocks without near-ties
    M, K, L = 5, 16, 2
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", 0.4, M, K, L), M)
    frame = R.modulate(draw(rng, name, (8, M * K)), nt, M, K, L)
    ref, st = R.advanced_receive(frame, nt, M, K, L, np.arange(K), pts, 1, kind="nearest", return_stages=True)
    keep = st["dec_margin"] > DECISION_GUARD
    assert keep.sum() >= 4
    got = c_oracle.COracle(M, K, L, nt).advanced_receive(frame, np.arange(K), pts, 1, kind="nearest")
    assert rel_err(got[keep], ref[keep]) < TOL_F32


def test_exact_ties_go_to_the_first_minimum():
    """Exact ties (integer points: every distance exact in float32): gfdm_ref.decide, constellation::decision_maker and the C
    oracle take the first of the equally distant points, and reordering the points changes the answer accordingly."""
    q16 = (np.arange(-3, 4, 2)[None, :] + 1j * np.arange(-3, 4, 2)[:, None]).ravel()
    cases = [(q16, 0j, [5, 6, 9, 10]), (q16, 2 + 1j, [10, 11]), (q16, -2 - 2j, [0, 1, 4, 5]),
             (np.array([1, -1], complex), 0j, [0, 1]), (np.array([1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j]), 0j, [0, 1, 2, 3])]
    rng = np.random.default_rng(2)
    for pts, x, tied in cases:
        for _ in range(4):
            order = rng.permutation(pts.size)
            p = pts[order]
            first = int(np.min([np.flatnonzero(order == t)[0] for t in tied]))
            assert _index(np.array([x]), p, "nearest")[0] == first
            assert _cpp_decide(p, [x])[0] == first
            assert R.decision_margin(np.array([x]), p)[0] == 0
    # the C oracle on an all-zero frame: d0 = 0 exactly, the four inner 16-QAM points tie, the first listed one is decided everywhere
    M, K, L = 5, 16, 2
    nt = R.normalize_taps(get_frequency_domain_filter("rrc", 0.4, M, K, L), M)
    co = c_oracle.COracle(M, K, L, nt)
    zero = np.zeros((2, M * K), complex)
    zero[1] = -0.0 - 0.0j
    outs = []
    for order in (np.arange(16), np.arange(16)[::-1], rng.permutation(16)):
        p = q16[order]
        ref = R.advanced_receive(zero, nt, M, K, L, np.arange(K), p, 1, kind="nearest")
        got = co.advanced_receive(zero, np.arange(K), p, 1, kind="nearest")
        assert rel_err(got, ref) < TOL_F32
        outs.append(ref[0])
    assert rel_err(outs[0], outs[1]) > 0.5                    # another first inner point: another answer
    # the BPSK sign test: zero goes to the negative point (index 0 of GNU Radio's table)
    b = np.array([-1, 1], complex)
    ref = R.advanced_receive(zero, nt, M, K, L, np.arange(K), b, 1, kind="bpsk")
    assert rel_err(co.advanced_receive(zero, np.arange(K), b, 1, kind="bpsk"), ref) < TOL_F32
    assert rel_err(ref, R.advanced_receive(zero, nt, M, K, L, np.arange(K), b[:1], 1)) < 1e-12


@pytest.mark.parametrize("name", ["16qam", "8psk", "bpsk_gr"])
@pytest.mark.parametrize("pc", [0, 1])
def test_c_oracle_ic_receiver_matches_numpy_oracle_beyond_qpsk(name, pc):
    """The plain-C oracle's IC receiver against the float64 one: 16-QAM, 8-PSK (a point on arg's cut) and BPSK (sign test),
    partial map, ZF input, phase compensation on and off, blocks whose decisions (and, with phase compensation, arg's cut)
    are clear of float32 noise."""
    M, K, L = 9, 16, 2
    rng = np.random.default_rng(len(name) + 10 * pc)
    taps = get_frequency_domain_filter("rrc", 0.3, M, K, L)
    nt = R.normalize_taps(taps, M)
    pts, kind, _ = CONSTELLATIONS[name]
    B, N = 12, M * K
    smap = np.concatenate((np.arange(1, 7), np.arange(9, K)))
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = draw(rng, name, (B, smap.size, M), phase=0.5 if kind == "bpsk" else 0.0)
    x = R.modulate(d.reshape(B, N), nt, M, K, L)
    feq = np.fft.fft(np.array([1, .4 - .2j, .1j]), N)[None, :] * np.exp(0.03j * np.arange(B))[:, None]
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    co = c_oracle.COracle(M, K, L, taps)
    kept = 0
    for ic_iter in (1, 3):
        ref, st = R.advanced_receive(xe, nt, M, K, L, smap, pts, ic_iter, f_eq=feq, do_phase_compensation=pc, kind=kind, return_stages=True)
        keep = st["dec_margin"] > DECISION_GUARD
        kept += int(keep.sum())
        got = co.advanced_receive(xe, smap, pts, ic_iter, f_eq=feq, do_phase_compensation=pc, kind=kind)
        if keep.any():
            assert rel_err(got[keep], ref[keep]) < TOL_F32
    assert kept >= B
