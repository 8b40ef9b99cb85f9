"""CPU-side checks of the fading model (contract in include/gfdm_hip.h, gfdm_hip_fading_model): the entry points are exported and bound,
the argument table answers without a device, create refuses what it can before any device is touched and there is no CPU fallback,
Python-side argument errors come before any device, the table helpers give their known answers and equal the restatement of
tests/fading_model_ref.py value by value, the restated model has Clarke's autocorrelation, a float32 emulation of the kernel's
run-of-eight scheme stays inside the error budget (the bound itself, apart from the kernel), the restatement's integer phases equal
Python's big integers, and the preconditions of the GPU tests hold on the restatements alone."""
import os

import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import fading_model_ref as Fd
import grid_bound_cases as G
import resampler_cases as RC
from conftest import ROOT, have_gpu

PLAIN = ("create", "destroy", "n_paths", "n_sinusoids", "n_taps", "taps", "amplitudes", "frequencies", "phases", "check")


def test_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.capi.exported_symbols())
    for kind in ("host", "device", "sc16_host", "sc16_device"):
        assert "gfdm_hip_fading_model_apply_%s" % kind in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_fading_model_apply_%s" % kind)
    for name in PLAIN:
        assert "gfdm_hip_fading_model_" + name in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_fading_model_" + name)
    assert not any(n.startswith("gfdm_hip_fading_model_set_") for n in names)           # there are no setters
    assert gfdm_amd.FadingModel is gfdm_amd.capi.FadingModel
    assert gfdm_amd.fading_taps is gfdm_amd.capi.fading_taps and gfdm_amd.fading_sinusoids is gfdm_amd.capi.fading_sinusoids


NAN, INF = float("nan"), float("inf")
# (n_paths, n_sinusoids, n_taps, n, history, offset, gain) -> what the message names; None = accepted
TABLE = [
    ((1, 1, 1, 0, 0, 0, 1.0), None),
    ((8, 17, 64, 1 << 40, 63, 1 << 61, -3.5), None),
    ((2, 3, 3, 1, 0, (1 << 62) - 1, 0.0), None),                      # offset + n == 2^62
    ((2, 3, 3, 1 << 59, (1 << 60) - (1 << 59) - 1, 0, 1.0), None),   # 8 (history + n) just fits
    ((0, 3, 3, 1, 0, 0, 1.0), "n_paths"),
    ((9, 3, 3, 1, 0, 0, 1.0), "n_paths"),
    ((-1, 3, 3, 1, 0, 0, 1.0), "n_paths"),
    ((2, 0, 3, 1, 0, 0, 1.0), "n_sinusoids"),
    ((2, 18, 3, 1, 0, 0, 1.0), "n_sinusoids"),
    ((2, 3, 0, 1, 0, 0, 1.0), "n_taps"),
    ((2, 3, 65, 1, 0, 0, 1.0), "n_taps"),
    ((2, 3, 3, 1, 0, 0, NAN), "gain"),
    ((2, 3, 3, 1, 0, 0, -INF), "gain"),
    ((2, 3, 3, -1, 0, 0, 1.0), "n must"),
    ((2, 3, 3, 1, -1, 0, 1.0), "history"),
    ((2, 3, 3, 1, 0, -1, 1.0), "offset must"),
    ((2, 3, 3, 2, 0, (1 << 62) - 1, 1.0), "2^62"),
    ((2, 3, 3, 1, 0, 1 << 62, 1.0), "2^62"),
    ((2, 3, 3, (1 << 62) + 1, 0, 0, 1.0), "2^62"),
    ((2, 3, 3, 1 << 60, 0, 0, 1.0), "overflow"),                      # 8 n
    ((2, 3, 3, 1, 1 << 60, 0, 1.0), "overflow"),                      # 8 (history + n)
    ((2, 3, 3, 1 << 59, (1 << 60) - (1 << 59), 0, 1.0), "overflow"),
]


@pytest.mark.parametrize("args,match", TABLE)
def test_argument_table(args, match):
    import gfdm_amd
    L = gfdm_amd.lib()
    rc = L.gfdm_hip_fading_model_check(*args)
    if match is None:
        assert rc == gfdm_amd.capi.OK
    else:
        assert rc == gfdm_amd.capi.EINVAL
        assert match in L.gfdm_hip_last_error().decode()


def test_create_refuses_before_any_device_and_there_is_no_cpu_fallback():
    """what create can refuse without a device it refuses first (here, without a GPU, every one of these would otherwise answer ENODEV);
    with good tables: ENODEV without a device, the getters bit for bit with one"""
    import ctypes
    import gfdm_amd
    c, A, F, ph = Fd.tables_for((2, 3, 3))
    make = gfdm_amd.FadingModel.from_tables
    bad_c, bad_A = c.copy(), A.copy()
    bad_c[1, 2], bad_A[0, 1] = NAN, -INF
    for args, match in (((np.ones((9, 2)), np.ones((9, 1)), np.zeros((9, 1), np.int64), np.zeros((9, 1), np.uint64)), "n_paths"),
                        ((np.ones((1, 2)), np.ones((1, 18)), np.zeros((1, 18), np.int64), np.zeros((1, 18), np.uint64)), "n_sinusoids"),
                        ((np.ones((1, 65)), np.ones((1, 1)), np.zeros((1, 1), np.int64), np.zeros((1, 1), np.uint64)), "n_taps"),
                        ((np.ones((1, 0)), np.ones((1, 1)), np.zeros((1, 1), np.int64), np.zeros((1, 1), np.uint64)), "n_taps"),
                        ((bad_c, A, F, ph), "c must be finite"), ((c, bad_A, F, ph), "A must be finite"),
                        ((c, A[:1], F[:1], ph[:1]), "shapes"), ((c, A, F[:, :2], ph), "shapes"), ((c[0], A, F, ph), "shapes")):
        with pytest.raises(ValueError, match=match):
            make(*args)
    with pytest.raises(TypeError, match="integers"):
        make(c, A, F.astype(np.float64), ph)
    L = gfdm_amd.lib()
    h = ctypes.c_void_p()
    assert L.gfdm_hip_fading_model_create(ctypes.byref(h), c.ctypes.data, None, F.ctypes.data, ph.ctypes.data, 2, 3, 3, 0) == gfdm_amd.capi.EINVAL
    assert b"NULL table" in L.gfdm_hip_last_error() and not h.value
    # the constructor in GNU Radio's argument order: the helpers refuse first
    for kw, match in ((dict(N=17, LOS=True), "17 sinusoids"), (dict(N=0), "N"), (dict(fDTs=0.6), "fDTs"), (dict(fDTs=NAN), "fDTs"), (dict(LOS=True, K=-1.0), "k_factor"),
                      (dict(delays=(0.0, 2.5), mags=(1.0, 0.3), ntaps=2), "delays"), (dict(delays=(0.0,), mags=(1.0, 0.3)), "one length"),
                      (dict(delays=np.zeros(9), mags=np.ones(9)), "n_paths"), (dict(ntaps=65), "ntaps")):
        with pytest.raises(ValueError, match=match):
            gfdm_amd.FadingModel(**kw)
    if have_gpu():
        fm = make(c, A, F, ph)
        assert (fm.n_paths(), fm.n_sinusoids(), fm.n_taps()) == (2, 3, 3)
        for got, want in ((fm.taps(), c), (fm.amplitudes(), A), (fm.frequencies(), F), (fm.phases(), ph)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        fm = gfdm_amd.FadingModel(8, 0.01, True, 4.0, 7, (0.0, 1.5), (1.0, 0.3), 8)
        assert (fm.n_paths(), fm.n_sinusoids(), fm.n_taps()) == (2, 9, 8)
        assert np.array_equal(fm.taps(), Fd.taps((0.0, 1.5), (1.0, 0.3), 8)) and np.array_equal(fm.frequencies(), Fd.sinusoids(2, 8, 0.01, 7, True, 4.0)[1])
    else:
        with pytest.raises(gfdm_amd.GfdmHipError, match="no HIP device") as e:
            make(c, A, F, ph)
        assert e.value.status == gfdm_amd.capi.ENODEV


def test_python_argument_errors_come_before_any_device():
    import torch
    import gfdm_amd
    fm = object.__new__(gfdm_amd.FadingModel)              # no handle: whatever these calls raise, they raise before the library is asked
    x = np.zeros(10, np.complex64)
    for dt in (np.int16, np.int32, np.uint8, bool):
        with pytest.raises(TypeError, match="x must be complex samples"):
            fm.apply(np.zeros(10, dt))
    with pytest.raises(TypeError, match="x must be a contiguous complex64"):
        fm.apply(torch.zeros(10, dtype=torch.complex64))                        # a tensor off the device
    with pytest.raises(ValueError, match="int16 out"):
        fm.apply(x, gain=2.0)
    with pytest.raises(TypeError, match="int16"):
        fm.apply(x, sc16=True, out=np.zeros(10, np.complex64))
    with pytest.raises(TypeError, match="complex64"):
        fm.apply(x, sc16=False, out=np.zeros((10, 2), np.int16))
    with pytest.raises(ValueError, match="odd"):
        fm.apply(x, out=np.zeros(21, np.int16))                                  # an int16 out selects sc16
    with pytest.raises(ValueError, match="shape"):
        fm.apply(x, out=np.zeros((10, 3), np.int16))
    with pytest.raises(TypeError, match="contiguous"):
        fm.apply(x, out=np.zeros((10, 4), np.int16)[:, :2])
    with pytest.raises(TypeError, match="numpy array, as x is"):
        fm.apply(x, out=torch.zeros(10, dtype=torch.complex64))
    for history in (-1, 11):
        with pytest.raises(ValueError, match="history"):
            fm.apply(x, history=history)
    with pytest.raises(RuntimeError, match="out holds 10 samples, expected 7"):
        fm.apply(x, history=3, out=np.zeros(10, np.complex64))


# ---- the helpers ----
def test_helper_known_answers():
    import gfdm_amd
    # the hash: splitmix64's published first outputs for seed 0 are mix(1 G), mix(2 G), mix(3 G) with G the golden-ratio increment
    assert [Fd.mix((i * Fd.GOLDEN) & Fd.U64) for i in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert Fd.hash64(0, 0, 0, 0) == Fd.mix(Fd.mix(0) + Fd.GOLDEN) == Fd.mix(Fd.GOLDEN) == 0xE220A8397B1DCDAF
    # fDTs = 0: every F is 0
    for los in (False, True):
        A, F, ph = gfdm_amd.fading_sinusoids(3, 8, 0.0, 11, los, 2.5)
        assert A.dtype == np.float32 and F.dtype == np.int64 and ph.dtype == np.uint64 and A.shape == F.shape == ph.shape == (3, 8 + los)
        assert not F.any()
    # the amplitudes square-sum to 1 per path, with and without LOS
    for N, los, k in ((4, False, 0.0), (8, True, 4.0), (16, True, 0.0), (16, True, 100.0), (1, False, 0.0)):
        A, F, ph = gfdm_amd.fading_sinusoids(4, N, 0.01, 3, los, k)
        assert np.allclose(np.sum(A.astype(np.float64) ** 2, axis=1), 1.0, rtol=0, atol=(N + 1) * 2.0 ** -24)
        assert np.all(np.abs(F) <= round(0.01 * 2 ** 64)) and F.any()
        if los:
            assert A[0, N] == np.float32(np.sqrt(k / (k + 1))) and not A[1:, N].any() and not F[1:, N].any() and not ph[1:, N].any()
    # the stratum of sinusoid s is [s, s + 1) / N of the circle: F = rint(fd cos(alpha) 2^64) with alpha inside it
    A, F, ph = gfdm_amd.fading_sinusoids(2, 8, 0.25, 5)
    alpha = np.arccos(np.clip(F.astype(np.float64) / (0.25 * 2.0 ** 64), -1, 1))                 # in [0, pi]: alpha or 2 pi - alpha
    for s in range(8):
        lo, hi = 2 * np.pi * s / 8, 2 * np.pi * (s + 1) / 8
        assert np.all(((alpha[:, s] >= lo - 1e-9) & (alpha[:, s] <= hi + 1e-9)) | ((2 * np.pi - alpha[:, s] >= lo - 1e-9) & (2 * np.pi - alpha[:, s] <= hi + 1e-9)))
    # integer delays: a one-hot row times mags
    c = gfdm_amd.fading_taps((0, 3, 7), (1.0, -0.5, 0.25), 8)
    want = np.zeros((3, 8), np.float32)
    want[0, 0], want[1, 3], want[2, 7] = 1.0, -0.5, 0.25
    assert c.dtype == np.float32 and np.array_equal(c, want)
    half = gfdm_amd.fading_taps((1.5,), (1.0,), 4)[0].astype(np.float64)
    assert np.allclose(half, [-2 / (3 * np.pi), 2 / np.pi, 2 / np.pi, -2 / (3 * np.pi)], rtol=1e-7)


def test_helpers_equal_the_restatement():
    """gfdm_amd.fading_sinusoids / fading_taps against tests/fading_model_ref.py's own splitmix64 and formulas: equal, value by value"""
    import gfdm_amd
    for P, N, fd, seed, los, k in ((1, 1, 0.5, 0, False, 0.0), (8, 16, 0.01, 12345, True, 4.0), (3, 8, -0.05, 2 ** 64 - 1, True, 0.5), (2, 17, 1e-5, -7, False, 0.0)):
        got, want = gfdm_amd.fading_sinusoids(P, N, fd, seed, los, k), Fd.sinusoids(P, N, fd, seed, los, k)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    for delays, mags, T in (((0.0,), (1.0,), 1), ((0.0, 1.5), (1.0, 0.3), 8), ((0.25, 2.0, 63.0), (1.0, -0.7, 0.1), 64)):
        assert np.array_equal(gfdm_amd.fading_taps(delays, mags, T), Fd.taps(delays, mags, T))


@pytest.mark.parametrize("N", [4, 8, 16])
def test_statistics_of_the_model(N):
    """fDTs = 0.01, 512 seeds times 8 paths = 4096 realisations, a0 = 12345: the mean of conj(g(a0)) g(a0 + tau) is within 5 / sqrt(4096) =
    0.078 of J0(2 pi fDTs tau) for tau in 0, 5, 10, 20, 38, 50, 80, 120.  |g|^2 has mean 1 and E|g|^4 <= 2, so 0.078 is above four standard
    deviations of the mean.  (Measured while writing the issue: worst deviation 0.014 / 0.027 / 0.026 for N = 4 / 8 / 16.)"""
    fd, a0 = 0.01, 12345
    taus = (0, 5, 10, 20, 38, 50, 80, 120)
    acc = np.zeros(len(taus), np.complex128)
    power = 0.0
    for seed in range(512):
        A, F, ph = Fd.sinusoids(8, N, fd, seed)
        g = Fd.gains_at(A, F, ph, a0 + np.array(taus, np.uint64))                 # (8 paths, the lags); tau = 0 is g(a0) itself
        acc += np.sum(np.conj(g[:, :1]) * g, axis=0)
        power += float(np.sum(np.abs(g[:, 0]) ** 2))
    acc /= 4096
    want = np.array([Fd.j0(2 * np.pi * fd * tau) for tau in taus])
    dev = np.abs(acc - want)
    print("N %d: mean |g|^2 %.4f, worst deviation from J0 %.4f (at tau %d)" % (N, power / 4096, dev.max(), taus[int(dev.argmax())]))
    assert abs(want[0] - 1.0) < 1e-12 and abs(Fd.j0(2.404825557695773)) < 1e-12           # the helper's J0: J0(0) = 1, its first zero
    assert np.all(dev <= 5 / np.sqrt(4096))


# ---- the restatement ----
def test_exact_arithmetic_preconditions():
    """the restatement's phases at offset = 2^40 + 1 and at 2^62 - n equal a Python big-integer evaluation, for frequencies anywhere in
    the 64 bits; and the phase is a pure function of the index: any cut gives the same gains"""
    rng = np.random.default_rng(9)
    n = 4097
    Fs = [int(v) for v in rng.integers(-2 ** 63, 2 ** 63 - 1, 6, dtype=np.int64, endpoint=True)] + [0, 1, -1, 2 ** 63 - 1, -2 ** 63, round(0.05 * 2 ** 64)]
    Ps = [int(v) for v in rng.integers(0, 2 ** 64 - 1, len(Fs), dtype=np.uint64, endpoint=True)]
    for offset in (0, 2 ** 40 + 1, 2 ** 62 - n):
        idx = np.uint64(offset) + np.arange(n, dtype=np.uint64)
        for f, p in zip(Fs, Ps):
            got = Fd.phase(f, p, idx)
            assert got.dtype == np.uint64
            for i in (0, 1, 7, 8, n // 2, n - 1):
                assert int(got[i]) == Fd.phase_bigint(f, p, offset + i)
            assert [int(v) for v in got[::97]] == [Fd.phase_bigint(f, p, offset + i) for i in range(0, n, 97)]
    c, A, F, ph = Fd.tables_for((2, 3, 3))
    whole = Fd.gains(A, F, ph, 2 ** 40 + 1, 100)
    assert np.array_equal(np.concatenate((Fd.gains(A, F, ph, 2 ** 40 + 1, 37), Fd.gains(A, F, ph, 2 ** 40 + 38, 63)), axis=1), whole)
    # F = 0, Ph0 = 0, A = c = 1 is the identity; F = rint(f 2^64) is the channel model's mixer up to the rounding of f
    x = C.signal(1, 50)
    y, budget = Fd.apply(x, 0, [[1.0]], [[1.0]], [[0]], [[0]], 12345)
    assert np.array_equal(y, x.astype(np.complex128)) and np.all(budget == 18 * 2.0 ** -23 * np.abs(x.astype(np.complex128)))
    f = 0.002
    y, _ = Fd.apply(x, 0, [[1.0]], [[1.0]], [[round(f * 2 ** 64)]], [[0]], 2 ** 33)
    want, _ = C.apply(x, 0, [1], f, 0.0, 0, 2 ** 33)
    assert np.max(np.abs(y - want)) <= 2 * np.pi * (2.0 ** -31 + 2.0 ** -28) * np.max(np.abs(x))      # the phase's 32 bits and F's rounding times 2^33; the float64 product f a < 2^25 of the mixer


@pytest.mark.parametrize("shape", Fd.SHAPES)
def test_float32_emulation_stays_inside_the_budget(shape):
    """a float32 numpy emulation of the run-of-eight scheme (the phasor at the aligned index from its 24 + 8 bits, at most three float32
    rotations with tables rounded from float64, float32 sums over s, k and p, no fused multiply-add) against the float64 restatement over
    the case table: the bound itself, apart from the kernel.  Shares measured while writing: 0.13, 0.08, 0.06, 0.02, 0.01 for the five
    shapes."""
    worst = 0.0
    for idx in range(len(Fd.cases(shape))):
        d = Fd.case_data(shape, idx)
        y32 = Fd.apply32(d["x"], d["history"], d["c"], d["A"], d["F"], d["Ph0"], d["offset"])
        worst = max(worst, Fd.share_of_budget(y32, d["y"], d["budget"]))
    print("P %d S %d T %d: the float32 emulation's worst share of the budget %.3f" % (shape + (worst,)))
    assert 0 < worst <= 1.0


@pytest.mark.parametrize("S", [1, 8, 17])
def test_float32_emulation_of_the_gains_at_large_offsets(S):
    """the phasor part alone, as the issue measured it: f_d = 0.05, offsets up to 2^61, against the 12 * 2^-23 * Abar that the budget grants
    g beyond the delay line's T + P + 4"""
    rng = np.random.default_rng(S)
    A = (np.ones((1, S)) / np.sqrt(S)).astype(np.float32)
    F = np.rint(0.05 * np.cos(2 * np.pi * rng.random((1, S))) * 2.0 ** 64).astype(np.int64)
    ph = rng.integers(0, 2 ** 64 - 1, (1, S), dtype=np.uint64, endpoint=True)
    worst = 0.0
    for offset in (0, 3, 2 ** 31 - 1, 2 ** 40 + 1, 2 ** 61 + 5):
        err = np.abs(Fd.gains32(A, F, ph, offset, 8192) - Fd.gains(A, F, ph, offset, 8192))
        worst = max(worst, float(err.max() / (2.0 ** -23 * np.sum(np.abs(A.astype(np.float64))))))
    print("S %d: worst error of g %.2f * 2^-23 * Abar, of the 12 granted" % (S, worst))
    assert worst <= 12.0


def test_case_table_covers_what_the_contract_names():
    cases = Fd.all_cases()
    assert len(cases) == 2 * len(Fd.SHAPES) * len(Fd.NS)
    assert {c["shape"] for c in cases} == set(Fd.SHAPES) and {c["offset"] for c in cases} == set(Fd.OFFSETS)
    for shape in Fd.SHAPES:
        per = Fd.cases(shape)
        assert {c["n"] for c in per} == set(Fd.NS) and {c["history"] for c in per} == set(Fd.histories(shape[2])) and {c["offset"] for c in per} == set(Fd.OFFSETS)
        for fmt, outs in (("c64", 2), ("sc16", 4)):
            mine = [c for c in per if c["fmt"] == fmt]
            assert len(mine) == len(Fd.NS) and {c["in_shift"] for c in mine} == {0, 1} and {c["out_shift"] for c in mine} == set(range(outs))
        assert all(len({c["fmt"] for c in per if c["n"] == n}) == 2 for n in Fd.NS)                     # every n in both formats
        c, A, F, ph = Fd.tables_for(shape)
        assert (c.shape, A.shape, F.shape, ph.shape) == ((shape[0], shape[2]), (shape[0], shape[1]), (shape[0], shape[1]), (shape[0], shape[1]))
    assert {(c["fmt"], c["in_shift"], c["out_shift"]) for c in cases} == {("c64", i, o) for i in (0, 1) for o in (0, 1)} | {("sc16", i, o) for i in (0, 1) for o in range(4)}
    # calls that begin and end inside a run of eight, at its first and at its last index; a first piece shorter than T
    assert {c["offset"] % 8 for c in cases} >= {0, 1, 5, 7} and {(c["offset"] + c["n"]) % 8 for c in cases} >= {0, 1, 7}
    assert any(c["n"] < c["shape"][2] for c in cases)


def test_sc16_guard_band_stays_small():
    """the guard band of the sc16 comparison -- components within gain * budget of a step of q -- holds at most GUARD_CAP of the components
    of every sc16 case of the table and of the grid-bound case's gain on seeded input, and no case saturates: the gains of
    fading_model_ref.sc16_gain are chosen for that"""
    worst = 0.0
    for c in Fd.all_cases():
        if c["fmt"] != "sc16":
            continue
        d = Fd.case_data(c["shape"], Fd.cases(c["shape"]).index(c))
        want, guard = Fd.sc16(d["y"], d["budget"], Fd.sc16_gain(c["shape"]))
        assert np.abs(want.astype(np.int32)).max() < 32767
        if guard.size >= 200:
            worst = max(worst, float(guard.mean()))
        assert guard.sum() <= max(1, Fd.GUARD_CAP * guard.size), (c, guard.mean())
    print("largest guard band: %.4f of the components" % worst)
    assert 0 < worst <= Fd.GUARD_CAP


def test_grid_bound_case_arithmetic():
    """the constants mirrored in fading_model_ref are the kernel's, and each grid-bound case has 2 G + 3 tiles with a ragged last one, so
    that every workgroup takes a second tile and the first ones a third; the three pieces of check 2 stay below G tiles"""
    with open(os.path.join(ROOT, Fd.FADING_SOURCE)) as f:
        have = G.parse_constants(f.read())
    assert (have["kTile"], have["kMaxTiles"], have["kRun"]) == (Fd.K_TILE, Fd.K_MAX_TILES, Fd.K_RUN)
    assert (have["kMaxPaths"], have["kMaxSinusoids"], have["kMaxTaps"]) == (Fd.MAX_PATHS, Fd.MAX_SINUSOIDS, Fd.MAX_TAPS)
    assert {c["sc16"] for c in Fd.GRID_CASES} == {False, True}
    for case in Fd.GRID_CASES:
        geo = Fd.grid_geometry(case)
        t = geo["tiling"]
        assert t.ntiles == 2 * Fd.K_MAX_TILES + 3 and (t.total + t.mis) % Fd.K_TILE not in (0, Fd.K_TILE - 1)
        assert t.trips(0) == 3 and t.trips(3) == 2 and t.trips(Fd.K_MAX_TILES - 1) == 2
        for a, b in G.pieces(geo["n"]):
            assert -(-(b - a + 3) // Fd.K_TILE) < Fd.K_MAX_TILES
        ranges = t.edge_ranges()
        assert any(lo < t.edge(1) < hi for lo, hi in ranges) and any(lo < t.edge(2) < hi for lo, hi in ranges)
        assert (Fd.GRID_OFFSET + t.edge(1)) % 8 != 0                                   # the edge between two trips cuts a run of eight


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_preconditions(fmt):
    """what tests/test_fading_model_gpu.py::test_loop_with_a_fading_channel relies on, on the restatements alone.  The loop case through
    two paths (delays 0 and 1.5, mags 1 and 0.3, 8 taps), Rician on the first (K = 4, N = 8, seed 5), then the channel loop's CFO and
    noise: the float64 detector finds exactly the placed bursts, every maximum is at least 1e-3 from the threshold, every decision of both
    receivers is at least MARGIN from a boundary and right.  fDTs is the largest of the ladder 1e-5, 2e-5, 5e-5, 1e-4, 2e-4 at which that
    holds: 5e-5 (threshold margin 0.155, decision margins 0.146; at 1e-4 the decision margin is 0.004 and symbols are wrong).  And the
    point of the stage: |g_0| at the middle of the first burst differs from that of the last by more than |g_0| changes inside any one
    burst (0.201 against 0.028)."""
    import gfdm_amd
    c = B.loop_case()
    want = c["starts"] + c["pcp"]

    def capture(fd):
        _, _, _, y, budget = Fd.loop_stream(fd)
        if fmt == "c64":
            return y.astype(np.complex64)
        q, guard = C.sc16(y, budget, C.LOOP_GAIN)
        assert np.abs(q.astype(np.int32)).max() < 32767 and guard.mean() <= C.GUARD_CAP
        return gfdm_amd.from_sc16(q)

    held = []
    for fd in Fd.LOOP_FDTS_LADDER if fmt == "c64" else (Fd.LOOP_FDTS,):
        m = RC.loop_margins(capture(fd), want)
        print(fmt, "fDTs %g: found %s right %s threshold margin %.4f, decision margin IC %.3f MF %.3f" % (fd, m["found"], m["right"], m["thr"], m["ic"], m["mf"]))
        if RC.loop_holds(m):
            held.append(fd)
            assert np.array_equal(m["frame_start"], want)
    assert held and max(held) == Fd.LOOP_FDTS
    between, inside = Fd.loop_gain_change()
    print("|g_0| between the first and the last burst %.4f, inside one burst at most %.4f" % (between, inside))
    assert between > inside > 0
    # the second path is there: the faded stream differs from the first path's alone by far more than the budget of the comparison
    x, z, zb, _, _ = Fd.loop_stream()
    first = Fd.apply(x, 0, *[t[:1] for t in Fd.loop_tables()], 0)[0]
    assert np.max(np.abs(z - first)) > 1000 * np.max(zb)
