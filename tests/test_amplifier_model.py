"""CPU-side checks of the amplifier model (contract in include/gfdm_hip.h, gfdm_hip_amplifier_model): the entry points are exported and
bound, the argument table answers without a device with every bound hit from both sides, create refuses what it can before any device is
touched and there is no CPU fallback, Python-side argument errors come before any device, the helpers give their known answers, the
float32 numpy evaluation of tests/amplifier_model_ref.py stays inside the budgets (the bounds themselves, apart from the kernel) and the
naive Rapp formula does not, the case tables cover what the contract names, the mirrored constants are the kernel's, the sc16 guard band
stays small and the preconditions of the end-to-end GPU test hold on the restatements alone."""
import ctypes
import os

import numpy as np
import pytest

import amplifier_model_ref as Am
import burst_shaper_ref as B
import grid_bound_cases as G
import resampler_cases as RC
from conftest import ROOT, have_gpu

PLAIN = ("create", "destroy", "kind", "n_params", "n_delays", "n_orders", "params", "coefficients", "drive", "set_drive", "check")
CLIP, RAPP, SALEH, POLY = 0, 1, 2, 3
NAN, INF = float("nan"), float("inf")


def test_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.capi.exported_symbols())
    for kind in ("host", "device", "sc16_host", "sc16_device"):
        assert "gfdm_hip_amplifier_model_apply_%s" % kind in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_amplifier_model_apply_%s" % kind)
    for name in PLAIN:
        assert "gfdm_hip_amplifier_model_" + name in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_amplifier_model_" + name)
    assert [n for n in names if n.startswith("gfdm_hip_amplifier_model_set_")] == ["gfdm_hip_amplifier_model_set_drive"]     # the one setter
    assert gfdm_amd.AmplifierModel is gfdm_amd.capi.AmplifierModel
    assert gfdm_amd.amplifier_curve is gfdm_amd.capi.amplifier_curve and gfdm_amd.amplifier_drive is gfdm_amd.capi.amplifier_drive
    assert gfdm_amd.capi.AMPLIFIER_KINDS == {"clip": CLIP, "rapp": RAPP, "saleh": SALEH, "poly": POLY}


BIG = 3.5e38                       # finite as a double, not as a float
# (kind, params, n_delays, n_orders, drive, n, history, gain) -> what the message names; None = accepted
TABLE = [
    ((CLIP, (1.0,), 0, 0, 1.0, 0, 0, 1.0), None),
    ((CLIP, (1e-30,), 0, 0, 0.0, 1 << 40, 63, -3.5), None),
    ((RAPP, (1.0, 1.0, 0.5), 0, 0, 1.0, 1, 0, 0.0), None),
    ((RAPP, (1e-3, 1e3, 16.0), 0, 0, 3e38, 1, 0, 1.0), None),
    ((SALEH, (2.0, 0.0, -4.0, 0.0), 0, 0, 1.0, 1, 0, 1.0), None),
    ((SALEH, (-2.0, 1.0, 4.0, 9.0), 0, 0, 1.0, 1, 0, 1.0), None),
    ((POLY, (), 1, 1, 1.0, 1, 0, 1.0), None),
    ((POLY, (), 16, 5, 1.0, 1 << 59, (1 << 60) - (1 << 59) - 1, 1.0), None),       # 8 (history + n) just fits
    ((-1, (1.0,), 0, 0, 1.0, 1, 0, 1.0), "kind"),
    ((4, (1.0,), 0, 0, 1.0, 1, 0, 1.0), "kind"),
    ((CLIP, (), 0, 0, 1.0, 1, 0, 1.0), "n_params"),
    ((CLIP, (1.0, 1.0), 0, 0, 1.0, 1, 0, 1.0), "n_params"),
    ((RAPP, (1.0, 1.0), 0, 0, 1.0, 1, 0, 1.0), "n_params"),
    ((SALEH, (1.0, 1.0, 1.0), 0, 0, 1.0, 1, 0, 1.0), "n_params"),
    ((POLY, (1.0,), 1, 1, 1.0, 1, 0, 1.0), "n_params"),
    ((CLIP, (0.0,), 0, 0, 1.0, 1, 0, 1.0), "A must be > 0"),
    ((CLIP, (-1.0,), 0, 0, 1.0, 1, 0, 1.0), "A must be > 0"),
    ((CLIP, (1e-60,), 0, 0, 1.0, 1, 0, 1.0), "A must be > 0"),                     # 0 as a float
    ((CLIP, (NAN,), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((CLIP, (INF,), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((CLIP, (BIG,), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((RAPP, (0.0, 1.0, 2.0), 0, 0, 1.0, 1, 0, 1.0), "g must be > 0"),
    ((RAPP, (-1.0, 1.0, 2.0), 0, 0, 1.0, 1, 0, 1.0), "g must be > 0"),
    ((RAPP, (1.0, 0.0, 2.0), 0, 0, 1.0, 1, 0, 1.0), "A must be > 0"),
    ((RAPP, (1.0, 1.0, 0.4999), 0, 0, 1.0, 1, 0, 1.0), "p must lie"),
    ((RAPP, (1.0, 1.0, 16.001), 0, 0, 1.0, 1, 0, 1.0), "p must lie"),
    ((RAPP, (1.0, 1.0, NAN), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((RAPP, (1e15, 1e-4, 2.0), 0, 0, 1.0, 1, 0, 1.0), None),                        # g^2 / A^2 = 1e38: still a float
    ((RAPP, (1e-15, 1e7, 2.0), 0, 0, 1.0, 1, 0, 1.0), None),                        # 1e-44: a denormal, not 0
    ((RAPP, (1e30, 1e-30, 2.0), 0, 0, 1.0, 1, 0, 1.0), "g^2 / A^2"),                # inf as a float
    ((RAPP, (1e16, 1e-4, 2.0), 0, 0, 1.0, 1, 0, 1.0), "g^2 / A^2"),
    ((RAPP, (1e-30, 1e30, 2.0), 0, 0, 1.0, 1, 0, 1.0), "g^2 / A^2"),                # 0 as a float
    ((RAPP, (1.0, -INF, 2.0), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((SALEH, (2.0, -1e-9, 4.0, 9.0), 0, 0, 1.0, 1, 0, 1.0), "ba must be >= 0"),
    ((SALEH, (2.0, 1.0, 4.0, -1e-9), 0, 0, 1.0, 1, 0, 1.0), "bp must be >= 0"),
    ((SALEH, (INF, 1.0, 4.0, 9.0), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((SALEH, (2.0, 1.0, NAN, 9.0), 0, 0, 1.0, 1, 0, 1.0), "finite"),
    ((POLY, (), 0, 1, 1.0, 1, 0, 1.0), "n_delays"),
    ((POLY, (), 17, 1, 1.0, 1, 0, 1.0), "n_delays"),
    ((POLY, (), 1, 0, 1.0, 1, 0, 1.0), "n_orders"),
    ((POLY, (), 1, 6, 1.0, 1, 0, 1.0), "n_orders"),
    ((CLIP, (1.0,), 1, 0, 1.0, 1, 0, 1.0), "must be 0"),
    ((SALEH, (2.0, 1.0, 4.0, 9.0), 0, 1, 1.0, 1, 0, 1.0), "must be 0"),
    ((CLIP, (1.0,), 0, 0, -1e-9, 1, 0, 1.0), "drive"),
    ((CLIP, (1.0,), 0, 0, NAN, 1, 0, 1.0), "drive"),
    ((CLIP, (1.0,), 0, 0, INF, 1, 0, 1.0), "drive"),
    ((CLIP, (1.0,), 0, 0, BIG, 1, 0, 1.0), "drive"),
    ((CLIP, (1.0,), 0, 0, 1.0, 1, 0, NAN), "gain"),
    ((CLIP, (1.0,), 0, 0, 1.0, 1, 0, -INF), "gain"),
    ((CLIP, (1.0,), 0, 0, 1.0, -1, 0, 1.0), "n must"),
    ((CLIP, (1.0,), 0, 0, 1.0, 1, -1, 1.0), "history"),
    ((CLIP, (1.0,), 0, 0, 1.0, (1 << 62) + 1, 0, 1.0), "2^62"),
    ((CLIP, (1.0,), 0, 0, 1.0, 1 << 60, 0, 1.0), "overflow"),                      # 8 n
    ((CLIP, (1.0,), 0, 0, 1.0, 1, 1 << 60, 1.0), "overflow"),                      # 8 (history + n)
    ((POLY, (), 3, 3, 1.0, 1 << 59, (1 << 60) - (1 << 59), 1.0), "overflow"),
]


def _check(L, args):
    kind, params, Q, K, drive, n, history, gain = args
    p = (ctypes.c_double * max(len(params), 1))(*params)
    return L.gfdm_hip_amplifier_model_check(kind, p, len(params), Q, K, drive, n, history, gain)


@pytest.mark.parametrize("args,match", TABLE)
def test_argument_table(args, match):
    import gfdm_amd
    L = gfdm_amd.lib()
    rc = _check(L, args)
    if match is None:
        assert rc == gfdm_amd.capi.OK
    else:
        assert rc == gfdm_amd.capi.EINVAL
        assert match in L.gfdm_hip_last_error().decode()


def test_null_params():
    import gfdm_amd
    L = gfdm_amd.lib()
    assert L.gfdm_hip_amplifier_model_check(CLIP, None, 1, 0, 0, 1.0, 1, 0, 1.0) == gfdm_amd.capi.EINVAL and b"NULL params" in L.gfdm_hip_last_error()
    assert L.gfdm_hip_amplifier_model_check(POLY, None, 0, 2, 2, 1.0, 1, 0, 1.0) == gfdm_amd.capi.OK


def test_create_refuses_before_any_device_and_there_is_no_cpu_fallback():
    """what create can refuse without a device it refuses first (here, without a GPU, every one of these would otherwise answer ENODEV);
    with good arguments: ENODEV without a device, the getters with one"""
    import gfdm_amd
    AM = gfdm_amd.AmplifierModel
    c = Am.poly_coefficients(3, 3)
    bad = c.copy()
    bad[1, 2] = NAN
    for make, match in ((lambda: AM.clip(0.0), "A must be > 0"), (lambda: AM.clip(1.0, drive=-1.0), "drive"), (lambda: AM.rapp(1.0, 1.0, 17.0), "p must lie"),
                        (lambda: AM.rapp(1.0, 1.0, 0.25), "p must lie"), (lambda: AM.saleh(1.0, -1.0, 1.0, 1.0), "ba"), (lambda: AM.saleh(1.0, 1.0, 1.0, -1.0), "bp"),
                        (lambda: AM.poly(np.ones((17, 1))), "n_delays"), (lambda: AM.poly(np.ones((1, 6))), "n_orders"), (lambda: AM.poly(np.ones((0, 1))), "n_delays"),
                        (lambda: AM.poly(bad), "coefficients must be finite"), (lambda: AM.poly(np.ones((2, 2, 2))), "shape"),
                        (lambda: AM("clip", (1.0, 2.0)), "takes the parameters"), (lambda: AM("tube", (1.0,)), "kind must be one of"),
                        (lambda: AM("clip", (1.0,), c=c), "no coefficients"), (lambda: AM.clip(INF), "finite")):
        with pytest.raises(ValueError, match=match):
            make()
    L = gfdm_amd.lib()
    h = ctypes.c_void_p()
    assert L.gfdm_hip_amplifier_model_create(ctypes.byref(h), POLY, None, 0, None, 2, 2, 1.0, 0) == gfdm_amd.capi.EINVAL
    assert b"NULL coefficients" in L.gfdm_hip_last_error() and not h.value
    if have_gpu():
        am = AM.rapp(2.0, 1.5, 0.1 + 0.2, drive=0.75)
        assert (am.kind(), am.n_delays(), am.n_orders(), am.drive) == ("rapp", 0, 0, 0.75) and am.coefficients() is None
        assert np.array_equal(am.params(), np.array([2.0, 1.5, 0.1 + 0.2], np.float32).astype(np.float64))
        am = AM.poly(c)
        assert (am.kind(), am.n_delays(), am.n_orders(), am.drive) == ("poly", 3, 3, 1.0) and am.params().size == 0
        assert am.coefficients().dtype == np.complex64 and np.array_equal(am.coefficients(), c)
        am.drive = 0.0
        assert am.drive == 0.0
        for d in (-1.0, NAN, INF):
            with pytest.raises(ValueError, match="drive"):
                am.set_drive(d)
        assert am.drive == 0.0
    else:
        for make in (lambda: AM.clip(1.0), lambda: AM.rapp(1.0, 1.0, 2.0), lambda: AM.saleh(*Am.SALEH_CLASSIC), lambda: AM.poly(c)):
            with pytest.raises(gfdm_amd.GfdmHipError, match="no HIP device") as e:
                make()
            assert e.value.status == gfdm_amd.capi.ENODEV


def test_python_argument_errors_come_before_any_device():
    import torch
    import gfdm_amd
    am = object.__new__(gfdm_amd.AmplifierModel)           # no handle: whatever these calls raise, they raise before the library is asked
    x = np.zeros(10, np.complex64)
    for dt in (np.int16, np.int32, np.uint8, bool):
        with pytest.raises(TypeError, match="x must be complex samples"):
            am.apply(np.zeros(10, dt))
    with pytest.raises(TypeError, match="x must be a contiguous complex64"):
        am.apply(torch.zeros(10, dtype=torch.complex64))                        # a tensor off the device
    with pytest.raises(ValueError, match="int16 out"):
        am.apply(x, gain=2.0)
    with pytest.raises(TypeError, match="int16"):
        am.apply(x, sc16=True, out=np.zeros(10, np.complex64))
    with pytest.raises(TypeError, match="complex64"):
        am.apply(x, sc16=False, out=np.zeros((10, 2), np.int16))
    with pytest.raises(ValueError, match="shape"):
        am.apply(x, out=np.zeros((10, 3), np.int16))
    with pytest.raises(TypeError, match="numpy array, as x is"):
        am.apply(x, out=torch.zeros(10, dtype=torch.complex64))
    for history in (-1, 11):
        with pytest.raises(ValueError, match="history"):
            am.apply(x, history=history)
    with pytest.raises(RuntimeError, match="out holds 10 samples, expected 7"):
        am.apply(x, history=3, out=np.zeros(10, np.complex64))


# ---- the helpers ----
def test_helper_known_answers():
    import gfdm_amd
    curve, drive = gfdm_amd.amplifier_curve, gfdm_amd.amplifier_drive
    a = np.array([0.0, 0.5, 1.0, 2.0, 1e6])
    am, pm = curve(("clip", 1.0), a)
    assert am.dtype == np.float64 and np.array_equal(am, [0.0, 0.5, 1.0, 1.0, 1.0]) and not pm.any()
    # Rapp at the knee g a = A: A 2^(-1 / (2 p)); far above it: A; far below: g a
    for p in (0.5, 1.0, 2.0, 16.0):
        am, pm = curve(("rapp", 2.0, 1.5, p), np.array([0.75, 1e-6, 1e30]))
        assert np.allclose(am, [1.5 * 2.0 ** (-0.5 / p), 2e-6, 1.5], rtol=1e-12) and not pm.any()
    # Saleh: the AM/AM peak aa / (2 sqrt ba) at r = 1 / ba; the phase climbs to ap / bp
    aa, ba, ap, bp = np.array(Am.SALEH_CLASSIC, np.float32).astype(np.float64)
    am, pm = curve(("saleh",) + Am.SALEH_CLASSIC, np.array([1.0 / np.sqrt(ba), 1e4]))
    assert am[0] == pytest.approx(aa / (2 * np.sqrt(ba)), rel=1e-12) and pm[0] == pytest.approx(ap / ba / (1 + bp / ba), rel=1e-12)
    assert pm[1] == pytest.approx(ap / bp, rel=1e-6)
    # a polynomial: the curve of a constant envelope sums over the delays
    c = np.array([[1.0, -0.2 + 0.05j], [0.5, 0.0]], np.complex64)
    am, pm = curve(("poly", c), np.array([0.25]))
    y = 1.5 * 0.25 + complex(c[0, 1]) * 0.25 ** 3
    assert am[0] == pytest.approx(abs(y), rel=1e-12) and pm[0] == pytest.approx(np.angle(y), rel=1e-12)
    # the curves are the restatement's on real inputs
    for sp in Am.closed_forms():
        amps = np.exp(np.linspace(-6, 3, 50)).astype(np.float32)
        y, _ = Am.apply(amps.astype(np.complex64), 0, sp)
        am, pm = curve((sp["kind"],) + tuple(sp["p"]), amps.astype(np.float64))
        assert np.allclose(am, np.abs(y), rtol=1e-12) and np.allclose(pm, np.angle(y), atol=1e-12)
    assert drive(1.0, 0.0) == 1.0 and drive(4.0, 0.0, 2.0) == 1.0 and drive(1.0, 20.0) == pytest.approx(0.1, rel=1e-15)
    assert drive(0.37, 6.0, 1.3) == Am.backoff_drive(0.37, 6.0, 1.3)
    d = drive(0.37, 6.0, 1.3)
    assert 10 * np.log10(1.3 ** 2 / (d * d * 0.37)) == pytest.approx(6.0, abs=1e-12)
    for bad in ((0.0, 6.0, 1.0), (-1.0, 6.0, 1.0), (NAN, 6.0, 1.0), (1.0, 6.0, 0.0), (1.0, 6.0, INF)):
        with pytest.raises(ValueError):
            drive(*bad)


# ---- the budgets, apart from the kernel ----
N_ACC = 2 * Am.K_TILE + 5


def test_float32_evaluation_of_the_closed_forms():
    """what plain float32 numpy needs of the closed forms' budgets on the inputs of the GPU test: under half the derived floors (8, 8,
    16), so B of the GPU test is the floor.  Measured while writing: 1.1 (clip), 1.4 .. 1.9 (rapp), 1.9 and 3.8 (saleh)."""
    for i, sp in enumerate(Am.closed_forms()):
        x = Am.wide_signal(i, N_ACC)
        y, _ = Am.apply(x, 0, sp)
        need = Am.need_of(Am.apply32(x, 0, sp), y)
        print("%s: float32 numpy needs %.2f * 2^-23 |y|; B = %.1f" % (Am.tag(sp), need, Am.closed_form_B(x, sp)))
        assert 0 < need <= 0.5 * Am.floor_of(sp["kind"]) and Am.closed_form_B(x, sp) == Am.floor_of(sp["kind"])
        if sp["kind"] == "saleh":
            u = x.astype(np.complex128)
            r = np.abs(u) ** 2
            assert np.all(np.abs(sp["p"][2] * r / (1 + sp["p"][3] * r)) <= np.pi)                    # the range the floor of 16 is derived for


def test_float32_horner_stays_inside_the_budget():
    """Measured while writing: 0.00 (the identity), 0.07, 0.14, 0.14, 0.11 of the budget for the five shapes."""
    for i, sp in enumerate(Am.polys()):
        Q = Am.delays(sp)
        x = Am.wide_signal(100 + i, N_ACC + Q - 1)
        y, budget = Am.apply(x, Q - 1, sp)
        share = Am.share_of_budget(Am.apply32(x, Q - 1, sp), y, budget)
        print("%s: the float32 Horner's worst share of the budget %.3f" % (Am.tag(sp), share))
        assert share <= 1.0 and (share > 0 or sp["c"].shape == (1, 1))


def test_rapp_holds_where_the_naive_formula_gives_zero():
    sp = Am.spec("rapp", 2.0, 1.5, 16.0)
    x = (1.5 * np.exp2(np.linspace(-2, 60, 500))).astype(np.complex64)
    y, _ = Am.apply(x, 0, sp)
    assert np.all(np.isfinite(y)) and np.all(np.abs(y) > 0) and np.all(np.abs(y) <= 1.5 * (1 + 2.0 ** -40))
    assert Am.need_of(Am.apply32(x, 0, sp), y) <= 4.0
    naive = Am.rapp32_naive(x, sp)
    assert np.count_nonzero(naive == 0) > 400                                      # relative error 1


def test_restatement_known_answers():
    x = Am.wide_signal(7, 300)
    u = x.astype(np.complex128)
    # CLIP: below the knee u itself, above it modulus A and the phase of u
    y, _ = Am.apply(x, 0, Am.spec("clip", 1.0))
    low = np.abs(u) ** 2 <= 1.0
    assert low.any() and (~low).any() and np.array_equal(y[low], u[low]) and np.allclose(np.abs(y[~low]), 1.0, rtol=1e-15)
    assert np.allclose(y[~low] / u[~low], (y[~low] / u[~low]).real, rtol=1e-15)
    # POLY(1, 1) is a gain; the drive scales u; history: the memoryless kinds drop it, POLY reads it
    y, b = Am.apply(x, 0, Am.spec("poly", c=[[2.0]]), 0.5)
    assert np.array_equal(y, u) and np.array_equal(b, 13 * Am.EPS * np.abs(u))
    sp = Am.spec("poly", c=Am.poly_coefficients(3, 3))
    whole, _ = Am.apply(x, 0, sp)
    assert np.array_equal(Am.apply(x, 100, sp)[0], whole[100:]) and not np.array_equal(Am.apply(x[100:], 0, sp)[0][:2], whole[100:102])
    assert np.array_equal(Am.apply(x[98:], 2, sp)[0], whole[100:])
    # the two tones: the closed-form powers to 1e-6 on the complex64 input (the slack of the GPU test holds their rounding)
    y, budget = Am.apply(Am.two_tones(), 0, Am.spec("poly", c=[1, Am.TONE_C3]))
    Y = np.fft.fft(y[:Am.TONE_NFFT]) / Am.TONE_NFFT
    for k, want in Am.two_tone_answer().items():
        assert abs(Y[k]) ** 2 == pytest.approx(want, rel=1e-6)
    assert budget.max() <= Am.two_tone_slack()


def test_case_table_covers_what_the_contract_names():
    kinds = Am.geometry_kinds()
    assert {sp["kind"] for sp in kinds} == set(Am.KINDS)
    assert any(sp["kind"] == "poly" and not sp["c"].imag.any() for sp in kinds) and any(sp["kind"] == "poly" and sp["c"].imag.any() for sp in kinds)
    assert Am.GEOMETRY_NS == (1, 2, 3, Am.K_TILE - 1, Am.K_TILE, Am.K_TILE + 1)
    for ki, sp in enumerate(kinds):
        cases = Am.geometry_cases(ki)
        Q = Am.delays(sp)
        assert {c["n"] for c in cases} == set(Am.GEOMETRY_NS) and {c["history"] for c in cases} == {0, Q - 1, Q + 4}
        assert len(cases) == len(Am.GEOMETRY_NS) * len(set(Am.histories(sp))) or Q == 1
        for c in cases:
            assert set(c["aligns"]) == {("c64", i, o) for i in (0, 1) for o in (0, 1)} | {("sc16", i, o) for i in (0, 1) for o in range(4)}
    assert {sp["c"].shape for sp in Am.polys()} == set(Am.POLY_SHAPES) == {(1, 1), (1, 2), (3, 3), (4, 5), (16, 5)}
    assert sorted(sp["p"][2] for sp in Am.closed_forms() if sp["kind"] == "rapp") == [0.5, 1, 2, 3, 10]
    assert [sp["kind"] for sp in Am.closed_forms()].count("saleh") == 2 and Am.closed_forms()[0]["kind"] == "clip"


def test_grid_bound_case_arithmetic():
    """the constants mirrored in amplifier_model_ref are the kernel's, and each grid-bound case has 2 G + 3 tiles with a ragged last one, so
    that every workgroup takes a second tile and the first ones a third; the three pieces stay below G tiles.  The tile arithmetic is
    gfdm_streamtile.h's StreamTiles alone (brute-forced by tests/sanitize/streamtile_check.cc): the kernel has no host half of its own."""
    with open(os.path.join(ROOT, Am.SOURCE)) as f:
        have = G.parse_constants(f.read())
    assert (have["kTile"], have["kMaxTiles"], have["kLanes"]) == (Am.K_TILE, Am.K_MAX_TILES, Am.K_LANES)
    assert (have["kMaxDelays"], have["kMaxOrders"]) == (Am.MAX_DELAYS, Am.MAX_ORDERS)
    assert {c["sc16"] for c in Am.GRID_CASES} == {False, True} and all(c["mis"] == 1 for c in Am.GRID_CASES)
    for case in Am.GRID_CASES:
        geo = Am.grid_geometry(case)
        t = geo["tiling"]
        assert t.ntiles == 2 * Am.K_MAX_TILES + 3 and (t.total + t.mis) % Am.K_TILE not in (0, Am.K_TILE - 1)
        assert 60e6 <= 8 * geo["n"] <= 72e6
        assert t.trips(0) == 3 and t.trips(3) == 2 and t.trips(Am.K_MAX_TILES - 1) == 2
        for a, b in G.pieces(geo["n"]):
            assert -(-(b - a + 3) // Am.K_TILE) < Am.K_MAX_TILES
        ranges = t.edge_ranges()
        assert any(lo < t.edge(1) < hi for lo, hi in ranges) and any(lo < t.edge(2) < hi for lo, hi in ranges)


def test_sc16_guard_band_stays_small():
    """the guard band of the sc16 comparison -- components within gain * budget of a step of q -- holds at most GUARD_CAP of the components
    of every geometry case with 200 components or more, and no case saturates: the gains of amplifier_model_ref.sc16_gain are chosen for that"""
    worst = 0.0
    for ki, sp in enumerate(Am.geometry_kinds()):
        gain = Am.sc16_gain(sp)
        for c in Am.geometry_cases(ki):
            x = Am.geometry_signal(c["seed"], c["history"] + c["n"])
            y, budget = Am.apply(x, c["history"], sp)
            want, guard = Am.sc16(y, budget, gain)
            assert np.abs(want.astype(np.int32)).max() < 32767
            if guard.size >= 200:
                worst = max(worst, float(guard.mean()))
                assert guard.mean() <= Am.GUARD_CAP, (Am.tag(sp), c["n"], guard.mean())
    print("largest guard band: %.4f of the components" % worst)
    assert 0 < worst <= Am.GUARD_CAP


def test_loop_preconditions():
    """what tests/test_amplifier_model_gpu.py::test_end_to_end relies on, on the restatements alone.  The loop case through RAPP(g = 1, A =
    1, p = 2) at a drive that puts the mean power of the placed stream `backoff` dB below A^2, the level taken back by the channel's tap
    1 / d, then the channel loop's CFO and noise: the float64 detector finds exactly the placed bursts, every maximum is at least 1e-3 from
    the threshold, every decision of both receivers is at least MARGIN from a boundary and right.  The back-off is the smallest of the
    ladder 12, 9, 6, 4, 3 dB at which that holds: 6 dB (decision margins 0.260, 0.254, 0.196 at 12, 9, 6 dB; 0.087 at 4 dB, 0.033 at 3)."""
    c = B.loop_case()
    want = c["starts"] + c["pcp"]
    held = []
    for backoff in Am.LOOP_BACKOFF_LADDER:
        x, d, z, y, budget = Am.loop_stream(backoff)
        m = RC.loop_margins(y.astype(np.complex64), want)
        print("back-off %g dB, drive %.4f: found %s right %s threshold margin %.4f, decision margin IC %.3f MF %.3f" % (backoff, d, m["found"], m["right"], m["thr"], m["ic"], m["mf"]))
        if RC.loop_holds(m):
            held.append(backoff)
            assert np.array_equal(m["frame_start"], want)
    assert held and min(held) == Am.LOOP_BACKOFF
    # the amplifier is at work there: the stream it returns differs from d x by far more than the budget of the comparison
    x, d, z, _, _ = Am.loop_stream()
    assert np.max(np.abs(z - d * x.astype(np.complex128))) > 1000 * 8 * Am.EPS * np.max(np.abs(z))
