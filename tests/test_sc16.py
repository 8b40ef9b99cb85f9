"""CPU-side checks of the sc16 capture format (int16 I/Q, contract in include/gfdm_hip.h): to_sc16 / from_sc16 against the rule written
out, the *_sc16_* entry points exported and bound, the dtype and shape errors of the Python calls raised before a handle or a device is
touched, and the preconditions of tests/test_sc16_gpu.py on the float64 restatements alone: 12-bit quantisation leaves the detect
fixtures' peaks and core starts where pygfdm has them, and every case of burst_receive_cases decided."""
import numpy as np
import pytest

from burst_detect_ref import detect_names, load_detect, ref_detect
from burst_receive_cases import CASES, MARGIN, make_case, restatement, virtual_bursts

STEMS = ("gfdm_hip_burst_sync_find_frame_start", "gfdm_hip_burst_sync_find_frame_start_at", "gfdm_hip_burst_sync_auto_correlate",
         "gfdm_hip_burst_sync_detect", "gfdm_hip_burst_extractor_extract", "gfdm_hip_receiver_demodulate_bursts",
         "gfdm_hip_advanced_receiver_work_bursts")


def test_to_sc16_is_the_rule_written_out():
    import gfdm_amd
    rng = np.random.default_rng(16)
    x = rng.standard_normal(1000) + 1j * rng.standard_normal(1000)
    x[17] = -3.75 + 0.5j                                                # the largest component is a negative real part
    keep = x.copy()
    q = gfdm_amd.to_sc16(x)
    assert q.dtype == np.int16 and q.shape == (1000, 2) and q.flags.c_contiguous
    assert np.array_equal(x, keep)                                      # (pygfdm scales its argument in place; this one does not)
    peak = 0.9 * 2048
    g = peak / 3.75
    # truncation toward zero, of negative values too: floor would give -1844 at the peak and one less at every negative component
    want = np.stack((np.fix(x.real * g), np.fix(x.imag * g)), axis=1)
    assert np.array_equal(q, want.astype(np.int16))
    assert q[17, 0] == -1843 and np.abs(q).max() == 1843                # the peak lands at trunc(0.9 * 2048) = trunc(1843.2)
    neg = x.real < 0
    assert np.all(q[neg, 0] >= np.floor(x.real[neg] * g)) and np.any(q[neg, 0] > np.floor(x.real[neg] * g))
    q2 = gfdm_amd.to_sc16(x, peak=32767)
    assert q2[17, 0] == -32767 and np.abs(q2).max() == 32767
    assert np.array_equal(gfdm_amd.to_sc16(np.zeros(5, complex)), np.zeros((5, 2), np.int16))
    assert gfdm_amd.to_sc16(np.zeros(0, complex)).shape == (0, 2)
    for bad in (0, -1.0, 32768):
        with pytest.raises(ValueError, match="peak"):
            gfdm_amd.to_sc16(x, peak=bad)


def test_from_sc16_and_the_round_trip_of_integers():
    import gfdm_amd
    rng = np.random.default_rng(17)
    iq = rng.integers(-32768, 32768, (500, 2)).astype(np.int16)
    iq[0] = (-32768, 32767)
    f = gfdm_amd.from_sc16(iq)
    assert f.dtype == np.complex64 and f.shape == (500,)
    assert np.array_equal(f.real, iq[:, 0].astype(np.float32)) and np.array_equal(f.imag, iq[:, 1].astype(np.float32))      # unscaled, exact
    assert np.array_equal(gfdm_amd.from_sc16(iq.ravel()), f)            # the flat layout I0, Q0, I1, Q1, ...
    # exact integers whose largest component is the peak come back as they went in
    iq[1] = (1843, -7)
    small = np.clip(iq, -1843, 1843)
    back = gfdm_amd.to_sc16(gfdm_amd.from_sc16(small), peak=1843)
    assert np.array_equal(back, small)
    with pytest.raises(TypeError):
        gfdm_amd.from_sc16(iq.astype(np.int32))
    with pytest.raises(ValueError, match="odd"):
        gfdm_amd.from_sc16(iq.ravel()[:-1])
    with pytest.raises(ValueError, match="shape"):
        gfdm_amd.from_sc16(np.zeros((4, 3), np.int16))


def test_sc16_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.exported_symbols())
    for stem in STEMS:
        for kind in ("host", "device"):
            assert "%s_sc16_%s" % (stem, kind) in names and "%s_%s" % (stem, kind) in names
            assert hasattr(gfdm_amd.lib(), "%s_sc16_%s" % (stem, kind))


def _calls():
    """every Python call that takes a capture, on objects without a handle: whatever they raise, they raise before the library is asked"""
    import gfdm_amd
    sync, ex = object.__new__(gfdm_amd.BurstSync), object.__new__(gfdm_amd.BurstExtractor)
    dem, adv = object.__new__(gfdm_amd.Demodulator), object.__new__(gfdm_amd.AdvancedReceiver)
    offs = np.zeros(1, np.int64)
    return [lambda s: sync.find_frame_start(s), lambda s: sync.find_frame_start_at(s, offs), lambda s: sync.auto_correlate(s),
            lambda s: sync.detect(s, 0.5, 100), lambda s: ex.extract(s, offs), lambda s: dem.demodulate_bursts(s, offs),
            lambda s: adv.demodulate_bursts(s, offs)]


def test_dtype_and_shape_errors_come_before_any_device():
    import torch
    for call in _calls():
        for dt in (np.int8, np.uint8, np.uint16, np.int32, np.int64):
            with pytest.raises(TypeError, match="int16"):
                call(np.zeros((64, 2), dt))
        with pytest.raises(TypeError, match="int16"):
            call(torch.zeros(64, 2, dtype=torch.int32))
        with pytest.raises(ValueError, match="odd"):
            call(np.zeros(63, np.int16))
        with pytest.raises(ValueError, match="shape"):
            call(np.zeros((21, 3), np.int16))
        with pytest.raises(ValueError, match="shape"):
            call(np.zeros((8, 4, 2), np.int16))
        with pytest.raises(TypeError, match="contiguous"):
            call(np.zeros((64, 4), np.int16)[:, :2])                    # a strided (n, 2) view
        with pytest.raises(TypeError, match="contiguous"):
            call(np.zeros(128, np.int16)[::2])
        with pytest.raises(TypeError, match="contiguous"):              # as the complex path: a tensor off the device, or strided
            call(torch.zeros(64, 2, dtype=torch.int16))
        with pytest.raises(TypeError, match="contiguous"):
            call(torch.zeros(64, 2, dtype=torch.complex64))


# ---- the preconditions of tests/test_sc16_gpu.py, on the float64 restatements alone ----
@pytest.mark.parametrize("name", detect_names())
def test_quantisation_leaves_the_detect_fixtures_decided(name):
    import gfdm_amd
    g = load_detect(name)
    f = gfdm_amd.from_sc16(gfdm_amd.to_sc16(g["stream"]))
    ref = ref_detect(f, g["preamble"], g["K"], g["cp_len"], g["window_len"], g["threshold"], g["min_distance"], g["lead"])
    assert np.array_equal(ref["peaks"], g["peaks"]) and np.array_equal(ref["frame_start"], g["core_starts"])
    n = g["peaks"].size
    if n:
        d_cfo, d_met = np.max(np.abs(ref["cfo"] - g["cfo"])), np.max(np.abs(ref["metric"] - g["metric"]))
        margin = np.min(np.abs(ref["ic"][ref["peaks"]] - g["threshold"]))
        print(name, "cfo shift %.3e metric shift %.3e threshold margin %.3f" % (d_cfo, d_met, margin))
        assert d_cfo < 1e-4 and margin > 0.4       # the GPU test's cfo bound, 2e-4, leaves fp32 the 1e-4 of tests/test_burst_detect_gpu.py


@pytest.mark.parametrize("name", sorted(CASES))
def test_quantisation_leaves_the_receive_cases_decided(name):
    import gfdm_amd
    M, K, L, A, nb, seed = CASES[name]
    c = make_case(M, K, L, A, nb, seed)
    f = gfdm_amd.from_sc16(gfdm_amd.to_sc16(c["stream"]))
    out, margin = restatement(c, virtual_bursts(f, c["starts"], c["sc_rot"], 0, c["F"]), 2)
    print(name, "margin", margin)
    assert margin > MARGIN
    assert np.array_equal(out.real > 0, c["sym"].real > 0) and np.array_equal(out.imag > 0, c["sym"].imag > 0)
