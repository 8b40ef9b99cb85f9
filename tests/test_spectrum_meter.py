"""CPU-side tests of the spectrum meter (contract in include/gfdm_hip.h, gfdm_hip_spectrum_meter): the exports and the argument tables of
the library, plan, the numpy helpers of the package, and the numpy restatement of tests/spectrum_meter_ref.py against known answers --
the yardstick of tests/test_spectrum_meter_gpu.py must itself be right."""
import ctypes
import math
import os

import numpy as np
import pytest

import grid_bound_cases as G
import spectrum_meter_ref as R
from conftest import ROOT, have_gpu

EINVAL = -3
ENTRY_POINTS = ("create", "destroy", "nfft", "hop", "window", "plan", "totals_device", "totals_bytes", "reset", "read") + tuple(
    stem + infix + flavour for stem in ("accumulate", "accumulate_at", "power") for infix in ("", "_sc16") for flavour in ("_host", "_device"))


def test_exports_and_python_surface():
    import gfdm_amd
    bound = gfdm_amd.exported_symbols()
    assert sorted(n for n in bound if n.startswith("gfdm_hip_spectrum_meter_")) == sorted("gfdm_hip_spectrum_meter_" + n for n in ENTRY_POINTS)
    for name in ("plan", "update", "update_at", "power", "reset", "read", "totals_ptr", "psd", "band_power", "mean_power", "papr_db", "ccdf", "nfft", "hop",
                 "window"):
        assert callable(getattr(gfdm_amd.SpectrumMeter, name))
    assert gfdm_amd.SpectrumMeter.HEAD == R.HEAD and gfdm_amd.SpectrumMeter.HIST_BINS == R.HIST_BINS
    for name in ("spectrum_window", "subcarrier_power", "oob_ratio_db"):
        assert callable(getattr(gfdm_amd, name))


def test_the_mirrored_constants_are_the_source_s():
    with open(os.path.join(ROOT, R.SOURCE)) as f:
        have = G.parse_constants(f.read())
    for name, value in R.CONSTANTS.items():
        assert have.get(name) == value, name
    assert R.TILE == R.CONSTANTS["kPowerTile"] and R.HIST_BINS == R.CONSTANTS["kHistBins"] and R.HIST_BIAS == R.CONSTANTS["kHistBias"]
    for c in R.GRID_CASES:
        geo = R.grid_geometry(c)
        # more trips than workgroups: the runs are contiguous, so 2 G + 3 trips are three trips a workgroup on ceil((2 G + 3) / 3) workgroups
        assert geo["trips"] >= 2 * R.CONSTANTS["kMaxGroups"] + 3 and 1 < geo["groups"] <= R.CONSTANTS["kMaxGroups"]
        assert geo["per"] == 3 * (R.CONSTANTS["kSlotSamples"] // c["nfft"]) and geo["groups"] == -(-geo["trips"] // 3)
        assert all(-(-(b - a) // geo["per"]) < R.CONSTANTS["kMaxGroups"] and (b - a) // (R.CONSTANTS["kSlotSamples"] // c["nfft"]) < R.CONSTANTS["kMaxGroups"]
                   for a, b in G.pieces(geo["n_seg"]))                               # the three pieces stay below G trips: one trip a workgroup
        assert geo["n_seg"] % geo["per"] and R.segments_of(c["nfft"], c["hop"], geo["n"]) == geo["n_seg"]
        assert geo["power_tiles"] == -(-geo["power_n"] // R.TILE) >= 2 * R.CONSTANTS["kPowerGroups"] + 3


def test_einval_table_needs_no_device():
    import gfdm_amd
    L = gfdm_amd.lib()
    h = ctypes.c_void_p()
    w = np.ones(4096, np.float32)
    create = L.gfdm_hip_spectrum_meter_create
    for nfft, hop in ((8, 4), (0, 1), (-16, 1), (48, 8), (8192, 64), (4097, 1), (64, 0), (64, 65), (64, -1)):
        assert create(ctypes.byref(h), w.ctypes.data, nfft, hop, 0) == EINVAL, (nfft, hop)
        assert not h.value
    assert create(ctypes.byref(h), None, 64, 32, 0) == EINVAL
    assert create(None, w.ctypes.data, 64, 32, 0) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        v = w.copy()
        v[63] = bad
        assert create(ctypes.byref(h), v.ctypes.data, 64, 32, 0) == EINVAL
        assert b"finite" in L.gfdm_hip_last_error()
    v = w.copy()
    v[64] = np.nan                                                     # behind the window: not read
    rc = create(ctypes.byref(h), v.ctypes.data, 64, 64, 0)
    if have_gpu():
        assert rc == 0 and L.gfdm_hip_spectrum_meter_destroy(h) == 0
    else:
        assert rc == gfdm_amd.capi.ENODEV and not h.value
    p = w.ctypes.data
    assert L.gfdm_hip_spectrum_meter_nfft(None) == EINVAL and L.gfdm_hip_spectrum_meter_hop(None) == EINVAL
    assert L.gfdm_hip_spectrum_meter_window(None, p) == EINVAL and L.gfdm_hip_spectrum_meter_totals_bytes(None) == EINVAL
    assert L.gfdm_hip_spectrum_meter_totals_device(None) is None
    assert L.gfdm_hip_spectrum_meter_reset(None, None) == EINVAL and L.gfdm_hip_spectrum_meter_read(None, p, p, p, p, None) == EINVAL
    for infix in ("", "_sc16"):
        assert getattr(L, "gfdm_hip_spectrum_meter_accumulate%s_host" % infix)(None, p, 64) == EINVAL
        assert getattr(L, "gfdm_hip_spectrum_meter_accumulate%s_device" % infix)(None, p, 64, None) == EINVAL
        assert getattr(L, "gfdm_hip_spectrum_meter_power%s_host" % infix)(None, p, 64) == EINVAL
        assert getattr(L, "gfdm_hip_spectrum_meter_power%s_device" % infix)(None, p, 64, None) == EINVAL
        assert getattr(L, "gfdm_hip_spectrum_meter_accumulate_at%s_host" % infix)(None, p, 64, p, None, 0, 1, 1) == EINVAL
        assert getattr(L, "gfdm_hip_spectrum_meter_accumulate_at%s_device" % infix)(None, p, 64, p, None, 0, 1, 1, None) == EINVAL
    with pytest.raises(ValueError, match="power of two"):
        gfdm_amd.SpectrumMeter(100)
    with pytest.raises(ValueError, match="hop"):
        gfdm_amd.SpectrumMeter(64, hop=65)
    with pytest.raises(ValueError, match="expected nfft"):
        gfdm_amd.SpectrumMeter(64, window=np.ones(63))
    with pytest.raises(ValueError, match="window must be one of"):
        gfdm_amd.SpectrumMeter(64, window="kaiser")


def test_plan():
    import gfdm_amd
    plan = gfdm_amd.SpectrumMeter.plan_for
    for nfft in (16, 64, 4096):
        for hop in (1, 3, nfft // 2, nfft - 1, nfft):
            for n in (0, 1, nfft - 1, nfft, nfft + 1, nfft + hop - 1, nfft + hop, 5 * nfft + 7, 10 ** 12):
                n_seg, advance = plan(nfft, hop, n)
                assert (n_seg, advance) == R.plan(nfft, hop, n), (nfft, hop, n)
                assert advance == n_seg * hop
                if n_seg:
                    assert (n_seg - 1) * hop + nfft <= n < n_seg * hop + nfft
    # a stream cut by plan has the segments of the whole
    nfft, hop, n = 64, 24, 1000
    start, total = 0, 0
    for cut in (300, 511, n):                    # the calls see x[start:cut]
        s, adv = plan(nfft, hop, cut - start)
        total, start = total + s, start + adv
    assert total == R.segments_of(nfft, hop, n)
    L = gfdm_amd.lib()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for nfft, hop, n in ((48, 8, 100), (64, 0, 100), (64, 65, 100), (64, 32, -1), (64, 32, 2 ** 61 + 1)):
        assert L.gfdm_hip_spectrum_meter_plan(nfft, hop, n, ctypes.byref(a), ctypes.byref(b)) == EINVAL
    assert L.gfdm_hip_spectrum_meter_plan(64, 32, 2 ** 61, None, None) == 0


def test_windows():
    import gfdm_amd
    for nfft in (16, 256):
        assert np.array_equal(gfdm_amd.spectrum_window("rect", nfft), np.ones(nfft, np.float32))
        hann = gfdm_amd.spectrum_window("hann", nfft)
        assert hann.dtype == np.float32 and np.array_equal(hann, R.hann(nfft))
        assert hann[0] == 0 and hann[nfft // 2] == 1 and np.allclose(hann[1:], hann[1:][::-1], rtol=0, atol=1e-7)  # periodic: symmetric about nfft / 2
        bh = gfdm_amd.spectrum_window("blackmanharris", nfft)
        assert abs(bh[0] - 6e-5) < 1e-6 and bh[nfft // 2] == pytest.approx(1.0, abs=1e-6) and np.all(bh > 0)
        ft = gfdm_amd.spectrum_window("flattop", nfft)
        assert ft[nfft // 2] == pytest.approx(1.0, abs=1e-6) and ft.min() < 0                                  # the flat top has negative lobes
        # a cosine-sum window's transform is its coefficients: a_0 at DC, a_i / 2 at +-i
        for name, coeff in gfdm_amd.capi.SPECTRUM_WINDOWS.items():
            W = np.fft.fft(gfdm_amd.spectrum_window(name, nfft).astype(np.float64)) / nfft
            want = np.zeros(nfft)
            for i, a in enumerate(coeff):
                if i == 0:
                    want[0] = a
                else:
                    want[i] = want[-i] = (-1) ** i * a / 2
            assert np.allclose(W.real, want, rtol=0, atol=1e-7) and np.allclose(W.imag, 0, rtol=0, atol=1e-7), name
    with pytest.raises(ValueError):
        gfdm_amd.spectrum_window("kaiser", 16)


def test_subcarrier_power_and_oob_ratio():
    import gfdm_amd
    nfft, K = 256, 64
    P = np.zeros(nfft)
    P[4 * 5 - 2:4 * 5 + 2] = 1.0                 # the four bins of subcarrier 5: [18, 22)
    P[254:] = 3.0                                # subcarrier 0 wraps: [-2, 2)
    P[0:2] = 3.0
    sc = gfdm_amd.subcarrier_power(P, K)
    assert sc.shape == (K,) and sc[5] == 4.0 and sc[0] == 12.0 and sc.sum() == P.sum() and np.count_nonzero(sc) == 2
    P[4 * 6 - 2] = 0.5                           # the first bin of subcarrier 6
    assert gfdm_amd.subcarrier_power(P, K)[6] == 0.5
    assert gfdm_amd.oob_ratio_db(P, K, [0, 5]) == pytest.approx(10 * math.log10(0.5 / 16.0))
    assert gfdm_amd.oob_ratio_db(P, K, [0, 5, 6]) == -math.inf
    assert math.isnan(gfdm_amd.oob_ratio_db(P, K, []))
    assert gfdm_amd.oob_ratio_db(P, K, [-64, 5 + 64]) == gfdm_amd.oob_ratio_db(P, K, [0, 5])               # the map is cyclic
    assert np.array_equal(gfdm_amd.subcarrier_power(np.arange(8.0), 8), np.arange(8.0))                     # one bin a subcarrier
    with pytest.raises(ValueError):
        gfdm_amd.subcarrier_power(np.ones(100), 64)


# ---- the restatement against known answers ----
def test_impulse_with_a_rectangular_window_is_flat():
    for nfft in (16, 256):
        for n0 in (0, 1, nfft - 1):
            x = np.zeros(nfft, np.complex64)
            x[n0] = 1.0
            r = R.psd(x, np.ones(nfft, np.float32), [0])
            assert r["segments"] == 1 and np.allclose(r["psd_sum"], 1.0, rtol=0, atol=1e-12)


def test_tone_on_a_bin():
    nfft, b, A = 64, 5, 0.75
    x = (A * np.exp(2j * np.pi * b * np.arange(3 * nfft) / nfft)).astype(np.complex64)
    r = R.psd(x, np.ones(nfft, np.float32), R.stream_origins(nfft, nfft, x.size))
    assert r["segments"] == 3
    assert r["psd_sum"][b] == pytest.approx(3 * A * A * nfft * nfft, rel=1e-6)
    assert np.delete(r["psd_sum"], b).max() < 1e-9 * r["psd_sum"][b]
    assert R.budget_share(r["psd_sum"], r) == 0.0 and np.all(r["budget"] > 0)


def test_parseval():
    """sum_k |X_s[k]|^2 = nfft sum_n |x_n w_n|^2: the bins of psd_sum / (segments nfft sum w^2) add up to the mean power of a stationary input"""
    nfft, hop = 128, 64
    x = R.gaussian_with_tone(40 * nfft, 1, nfft)
    w = R.hann(nfft)
    o = R.stream_origins(nfft, hop, x.size)
    r = R.psd(x, w, o)
    f = x[o[:, None] + np.arange(nfft)[None, :]].astype(np.complex128) * w.astype(np.float64)
    assert r["psd_sum"].sum() == pytest.approx(nfft * (np.abs(f) ** 2).sum(), rel=1e-12)
    P = r["psd_sum"] / (r["segments"] * nfft * float((w.astype(np.float64) ** 2).sum()))
    assert P.sum() == pytest.approx(float(np.mean(np.abs(x.astype(np.complex128)) ** 2)), rel=0.05)


def test_white_noise_is_flat_within_five_sigma():
    """white complex Gaussian noise of power s^2 through a rectangular window: |X[k]|^2 / nfft is exponential with mean s^2, so the mean of
    S independent segments has the standard deviation s^2 / sqrt(S); psd() then reads s^2 / nfft per bin.  5 sigma over 64 bins: a
    false alarm of 64 * 5.7e-7."""
    nfft, S, s2 = 64, 4000, 2.5
    rng = np.random.default_rng([R.SEED, 5])
    x = (math.sqrt(s2 / 2) * (rng.standard_normal(S * nfft) + 1j * rng.standard_normal(S * nfft))).astype(np.complex64)
    r = R.psd(x, np.ones(nfft, np.float32), R.stream_origins(nfft, nfft, x.size))
    P = r["psd_sum"] / (S * nfft * nfft)
    assert np.all(np.abs(P - s2 / nfft) <= 5 * (s2 / nfft) / math.sqrt(S))


def test_non_finite_segments_and_burst_origins():
    nfft = 16
    x = R.gaussian_with_tone(5 * nfft, 2, nfft)
    x[2 * nfft + 3] = np.nan
    o = R.stream_origins(nfft, nfft, x.size)
    r = R.psd(x, R.hann(nfft), o)
    assert (r["segments"], r["bad_segments"]) == (4, 1)
    clean = R.psd(x, R.hann(nfft), np.delete(o, 2))
    assert np.array_equal(r["psd_sum"], clean["psd_sum"])
    starts = np.array([40, -1, 0, 70, 90], np.int64)
    got = R.burst_origins(starts, None, -4, 2, 8, nfft, 100)
    assert got.tolist() == [36, 44, 4, 66, 74]                         # -1 skipped; 0 - 4 < 0 is out, 0 - 4 + 8 is live; 86 + 16 > 100 is out
    got = R.burst_origins(starts, None, 0, 2, 8, nfft, 100)
    assert got.tolist() == [40, 48, 0, 8, 70, 78]                      # 90 + 16 > 100: both segments of the last burst are out
    assert R.burst_origins(starts, 1, 0, 2, 8, nfft, 100).tolist() == [40, 48] and R.burst_origins(starts, -3, 0, 2, 8, nfft, 100).size == 0
    assert R.burst_origins(starts, 99, 0, 2, 8, nfft, 100).size == 6


def test_the_bin_rule_at_its_edges():
    f32 = np.float32
    p = np.array([2.0 ** -32, 1.0, 1.125, 2.0 ** 32, 0.0, 1e-40, np.nextafter(f32(2.0 ** -32), f32(0)), np.nextafter(f32(1.125), f32(0)), 2.0 ** 31.9, 3e38], f32)
    assert R.bin_of(p).tolist() == [0, 256, 257, 511, 0, 0, 0, 256, 510, 511]
    assert R.bin_of(np.array([2.0 ** -31.99, 2.0 ** 32 * 0.99], f32)).tolist() == [0, 511]                 # bin 511 begins at 1.875 * 2^31
    edges = R.hist_edges()
    assert edges[0] == 2.0 ** -32 and edges[256] == 1.0 and edges[257] == 1.125 and edges[511] == 1.875 * 2.0 ** 31
    assert np.array_equal(R.bin_of(edges.astype(f32)), np.arange(512)) and np.array_equal(R.bin_of(np.nextafter(edges[1:].astype(f32), f32(0))), np.arange(511))
    x = np.array([1.0, complex(np.inf, 0), complex(0, np.nan), 3e19 + 3e19j, 0.0, 1e-22, 2.0 ** -16, 0.75 + 0.75j], np.complex64)
    r = R.power(x)
    assert (r["samples"], r["bad_samples"]) == (5, 3)                  # inf, nan and the overflow count in bad_samples and nowhere else
    assert r["hist"].sum() == 5 and r["hist"][0] == 3 and r["hist"][256] == 1 and r["hist"][257] == 1          # |0.75 + 0.75j|^2 = 1.125
    assert r["peak_bits"] == int(np.array([1.125], f32).view(np.uint32)[0])
    assert r["power_sum"] == pytest.approx(1.0 + 1.125 + 2.0 ** -32, rel=1e-15) and r["tiles"] == 1
    # the two roundings of the contract, not a fused one: re^2 + im^2 with both products rounded first
    z = np.array([complex(1 + 2.0 ** -12, 1 + 2.0 ** -13)], np.complex64)
    re, im = f32(z.real[0]), f32(z.imag[0])
    assert R.sample_power(z)[0] == f32(f32(re * re) + f32(im * im))


def test_the_yardstick_has_an_error_of_its_own():
    """random Gaussian inputs with a tone: numpy's complex64 pipeline misses the float64 reference by about 2^-24 of its norm, and uses a
    small share of the derived budget -- the budget catches wrong indices and twiddles, the yardstick lost bits"""
    for nfft in (16, 256, 4096):
        x = R.gaussian_with_tone(2 * nfft, nfft, nfft)
        r = R.psd(x, R.hann(nfft), R.stream_origins(nfft, nfft // 2, x.size))
        assert 0.2 <= r["numpy_error"] / (2.0 ** -24 * r["norm"]) <= 3.0
        wrong = np.roll(r["psd_sum"], 1)
        assert R.budget_share(wrong, r) > 1.0 and R.yardstick_ratio(wrong, r) > 100.0
        assert R.yardstick_ratio(r["psd_sum"], r) == 0.0
