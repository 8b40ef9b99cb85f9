"""CPU-side checks of the burst detector (gfdm_hip_burst_sync_detect, find_frame_start_at): the float64 restatement of the contract
(tests/burst_detect_ref.py) against the pygfdm fixtures of tests/golden/detect (make_golden_detect.py), threshold_factor, the new
entry points' binding and the detector's argument table, which needs neither a handle nor a device."""
import numpy as np
import pytest

from burst_detect_ref import detect_names, load_detect, ref_detect, ref_peaks


def test_detect_fixtures_cover_the_cases():
    names = detect_names()
    gs = [load_detect(n) for n in names]
    assert {g["K"] for g in gs} >= {32, 64, 128, 256}
    assert any(g["core_starts"].size == 0 for g in gs)                                          # noise only
    assert any(g["starts"].size and g["starts"][-1] == g["stream"].size - g["window_len"] for g in gs)      # a window clamped to the stream end
    for g in gs:
        assert g["stream"].dtype == np.complex64 and float(g["threshold_margin"]) >= 1e-3
        gaps = np.diff(g["core_starts"])
        if gaps.size:
            burst = 2 * g["min_distance"]
            assert gaps.min() == burst and gaps.max() > 2 * burst                               # back to back, and a long pause


@pytest.mark.parametrize("name", detect_names())
def test_restatement_matches_pygfdm(name):
    g = load_detect(name)
    K, cp, W, R, lead = g["K"], g["cp_len"], g["window_len"], g["min_distance"], g["lead"]
    r = ref_detect(g["stream"], g["preamble"], K, cp, W, g["threshold"], R, lead)
    assert np.array_equal(r["peaks"], g["peaks"])                       # the stored detections (pygfdm's ic, the contract's peak rule)
    assert np.array_equal(r["starts"], g["starts"])
    assert np.array_equal(r["coarse"], r["peaks"])                      # the window's argmax is the peak it was cut around
    assert np.array_equal(r["frame_start"], g["starts"] + g["nc"])      # pygfdm's nc, as a stream index ...
    assert np.array_equal(r["frame_start"], g["core_starts"])           # ... which is the true core start
    if r["peaks"].size:
        assert np.max(np.abs(r["cfo"] - g["cfo"])) < 1e-9
        assert np.max(np.abs(r["metric"] - g["metric"])) < 1e-9
        assert np.max(np.abs(r["peaks"] - g["core_starts"])) <= cp // 4
    else:
        assert r["ic"].max() < g["threshold"]


def test_peak_rule_ties_and_ends():
    """first index of equal values wins, on either side; ranges are cut at the ends (a check of the reference the GPU tests compare with;
    the device's handling of ties is tests/test_burst_detect_gpu.py::test_equal_values_first_index_wins)"""
    ic = np.array([0.5, 0.9, 0.9, 0.1, 0.9, 0.2, 0.2, 0.95, 0.3])
    assert list(ref_peaks(ic, 0.4, 2)) == [1, 7]          # 2 loses to 1 (equal, earlier), 4 loses to 2 (equal within R before)
    assert list(ref_peaks(ic, 0.4, 1)) == [1, 4, 7]
    assert list(ref_peaks(ic, 0.4, 0)) == [0, 1, 2, 4, 7]
    assert list(ref_peaks(ic, 0.4, 100)) == [7]
    assert list(ref_peaks(np.zeros(5), 0.4, 2)) == []
    rng = np.random.default_rng(0)                         # the blocked sliding maximum against the rule written out
    for _ in range(200):
        P, Rr = int(rng.integers(1, 80)), int(rng.integers(0, 30))
        v = np.round(rng.random(P) * 6) / 6
        brute = [i for i in range(P) if v[i] >= 0.3 and all(v[j] < v[i] for j in range(max(0, i - Rr), i))
                 and all(v[j] <= v[i] for j in range(i + 1, min(P, i + Rr + 1)))]
        assert list(ref_peaks(v, 0.3, Rr)) == brute


def test_threshold_factor():
    import gfdm_amd
    for p in (1e-6, 1e-3, 0.01, 0.5, 0.999):
        assert gfdm_amd.threshold_factor(p) == pytest.approx(np.sqrt(-(4 / np.pi) * np.log(p)), rel=1e-15)
    assert gfdm_amd.threshold_factor(0.01) == pytest.approx(2.4215, abs=1e-4)
    for p in (1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="smaller 1.0"):
            gfdm_amd.threshold_factor(p)


def test_detect_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.exported_symbols())
    for stem in ("find_frame_start_at", "detect"):
        for kind in ("host", "device"):
            assert "gfdm_hip_burst_sync_%s_%s" % (stem, kind) in names
    assert {"gfdm_hip_burst_sync_detect_workspace_bytes", "gfdm_hip_burst_sync_detect_check"} <= names
    assert hasattr(gfdm_amd.BurstSync, "detect") and hasattr(gfdm_amd.BurstSync, "find_frame_start_at")


# K = 64, cp_len = 32, W = 288: P_w = W - 2K = 160
@pytest.mark.parametrize("stream_len,threshold,R,lead,max_bursts,match", [
    (10000, 0.45, 256, 31, 10, "lead"),                    # lead < cp_len
    (10000, 0.45, 256, 257, 10, "lead"),                   # lead > min_distance
    (10000, 0.45, 94, 64, 10, "min_distance"),             # W - 2K - lead - 1 = 95 > R
    (10000, 0.0, 256, 64, 10, "threshold"),
    (10000, -0.1, 256, 64, 10, "threshold"),
    (10000, float("nan"), 256, 64, 10, "threshold"),
    (10000, 0.45, 256, 64, -1, "max_bursts"),
    (1 << 20, 0.45, (1 << 16) + 1, 64, 10, "min_distance"),   # the scan's halo grows with it
    (287, 0.45, 256, 64, 10, "stream_len"),                # stream_len < W
    ((1 << 29) + 1, 0.45, 256, 64, 10, "stream_len"),      # beyond the scan's 32-bit positions
])
def test_detect_argument_table(stream_len, threshold, R, lead, max_bursts, match):
    """every row is EINVAL whatever the machine: the table is checked before a device is touched"""
    import gfdm_amd
    L = gfdm_amd.lib()
    assert L.gfdm_hip_burst_sync_detect_check(64, 32, 288, stream_len, threshold, R, lead, max_bursts) == gfdm_amd.capi.EINVAL
    assert match in L.gfdm_hip_last_error().decode()


def test_detect_argument_table_accepts_the_bounds():
    import gfdm_amd
    L = gfdm_amd.lib()
    ok = gfdm_amd.capi.OK
    assert L.gfdm_hip_burst_sync_detect_check(64, 32, 288, 288, 1e-6, 95, 64, 0) == ok          # W - 2K - lead - 1 == R, stream_len == W
    assert L.gfdm_hip_burst_sync_detect_check(64, 32, 288, 1 << 29, 0.45, 127, 32, 1) == ok     # lead == cp_len: 160 - 32 - 1 == 127
    assert L.gfdm_hip_burst_sync_detect_check(64, 32, 288, 10000, 0.45, 128, 128, 1) == ok      # lead == min_distance
    assert L.gfdm_hip_burst_sync_detect_check(64, 32, 288, 1 << 20, 0.45, 1 << 16, 64, 1) == ok    # the largest min_distance


def test_detect_needs_a_handle():
    import gfdm_amd
    L = gfdm_amd.lib()
    E = gfdm_amd.capi.EINVAL
    assert L.gfdm_hip_burst_sync_detect_workspace_bytes(None, 10000) == E
    assert L.gfdm_hip_burst_sync_detect_host(None, None, None, None, None, None, None, None, 10000, 0.45, 256, 64, 4) == E
    assert L.gfdm_hip_burst_sync_detect_device(None, None, None, None, None, None, None, None, 10000, 0.45, 256, 64, 4, None, None) == E
    assert L.gfdm_hip_burst_sync_find_frame_start_at_host(None, None, None, None, None, None, None, 10000, None, 1) == E
    assert L.gfdm_hip_burst_sync_find_frame_start_at_device(None, None, None, None, None, None, None, 10000, None, 1, None) == E
