"""CPU-side checks of the burst synchroniser and extractor handles (gfdm_hip_burst_sync, gfdm_hip_burst_extractor): the entry points
are bound, constructor arguments are validated before any device is touched, and without a GPU creation answers ENODEV; and the
float64 restatement of the synchroniser's contract, the expectation of the GPU tests, against every pygfdm fixture of tests/golden/sync."""
import numpy as np
import pytest

from burst_detect_ref import ref_ac_ic, ref_fine
from conftest import have_gpu
from test_burst_gpu import load_sync, sync_names


def _preamble(K):
    return np.tile(np.exp(2j * np.pi * np.arange(K) ** 2 / K), 2)


def test_burst_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.exported_symbols())
    for stem in ("find_frame_start", "auto_correlate"):
        for kind in ("host", "device"):
            assert "gfdm_hip_burst_sync_%s_%s" % (stem, kind) in names
            assert "gfdm_hip_burst_extractor_extract_%s" % kind in names
    assert {"gfdm_hip_burst_extractor_set_cfo_correction", "gfdm_hip_burst_extractor_get_cfo_correction"} <= names


@pytest.mark.parametrize("K,cp,n_pre,W,match", [
    (64, 32, 127, 600, "Preamble length"),                 # n_preamble != 2K
    (64, 32, 64, 600, "Preamble length"),
    (1, 0, 2, 600, "fft_len"),                             # K < 2
    (2048, 0, 4096, 9000, "fft_len"),                      # K > 1024
    (64, -1, 128, 600, "cp_len"),
    (64, 32, 128, 2 * 64 + 32, "window_len"),              # window_len < 2K + cp + 1
    (32, 0, 64, 64, "window_len"),
])
def test_burst_sync_argument_errors(K, cp, n_pre, W, match):
    """EINVAL (ValueError) whatever the machine: the arguments are checked before a device is looked for"""
    import gfdm_amd
    pre = np.resize(_preamble(max(K, 1)), n_pre)
    with pytest.raises(ValueError, match=match):
        gfdm_amd.BurstSync(K, cp, pre, W)


def test_burst_sync_smallest_window_is_accepted_or_needs_a_gpu():
    import gfdm_amd
    try:
        s = gfdm_amd.BurstSync(64, 32, _preamble(64), 2 * 64 + 32 + 1)
    except gfdm_amd.GfdmHipError as e:
        assert e.status == gfdm_amd.capi.ENODEV and not have_gpu()
        return
    assert s.corr_len() == 33 and s.window_len() == 161 and s.fft_len() == 64 and s.cp_len() == 32


def test_burst_extractor_argument_errors():
    import gfdm_amd
    for n in (0, -5):
        with pytest.raises(ValueError, match="burst_len"):
            gfdm_amd.BurstExtractor(n, 0)


def test_burst_handles_need_a_gpu():
    """no CPU fallback: valid arguments without a GPU answer GFDM_HIP_ENODEV"""
    if have_gpu():
        pytest.skip("a GPU is present")
    import gfdm_amd
    with pytest.raises(gfdm_amd.GfdmHipError) as e:
        gfdm_amd.BurstSync(64, 32, _preamble(64), 1600)
    assert e.value.status == gfdm_amd.capi.ENODEV
    with pytest.raises(gfdm_amd.GfdmHipError) as e:
        gfdm_amd.BurstExtractor(800, 32, True)
    assert e.value.status == gfdm_amd.capi.ENODEV


@pytest.mark.parametrize("name", sync_names())
def test_restatement_matches_pygfdm(name):
    """ref_ac_ic / ref_fine (and with them ref_sync, held to the same fixtures on the GPU) are pygfdm's auto_correlation_sync and
    find_frame_start at every fixture's shape: odd fft_len, cp_len = 0 and cp_len above 2 fft_len among them"""
    g = load_sync(name)
    K, cp = g["K"], g["cp_len"]
    win = g["stream"][g["first"]:g["first"] + g["window_len"]]
    ac, ic = ref_ac_ic(win, K, cp)
    assert ac.size == g["ac"].size == g["window_len"] - 2 * K
    assert np.max(np.abs(ac - g["ac"])) < 1e-12 and np.max(np.abs(ic - g["ic"])) < 1e-12
    f = ref_fine(win, g["preamble"], K, cp)
    assert f["nm"] == g["nm"] and f["nc"] == g["nc"] and abs(f["cfo"] - float(g["cfo"])) < 1e-12
    assert np.max(np.abs(f["score"] - g["napcc"])) < 1e-12
    if g["kind"] in ("burst", "tiled", "zeros"):
        assert g["nc"] == g["core_start"] - g["first"]
