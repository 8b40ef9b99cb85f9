"""CPU-side checks of the burst synchroniser and extractor handles (gfdm_hip_burst_sync, gfdm_hip_burst_extractor): the entry points
are bound, constructor arguments are validated before any device is touched, and without a GPU creation answers ENODEV."""
import numpy as np
import pytest

from conftest import have_gpu


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
