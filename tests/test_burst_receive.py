"""CPU-side checks of demodulate_bursts (the receivers that read detected bursts straight from the capture): the four entry points are
exported and bound, the kernels of the new part build through hiprtc, and the float64 restatement the GPU tests compare with meets
their precondition (every decided symbol clear of the QPSK decision boundaries) on the inputs they use."""
import os

import numpy as np
import pytest

from burst_receive_cases import CASES, MARGIN, make_case, restatement, virtual_bursts


def test_burst_receive_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.exported_symbols())
    for stem in ("gfdm_hip_receiver_demodulate_bursts", "gfdm_hip_advanced_receiver_work_bursts"):
        for kind in ("host", "device"):
            assert "%s_%s" % (stem, kind) in names
            assert hasattr(gfdm_amd.lib(), "%s_%s" % (stem, kind))
    assert callable(gfdm_amd.Demodulator.demodulate_bursts) and callable(gfdm_amd.AdvancedReceiver.demodulate_bursts)


def test_burst_receive_part_builds_through_hiprtc(tmp_path, monkeypatch):
    """part bit 5 of gfdm_hip_precompile: the gather-load receive kernels of a run-time shape compile from the embedded headers
    (the shared fetch among them) without a GPU, into a cache file of their own"""
    import gfdm_amd
    monkeypatch.setenv("GFDM_HIP_CACHE_DIR", str(tmp_path))
    gfdm_amd.precompile(3, 48, 2, 32)
    files = sorted(os.listdir(tmp_path))
    assert [f for f in files if f.endswith(".hsaco")] and all("_p5_" in f for f in files), files
    names = open(os.path.join(tmp_path, [f for f in files if f.endswith(".names")][0])).read()
    assert names.count("k_row_receive_burst") == 4                     # FD, demodulate, two kinds of vector-ALU rounds (no matrix-core rounds at K = 48)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_meets_the_precondition(name):
    """(C) for the seeds chosen: in (B) every active symbol of every cancellation round lies further than MARGIN from a decision
    boundary, so no round of the GPU's float32 hangs on rounding; and (B) recovers the transmitted symbols."""
    M, K, L, A, nb, seed = CASES[name]
    c = make_case(M, K, L, A, nb, seed)
    e = virtual_bursts(c["stream"], c["starts"], c["sc_rot"], 0, c["F"])
    out, margin = restatement(c, e, 2)
    print(name, "margin", margin)
    assert margin > MARGIN
    assert np.array_equal(out.real > 0, c["sym"].real > 0) and np.array_equal(out.imag > 0, c["sym"].imag > 0)
