"""The spectrum meter past its bounded grids, as tests/test_fading_grid_bound_gpu.py does it for the fading model: k_spectrum_psd launches
at most G = 1024 workgroups, each owning a contiguous run of trips (a trip: 4096 / nfft segments side by side), and the other GPU tests
stay far below G trips, so a workgroup's second and third trip -- the LDS tile and the flags reused behind a barrier, the fp64 bins kept
over the run, segment numbers of G trips and above, the ragged last run -- run here and nowhere else; likewise k_spectrum_power's run of
tiles.  One complex64 case (nfft 16, hop 16) and one sc16 case (nfft 256, hop 128) of 2 G + 3 trips less a ragged remainder
(tests/spectrum_meter_ref.py, held to the kernels' constants by tests/test_spectrum_meter.py), and 2 G + 3 tiles of the power pass:
  1. against the restatement: the budget and the yardstick for psd_sum, the integers exactly, power_sum under its bound;
  2. against the same handle called in three pieces that each stay below G trips: the integers equal, psd_sum within 2^-40;
  3. canaries on both sides of the input, which is unchanged."""
import gc

import numpy as np
import pytest

import grid_bound_cases as G
import spectrum_meter_ref as R
from conftest import have_gpu
from spectrum_gpu_common import INT, Guarded
from spectrum_gpu_common import check_psd as _check_psd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@pytest.fixture(autouse=True)
def _give_the_memory_back():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", R.GRID_CASES, ids=G.case_id)
def test_spectrum_meter(case):
    import gfdm_amd
    geo = R.grid_geometry(case)
    nfft, hop, n = case["nfft"], case["hop"], geo["n"]
    x = R.sc16_capture(n, case["seed"], nfft) if case["sc16"] else R.gaussian_with_tone(n, case["seed"], nfft)
    g = Guarded(x, 1)
    sm = gfdm_amd.SpectrumMeter(nfft, hop=hop)
    assert sm.plan(n)[0] == geo["n_seg"]
    assert sm.update(g.view) == geo["n_seg"] * hop
    t = sm.read()
    # 1.
    r = R.psd(R.widen(x) if case["sc16"] else x, sm.window(), R.stream_origins(nfft, hop, n))
    assert r["segments"] == geo["n_seg"]
    _check_psd(t, r, "past the bounded grid, %s" % case["id"])
    # 2. three pieces cut at segment boundaries, each below G trips
    again = gfdm_amd.SpectrumMeter(nfft, hop=hop)
    per = 2 if case["sc16"] else 1
    flat = g.view.reshape(-1) if case["sc16"] else g.view
    for a, b in G.pieces(geo["n_seg"]):
        end = n if b == geo["n_seg"] else (b - 1) * hop + nfft
        piece = flat[a * hop * per:end * per]
        assert again.update(piece) == (b - a) * hop
    u = again.read()
    assert all(t[k] == u[k] for k in INT)
    assert np.all(np.abs(t["psd_sum"] - u["psd_sum"]) <= 2.0 ** -40 * t["psd_sum"])
    # the power pass over 2 G + 3 tiles of the same samples, and in three pieces
    m = geo["power_n"]
    assert m <= n
    sm.power(flat[:m * per])
    p = sm.read()
    rp = R.power((R.widen(x) if case["sc16"] else x)[:m])
    assert rp["tiles"] == geo["power_tiles"]
    assert [p[k] for k in INT] == [geo["n_seg"], 0, rp["samples"], rp["bad_samples"], rp["peak_bits"]] and np.array_equal(p["hist"], rp["hist"])
    err, bound = abs(p["power_sum"] - rp["power_sum"]), R.power_bound(rp["tiles"], rp["power_sum"])
    print("spectrum accuracy: power_sum past the bounded grid, %s: |got - ref| = %.3g, bound %.3g" % (case["id"], err, bound))
    assert err <= bound
    assert np.array_equal(p["psd_sum"], t["psd_sum"])
    for a, b in G.pieces(m):
        again.power(flat[a * per:b * per])
    q = again.read()
    assert all(p[k] == q[k] for k in INT) and np.array_equal(p["hist"], q["hist"])
    assert abs(p["power_sum"] - q["power_sum"]) <= 2 * R.power_bound(rp["tiles"] + 3, rp["power_sum"])
    # 3.
    assert g.unchanged()
