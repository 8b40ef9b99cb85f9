#!/usr/bin/env python3
"""Known answers for gfdm_amd.awgn_noise_voltage from pygfdm's own noise sizing (python/pygfdm/utils.py): calculate_awgn_noise_variance
over seeded signals, SNRs and rates.  One fixture, awgn_variance.npz: per case the signal (complex64), snr_db, rate and the variance per
component that pygfdm returns; the channel model's noise_voltage for that case is sqrt(2 * variance).

The fixture lives in tests/golden/channel/: conftest.golden_names() globs the top level of tests/golden into the receiver tests.

Build container only (imports /root/reference/python/pygfdm); import notes as in make_golden.py / make_golden_snr.py.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import scipy.signal as signal

HERE = os.path.dirname(os.path.abspath(__file__))
np.complex = complex
sys.modules.setdefault("commpy", types.ModuleType("commpy"))
if not hasattr(signal, "gaussian"):
    signal.gaussian = signal.windows.gaussian
sys.path.insert(0, "/root/reference/python")

from pygfdm.utils import calculate_awgn_noise_variance       # noqa: E402

# n samples, amplitude, snr_db, rate
CASES = [(1, 1.0, 0.0, 1.0), (64, 1.0, 10.0, 1.0), (577, 0.5, 20.0, 1.0), (721, 3.0, -3.0, 0.5), (4096, 0.01, 35.5, 2.0)]


def main():
    out_dir = os.path.join(HERE, "channel")
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(2718)
    data = {"n_cases": len(CASES)}
    for i, (n, amp, snr_db, rate) in enumerate(CASES):
        x = (amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        data["signal_%d" % i] = x
        data["snr_db_%d" % i] = snr_db
        data["rate_%d" % i] = rate
        data["variance_%d" % i] = float(calculate_awgn_noise_variance(x.astype(np.complex128), snr_db, rate))
        print(i, n, snr_db, rate, data["variance_%d" % i])
    np.savez_compressed(os.path.join(out_dir, "awgn_variance.npz"), **data)


if __name__ == "__main__":
    main()
