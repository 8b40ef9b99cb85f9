#!/usr/bin/env python3
"""Known-answer vectors for the symbol mapper from pygfdm's own pair (python/pygfdm/symbolmapping.py): bits2symbols and symbols2bits over
pygfdm's constellations -- order 1: [1, -1], order 2: [1+1j, 1-1j, -1+1j, -1-1j] / sqrt 2.  Both orders differ from GNU Radio's, so a
handle built from these points runs the nearest-point rule.  Per fixture: rows of bits, bits2symbols of every row, the symbols plus
white Gaussian noise at SNR_DB (Es / N0, unit-energy symbols; drawn here from a seeded generator, rounded to complex64 as a receiver
delivers them), and symbols2bits of the noisy rows.  The row lengths are chosen so that a row does not end on a byte.

The fixtures live in tests/golden/symbols/: conftest.golden_names() globs the top level of tests/golden into the receiver tests.

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

from pygfdm.symbolmapping import bits2symbols, generate_constellation, symbols2bits       # noqa: E402

SNR_DB = 6.0
# name, constellation order, n_rows, n_sym
CASES = [
    ("sym_k1_r5_n13", 1, 5, 13),
    ("sym_k2_r4_n9", 2, 4, 9),
    ("sym_k2_r3_n467", 2, 3, 467),
]


def main():
    out_dir = os.path.join(HERE, "symbols")
    os.makedirs(out_dir, exist_ok=True)
    for name, k, n_rows, n_sym in CASES:
        rng = np.random.default_rng(sum(map(ord, name)))
        points = generate_constellation(k)
        bits = rng.integers(0, 2, (n_rows, n_sym * k)).astype(np.uint8)
        symbols = np.array([bits2symbols(b, points).ravel() for b in bits])        # (pack_bits keeps a column axis)
        sigma = np.sqrt(0.5 / 10.0 ** (SNR_DB / 10.0))                          # per component
        noisy = (symbols + sigma * (rng.standard_normal(symbols.shape) + 1j * rng.standard_normal(symbols.shape))).astype(np.complex64)
        rx_bits = np.array([symbols2bits(r, points) for r in noisy]).astype(np.uint8)
        # a decision that float32 points (as a handle takes them) could turn would make the fixture a coin toss: none is that close
        d = np.sort(np.abs(noisy[..., None] - points) ** 2, axis=-1)
        assert np.min(d[..., 1] - d[..., 0]) > 1e-4
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), k=k, snr_db=SNR_DB, points=points.astype(np.complex128), bits=bits,
                            symbols=symbols.astype(np.complex64), noisy=noisy, rx_bits=rx_bits)
        print(name, bits.shape, "bit errors at %.0f dB: %d" % (SNR_DB, int(np.sum(bits != rx_bits))))


if __name__ == "__main__":
    main()
