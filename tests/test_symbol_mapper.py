"""CPU-side tests of the symbol mapper (contract in include/gfdm_hip.h, gfdm_hip_symbol_mapper): the exports and the argument table of the
library, the numpy restatement of tests/symbol_mapper_ref.py against pygfdm's own bits2symbols / symbols2bits (tests/golden/symbols), and
the preconditions of tests/test_symbol_mapper_gpu.py on the restatement alone."""
import ctypes
import glob
import os

import numpy as np
import pytest

import symbol_mapper_ref as S
from conftest import GOLDEN_DIR, have_gpu

ENTRY_POINTS = ("create", "destroy", "bits_per_symbol", "n_points", "decision", "points", "row_bytes", "check",
                "map_host", "map_device", "decode_host", "decode_device", "soft_host", "soft_device")
I64_MAX = 2 ** 63 - 1


def test_every_entry_point_is_exported_and_bound():
    import gfdm_amd
    lib = ctypes.CDLL(gfdm_amd.capi.LIB_PATH)
    bound = set(gfdm_amd.exported_symbols())
    for n in ENTRY_POINTS:
        name = "gfdm_hip_symbol_mapper_" + n
        assert hasattr(lib, name), "libgfdm_hip.so does not export %s" % name
        assert name in bound, "%s is missing from the ctypes table" % name
    assert sorted(n for n in bound if n.startswith("gfdm_hip_symbol_mapper_")) == sorted("gfdm_hip_symbol_mapper_" + n for n in ENTRY_POINTS)
    for name in ("bits_per_symbol", "points", "decision_rule", "row_bytes", "map", "decode", "soft"):
        assert callable(getattr(gfdm_amd.SymbolMapper, name))
    assert (gfdm_amd.DECIDE_AUTO, gfdm_amd.DECIDE_NEAREST, gfdm_amd.DECIDE_QPSK, gfdm_amd.DECIDE_BPSK) == ("auto", "nearest", "qpsk", "bpsk")


def test_check_table_answers_without_a_device():
    import gfdm_amd
    L = gfdm_amd.lib()
    check = L.gfdm_hip_symbol_mapper_check
    EINVAL = gfdm_amd.capi.EINVAL
    for n_points in (2, 4, 8, 16, 32, 64, 128, 256):
        assert check(n_points, 1, 0) == 0 and check(n_points, 4097, 7) == 0 and check(n_points, 1, 1 << 40) == 0
    for n_points in (-4, 0, 1, 3, 6, 12, 255, 257, 512, 4096):
        assert check(n_points, 8, 1) == EINVAL
    assert b"points" in L.gfdm_hip_last_error()
    assert check(4, 0, 1) == EINVAL and check(4, -1, 1) == EINVAL and b"n_sym" in L.gfdm_hip_last_error()
    assert check(4, 1, -1) == EINVAL and b"n_rows" in L.gfdm_hip_last_error()
    # byte sizes: 8 n_rows n_sym for the symbols, 4 k n_rows n_sym for the soft bits (the larger one from k = 3 on)
    assert check(4, I64_MAX // 8, 1) == 0 and check(4, I64_MAX // 8 + 1, 1) == EINVAL and b"overflows" in L.gfdm_hip_last_error()
    assert check(4, 1 << 30, 1 << 29) == 0 and check(4, 1 << 30, 1 << 30) == EINVAL
    assert check(256, I64_MAX // 32, 1) == 0 and check(256, I64_MAX // 32 + 1, 1) == EINVAL and check(256, I64_MAX // 8, 1) == EINVAL
    assert check(256, 1 << 29, 1 << 28) == 0 and check(256, 1 << 29, 1 << 29) == EINVAL
    assert check(4, I64_MAX, 0) == EINVAL                                   # a row alone overflows, whatever n_rows is
    # create answers from the same table before it looks for a device; a NULL handle is EINVAL in every call
    h = ctypes.c_void_p()
    pts = np.zeros(8, np.complex64)
    create = L.gfdm_hip_symbol_mapper_create
    assert create(ctypes.byref(h), pts.ctypes.data, 3, -1, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 512, -1, 0) == EINVAL
    assert create(ctypes.byref(h), None, 4, -1, 0) == EINVAL and create(None, pts.ctypes.data, 4, -1, 0) == EINVAL
    assert create(ctypes.byref(h), pts.ctypes.data, 4, 3, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 4, -2, 0) == EINVAL
    assert create(ctypes.byref(h), pts.ctypes.data, 8, 1, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 4, 2, 0) == EINVAL      # QPSK over 8, BPSK over 4
    assert b"does not match" in L.gfdm_hip_last_error() and not h.value
    buf = np.zeros(16, np.uint8)
    assert L.gfdm_hip_symbol_mapper_decode_host(None, buf.ctypes.data, buf.ctypes.data, None, 1, 1) == EINVAL
    assert L.gfdm_hip_symbol_mapper_map_device(None, buf.ctypes.data, buf.ctypes.data, None, 1, 1, None) == EINVAL
    assert L.gfdm_hip_symbol_mapper_soft_host(None, buf.ctypes.data, buf.ctypes.data, None, None, 1, 1) == EINVAL
    assert L.gfdm_hip_symbol_mapper_row_bytes(None, 8) == EINVAL and L.gfdm_hip_symbol_mapper_bits_per_symbol(None) == EINVAL
    if not have_gpu():
        with pytest.raises(gfdm_amd.GfdmHipError) as e:                     # no CPU path: a valid constellation needs a device
            gfdm_amd.SymbolMapper(S.constellations()["gr_qpsk"][0])
        assert e.value.status == gfdm_amd.capi.ENODEV
    with pytest.raises(ValueError):
        gfdm_amd.SymbolMapper(np.ones(3))


def _fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "symbols", "*.npz")))


def test_fixtures_are_present():
    assert len(_fixtures()) >= 3
    assert {int(np.load(f)["k"]) for f in _fixtures()} == {1, 2}


@pytest.mark.parametrize("path", _fixtures(), ids=lambda p: os.path.splitext(os.path.basename(p))[0])
def test_restatement_equals_pygfdm(path):
    """bits2symbols / symbols2bits of pygfdm, row by row, against pack -> map and decode -> unpack of the restatement: exactly"""
    g = np.load(path)
    k, bits, points = int(g["k"]), g["bits"], g["points"].astype(np.complex64)
    n_rows, n_sym = g["symbols"].shape
    data = np.packbits(bits, axis=1)                                         # MSB first, every row starting on a byte, spare bits 0
    assert data.shape == (n_rows, S.row_bytes(n_sym, k)) and (n_sym * k) % 8
    assert np.array_equal(S.pack(S.unpack(data, n_sym, k), k), data)
    assert np.array_equal(S.map(data, n_sym, points), g["symbols"])
    for rule in ("nearest",):                                                # pygfdm's point order is not GNU Radio's: no sign tests
        got, margin = S.decode(g["noisy"], points, rule)
        assert np.array_equal(np.unpackbits(got, axis=1)[:, :n_sym * k], g["rx_bits"])
        assert np.array_equal(got & ~S.spare_mask(n_sym, k), np.zeros_like(got))
        assert margin.min() > 1e-3
    assert np.any(g["rx_bits"] != bits) or n_sym < 100                       # the noise does turn decisions
    # the hard decision is the sign of the max-log value: positive means bit 0
    llr, d0, d1 = S.soft(g["noisy"], points)
    assert np.array_equal(llr < 0, g["rx_bits"].astype(bool)) and np.all(np.minimum(d0, d1) >= 0)


@pytest.mark.parametrize("name", sorted(S.constellations()))
def test_decode_of_map_is_the_identity(name):
    points, rule = S.constellations()[name]
    k = S.bits_per_symbol(points)
    rng = np.random.default_rng(k)
    for n_sym in S.N_SYMS[:9]:
        for n_rows in S.N_ROWS:
            data = rng.integers(0, 256, (n_rows, S.row_bytes(n_sym, k)), dtype=np.uint8)
            mask = S.spare_mask(n_sym, k)
            sym = S.map(data, n_sym, points)
            assert sym.dtype == np.complex64 and sym.shape == (n_rows, n_sym)
            back, margin = S.decode(sym, points, rule)
            assert np.array_equal(back, data & mask)
            if rule == "nearest":
                assert margin.min() > 0.05
            for count in (0, 3, n_rows + 5, -1):
                n = S.live(count, n_rows)
                assert not S.map(data, n_sym, points, count)[n:].any() and np.array_equal(S.map(data, n_sym, points, count)[:n], sym[:n])
                assert np.array_equal(S.decode(sym, points, rule, count)[0][:n], back[:n]) and not S.decode(sym, points, rule, count)[0][n:].any()
    assert S.pack(np.array([[(1 << k) - 1, 0, 1]]), k).tolist() == {1: [[0b10100000]], 2: [[0b11000100]], 3: [[0b11100000, 0b10000000]],
                                                                     4: [[0xF0, 0x10]], 6: [[0xFC, 0x00, 0x40]], 8: [[0xFF, 0x00, 0x01]]}[k]


def test_rules_of_the_constellations():
    """what AUTO must resolve to follows from the points: GNU Radio's unit QPSK / BPSK take the sign tests and these agree with the nearest
    point wherever the margin is positive"""
    c = S.constellations()
    assert [c[n][1] for n in ("gr_bpsk", "gr_qpsk", "pygfdm_qpsk")] == ["bpsk", "qpsk", "nearest"]
    assert sorted(S.bits_per_symbol(p) for p, _ in c.values()) == [1, 2, 2, 3, 4, 4, 6, 8]
    for name in ("gr_bpsk", "gr_qpsk"):
        x = S.case(name, 7, 257)["x"]
        assert np.array_equal(S.indices(x, c[name][0], c[name][1]), S.indices(x, c[name][0], "nearest"))


def _f32_distances(x, p, fused):
    """d_i as float32 arithmetic gives it: differences rounded, then dr dr + di di either with every operation rounded or with the second
    product fused into the sum (fma(dr, dr, di di), evaluated in float64: exact for float32 operands up to the final rounding)"""
    xr, xi = x.real.astype(np.float32)[:, None], x.imag.astype(np.float32)[:, None]
    dr, di = (xr - p.real.astype(np.float32)), (xi - p.imag.astype(np.float32))
    if fused:
        return (dr.astype(np.float64) * dr + (di * di).astype(np.float64)).astype(np.float32)
    return dr * dr + di * di


def test_preconditions_of_the_gpu_tests():
    c = S.constellations()
    # the guard leaves out at most 0.1 % of every case, on the restatement alone
    for name, (points, rule) in c.items():
        if rule != "nearest":
            continue
        for n_rows, n_sym in S.shapes() + (list(S.MANY_ROWS) if name in S.MANY_ROWS_NAMES else []):
            k = S.case(name, n_rows, n_sym)
            _, margin = S.decode(k["x"], points, rule)
            out = np.count_nonzero(~S.guarded(k["x"], margin))
            assert out <= S.GUARD_CAP * n_rows * n_sym, (name, n_rows, n_sym, out)
    # every exact-tie input really ties in float32, fused or not, and the first index among the tied ones is the known answer
    x, want = S.tie_inputs()
    grid = c["qam16_grid"][0]
    assert np.array_equal(S.indices(x, grid, "nearest"), want)
    for fused in (False, True):
        d = _f32_distances(x, grid, fused)
        tied = d == d.min(axis=1, keepdims=True)
        assert np.all(tied.sum(axis=1) >= 2) and np.array_equal(np.argmax(tied, axis=1), want)
        assert np.array_equal(d, S._dist(x, grid))                          # integers: float32 is exact here
    assert np.all(S.decode(x[None, :], grid, "nearest")[1] == 0)
    # the known answers for NaN, infinities and zeros are the contract's formulas
    sx, qpsk, bpsk, nearest = S.special_inputs()
    assert np.array_equal(S.indices(sx, c["gr_qpsk"][0], "qpsk"), qpsk) and np.array_equal(S.indices(sx, c["gr_bpsk"][0], "bpsk"), bpsk)
    for name, (points, _) in c.items():
        assert np.array_equal(S.indices(sx[:nearest.size], points, "nearest"), nearest), name
        assert not np.isfinite(sx[:nearest.size]).any() and np.isfinite(sx[nearest.size:]).all()
    # the soft bound is positive wherever it is used and scales with |s_r|
    k = S.case("qam16", 7, 65)
    _, d0, d1 = S.soft(k["x"], k["points"], k["scale"])
    assert np.all(S.soft_bound(k["scale"], d0, d1) > 0)
