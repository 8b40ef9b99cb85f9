"""CPU-side tests of the link meter (contract in include/gfdm_hip.h, gfdm_hip_link_meter): the exports and the argument tables of the
library, the numpy restatement of tests/link_meter_ref.py against the symbol mapper's own restatement and against hand-written known
answers of the matching rule, and the preconditions of tests/test_link_meter_gpu.py on the restatement alone."""
import ctypes
import math

import numpy as np
import pytest

import link_meter_ref as M
import symbol_mapper_ref as S
from conftest import have_gpu

ENTRY_POINTS = ("create", "destroy", "bits_per_symbol", "n_points", "decision", "row_bytes", "totals_device", "reset", "totals",
                "match_workspace_bytes", "measure_workspace_bytes", "match_host", "match_device", "measure_host", "measure_device")


def test_every_entry_point_is_exported_bound_and_declared():
    import gfdm_amd
    from test_boundary import declared_functions
    lib = ctypes.CDLL(gfdm_amd.capi.LIB_PATH)
    bound, declared = set(gfdm_amd.exported_symbols()), set(declared_functions())
    for n in ENTRY_POINTS:
        name = "gfdm_hip_link_meter_" + n
        assert hasattr(lib, name), "libgfdm_hip.so does not export %s" % name
        assert name in bound, "%s is missing from the ctypes table" % name
        assert name in declared, "%s is missing from include/gfdm_hip.h" % name
    assert sorted(n for n in bound if n.startswith("gfdm_hip_link_meter_")) == sorted("gfdm_hip_link_meter_" + n for n in ENTRY_POINTS)
    for name in ("bits_per_symbol", "decision_rule", "row_bytes", "reset", "totals", "ber", "fer", "match", "measure", "match_workspace_bytes",
                 "measure_workspace_bytes"):
        assert callable(getattr(gfdm_amd.LinkMeter, name))
    assert gfdm_amd.LinkMeter.FIELDS == M.FIELDS


def test_argument_tables_answer_without_a_device():
    import gfdm_amd
    L = gfdm_amd.lib()
    EINVAL = gfdm_amd.capi.EINVAL
    # create: the symbol mapper's table, before it looks for a device
    h = ctypes.c_void_p()
    pts = np.zeros(8, np.complex64)
    create = L.gfdm_hip_link_meter_create
    assert create(ctypes.byref(h), pts.ctypes.data, 3, -1, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 512, -1, 0) == EINVAL
    assert create(ctypes.byref(h), None, 4, -1, 0) == EINVAL and create(None, pts.ctypes.data, 4, -1, 0) == EINVAL
    assert create(ctypes.byref(h), pts.ctypes.data, 4, 3, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 4, -2, 0) == EINVAL
    assert create(ctypes.byref(h), pts.ctypes.data, 8, 1, 0) == EINVAL and create(ctypes.byref(h), pts.ctypes.data, 4, 2, 0) == EINVAL
    assert b"does not match" in L.gfdm_hip_last_error() and not h.value
    # a NULL handle is EINVAL in every call
    buf = np.zeros(16, np.int64)
    p = buf.ctypes.data
    assert L.gfdm_hip_link_meter_match_host(None, p, p, p, None, 1, p, 1, 0, 0) == EINVAL
    assert L.gfdm_hip_link_meter_match_device(None, p, p, p, None, 1, p, 1, 0, 0, p, None) == EINVAL
    assert L.gfdm_hip_link_meter_measure_host(None, p, p, p, p, p, 1, None, None, 1, 1) == EINVAL
    assert L.gfdm_hip_link_meter_measure_device(None, p, p, p, p, p, 1, None, None, 1, 1, p, None) == EINVAL
    assert L.gfdm_hip_link_meter_reset(None, None) == EINVAL and L.gfdm_hip_link_meter_totals(None, p, None) == EINVAL
    assert L.gfdm_hip_link_meter_totals_device(None) is None
    assert L.gfdm_hip_link_meter_row_bytes(None, 8) == EINVAL and L.gfdm_hip_link_meter_bits_per_symbol(None) == EINVAL
    assert L.gfdm_hip_link_meter_n_points(None) == EINVAL and L.gfdm_hip_link_meter_decision(None) == EINVAL
    # the workspace sizes need no handle: one 64-bit key per sent burst, two 24-byte records per tile of 2048 symbols
    mws, ws = L.gfdm_hip_link_meter_match_workspace_bytes, L.gfdm_hip_link_meter_measure_workspace_bytes
    assert mws(0) == 16 and mws(2) == 16 and mws(300) == 2400 and mws(-1) == EINVAL and mws(1 << 31) == EINVAL and mws((1 << 31) - 1) == 8 * ((1 << 31) - 1)
    assert ws(1, 0) == 16 and ws(1, 1) == 48 and ws(M.TILE, 1) == 48 and ws(M.TILE + 1, 1) == 96 and ws(5, 32768 + 7) == 48 * math.ceil(5 * 32775 / M.TILE)
    assert ws(0, 1) == EINVAL and ws(1, -1) == EINVAL and ws(1 << 62, 1) == EINVAL
    if not have_gpu():
        with pytest.raises(gfdm_amd.GfdmHipError) as e:                     # no CPU path: a valid constellation needs a device
            gfdm_amd.LinkMeter(S.constellations()["gr_qpsk"][0])
        assert e.value.status == gfdm_amd.capi.ENODEV
    with pytest.raises(ValueError):
        gfdm_amd.LinkMeter(np.ones(3))


@pytest.mark.gpu
def test_einval_tables_of_match_and_measure():
    """the tables of match and measure need a handle, and a handle needs a device: every line of them, none of which launches"""
    if not have_gpu():
        pytest.fail("no MI355X visible")
    import gfdm_amd
    import torch
    L = gfdm_amd.lib()
    EINVAL = gfdm_amd.capi.EINVAL
    lm = gfdm_amd.LinkMeter(S.constellations()["qam16"][0])
    h = lm._h
    d = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    match, measure = L.gfdm_hip_link_meter_match_device, L.gfdm_hip_link_meter_measure_device
    for tol in (-1, 1 << 31):
        assert match(h, p, p, p, None, 2, p, 2, 0, tol, p, None) == EINVAL and b"tol" in L.gfdm_hip_last_error()
    for n in (-1, 1 << 31):
        assert match(h, p, p, p, None, n, p, 2, 0, 0, p, None) == EINVAL and b"n_rows" in L.gfdm_hip_last_error()
        assert match(h, p, p, p, None, 2, p, n, 0, 0, p, None) == EINVAL and b"n_sent" in L.gfdm_hip_last_error()
    assert match(h, p, p, None, None, 2, p, 2, 0, 0, p, None) == EINVAL and match(h, p, p, p, None, 2, None, 2, 0, 0, p, None) == EINVAL
    assert match(h, p, p, p, None, 2, p, 2, 0, 0, None, None) == EINVAL and b"workspace" in L.gfdm_hip_last_error()
    assert match(h, None, None, None, None, 0, None, 0, 0, 0, None, None) == 0          # nothing to do
    assert measure(h, p, p, p, p, p, 1, None, None, 0, 1, p, None) == EINVAL and b"n_sym" in L.gfdm_hip_last_error()
    assert measure(h, p, p, p, p, p, 1, None, None, 1, -1, p, None) == EINVAL and b"n_rows" in L.gfdm_hip_last_error()
    assert measure(h, p, p, p, p, p, 1, None, None, (1 << 29), 1, p, None) == EINVAL and b"int32" in L.gfdm_hip_last_error()      # 4 * 2^29 = 2^31
    assert measure(h, p, p, p, p, p, -1, None, None, 4, 1, p, None) == EINVAL and b"n_ref" in L.gfdm_hip_last_error()
    assert measure(h, p, p, p, p, None, 0, None, None, 4, 1, p, None) == EINVAL and b"payload" in L.gfdm_hip_last_error()          # bit_errors, no payload
    assert measure(h, None, p, p, None, None, 0, None, None, 4, 1, p, None) == EINVAL and measure(h, None, p, p, p, None, 0, None, None, 4, 1, None, None) == EINVAL
    assert measure(h, None, p, p, p + 4, None, 0, None, None, 4, 1, p, None) == EINVAL and b"alignment" in L.gfdm_hip_last_error()
    assert measure(h, None, None, None, None, None, 0, None, None, 4, 0, None, None) == 0    # n_rows == 0: no launch
    torch.cuda.synchronize()
    assert lm.totals() == M.zero_totals()


@pytest.mark.parametrize("name", sorted(S.constellations()))
def test_restatement_counts_what_decode_and_the_payload_differ_in(name):
    """bit_errors of the restatement == popcount(unpackbits(S.decode(x) ^ (data & mask))) per row, on every shape of the mapper's table"""
    points, rule = S.constellations()[name]
    for n_rows, n_sym in S.shapes():
        c = S.case(name, n_rows, n_sym)
        m = M.measure(c["x"], points, rule, c["data"])
        decoded, _ = S.decode(c["x"], points, rule)
        mask = S.spare_mask(n_sym, c["k"])
        want = np.unpackbits(decoded ^ (c["data"] & mask), axis=1).sum(axis=1)
        assert np.array_equal(m["bit_errors"], want) and np.array_equal(M.popcount_rows(decoded, c["data"], n_sym, c["k"]), want)
        assert np.array_equal(m["symbol_errors"], (S.indices(c["x"], points, rule) != c["idx"]).sum(axis=1))
        assert m["totals"]["bit_errors"] == want.sum() and m["totals"]["bits"] == n_rows * n_sym * c["k"] and m["totals"]["rows"] == n_rows
        # spare bits set to 1 change nothing; the powers are those of the definitions
        m1 = M.measure(c["x"], points, rule, c["data"] | ~mask)
        assert np.array_equal(m1["bit_errors"], want)
        sent = points[c["idx"]].astype(np.complex128)
        assert np.allclose(m["err_power"], (np.abs(c["x"].astype(np.complex128) - sent) ** 2).sum(axis=1), rtol=1e-12)
        assert np.allclose(m["ref_power"], (np.abs(sent) ** 2).sum(axis=1), rtol=1e-12)
        dd = M.measure(c["x"], points, rule)
        assert dd["bit_errors"] is None and np.all(dd["err_power"] <= m["err_power"] * (1 + 1e-12))        # the decided point is the nearest one
        assert dd["totals"]["bits"] == 0 and dd["totals"]["symbols"] == n_rows * n_sym


def _match(fs, sent, tol, offset=0, count=None):
    ref_row, sent_row, t = M.match(fs, sent, tol, offset, count)
    return ref_row.tolist(), sent_row.tolist(), (t["detections"], t["matched"], t["missed"], t["false_alarms"])


def test_known_answers_of_match():
    for args, want in M.KNOWN_MATCHES:
        assert _match(*args) == want, args


def test_preconditions_of_the_gpu_tests():
    c = S.constellations()
    for name in M.noisy_names():
        points, rule = c[name]
        for n_rows, n_sym in S.shapes() + (list(S.MANY_ROWS) if name in S.MANY_ROWS_NAMES else []):
            k = S.case(name, n_rows, n_sym)
            if n_rows * n_sym >= 63:                                        # the noise really turns decisions
                assert M.measure(k["x"], points, rule, k["data"])["totals"]["bit_errors"] > 0, (name, n_rows, n_sym)
            if rule == "nearest":
                _, margin = S.decode(k["x"], points, rule)
                assert np.count_nonzero(~S.guarded(k["x"], margin)) <= S.GUARD_CAP * n_rows * n_sym
    # the seeded match case has what it is there for: matches, misses, false alarms, two bids for one burst, detections beyond tol
    fs, sent, tol, offset = M.match_case()
    ref_row, sent_row, t = M.match(fs, sent, tol, offset)
    assert np.all(np.diff(sent) > 0) and fs.size == 320 and sent.size == 300 and np.any(np.diff(fs) < 0)
    assert t["matched"] > 150 and t["missed"] > 50 and t["false_alarms"] > 50 and t["detections"] == 314
    assert t["matched"] + t["missed"] == 300 and t["matched"] + t["false_alarms"] == t["detections"]
    near = np.abs(fs[:, None] - (sent + offset)[None, :]) <= tol
    assert np.any(near.sum(axis=0) >= 2), "no sent burst with two bids"
    assert np.array_equal(np.sort(ref_row[ref_row >= 0]), np.flatnonzero(sent_row >= 0))
