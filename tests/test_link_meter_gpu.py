"""GPU tests of the link meter (contract in include/gfdm_hip.h, gfdm_hip_link_meter).  Two yardsticks, neither the code under test:
  the symbol mapper's decode on the SAME device tensor: bit_errors[r] == popcount(decode(x)[r] ^ payload[ref(r)]) over the live bits and
           the integer totals equal the sums -- exactly, with no guard: measure decides with decode's own device function;
  the numpy restatement of tests/link_meter_ref.py (float64 on the float32 inputs): both powers within 2^-19 relative (the header's
           derivation: 23 roundings of 2^-24 at most), bit_errors within k per symbol whose float64 decision margin is inside the mapper's
           guard and exact on every row without one; decision-directed ref_power gets (max |p|^2 - min |p|^2) per such symbol,
           decision-directed err_power nothing: a minimum of rounded distances is within the same relative error of the exact minimum.
A tile of the measure kernel is 2048 symbols (link_meter_ref.TILE): rows of 4097 symbols are longer than two tiles, 7 of them cross a
boundary fourteen times, and 32768 + 7 rows of 5 put four hundred rows into every tile.  match is compared exactly."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import gfdm_ref as R
import link_meter_ref as M
import symbol_mapper_ref as S
from burst_detect_ref import ref_detect
from burst_receive_cases import restatement, virtual_bursts
from conftest import have_gpu, rel_err

pytestmark = pytest.mark.gpu
GUARD = 16                                  # canary elements on either side of an output
FILL = {"uint8": 0xA5, "float32": 777.0, "complex64": 7 + 7j, "int32": -777, "int64": -777}
WORST = {"share": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")
    yield
    print("worst measured share of the 2^-19 budget over the module: %.3f" % WORST["share"])


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def meters():
    import gfdm_amd
    return {name: gfdm_amd.LinkMeter(points) for name, (points, _) in S.constellations().items()}


@pytest.fixture(scope="module")
def mappers():
    import gfdm_amd
    return {name: gfdm_amd.SymbolMapper(points) for name, (points, _) in S.constellations().items()}


class Window:
    """n elements of `dtype` inside a larger device buffer, `shift` elements past a 16-byte boundary, canaries on either side"""

    def __init__(self, dtype, n, shift, content=None):
        import torch
        name = np.dtype(dtype).name
        self.lo, self.n = GUARD + shift, n
        self.buf = torch.full((self.lo + n + GUARD,), FILL[name], dtype=getattr(torch, name), device="cuda:0")
        self.view = self.buf[self.lo:self.lo + n]
        self.fill = _h(self.buf[:1]).copy()
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * np.dtype(dtype).itemsize) % 16
        if content is not None:
            self.view.copy_(_t(np.ascontiguousarray(content).ravel()))

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.fill) and np.all(b[self.lo + self.n:] == self.fill), "canaries overwritten"
        return b[self.lo:self.lo + self.n]


def _unguarded(c, x, ok):
    """per row: the measured symbols whose float64 decision margin is inside the mapper's guard (none under the sign rules, which are exact)"""
    if c["rule"] != "nearest":
        return np.zeros(x.shape[0], np.int64)
    xs = np.where(ok[:, None], x, 0).astype(np.complex64)
    _, margin = S.decode(xs, c["points"], c["rule"])
    return (~S.guarded(xs, margin) & ok[:, None]).sum(axis=1)


def _check(lm, mp, c, x=None, payload="data", ref_row=None, count=None, tag="", got=None):
    """one measure call (or `got`, the outputs of one that was made elsewhere, with its totals) against decode and against the
    restatement; returns the outputs as numpy arrays and the totals"""
    x = c["x"] if x is None else x
    payload = c["data"] if isinstance(payload, str) else payload
    n_rows, n_sym, k = x.shape[0], x.shape[1], c["k"]
    dx = _t(x)
    if got is None:
        lm.reset()
        q = lm.measure(dx, None if payload is None else _t(payload), ref_row=None if ref_row is None else _t(ref_row), count=count)
        got = ({key: _h(v) for key, v in q.items()}, lm.totals())
    q, t = got
    want = M.measure(x, c["points"], c["rule"], payload, ref_row, count)
    ok = want["measured"]
    assert q["err_power"].dtype == np.float32 and q["ref_power"].dtype == np.float32 and q["err_power"].shape == (n_rows,)
    assert not q["err_power"][~ok].any() and not q["ref_power"][~ok].any()
    assert t["detections"] == t["matched"] == t["missed"] == t["false_alarms"] == 0
    assert t["rows"] == int(ok.sum()) and t["symbols"] == int(ok.sum()) * n_sym
    ung = _unguarded(c, x, ok)
    if payload is not None:
        ref, _ = M.measured_rows(n_rows, len(payload), ref_row, count)
        dec = _h(mp.decode(dx))                                             # the same device tensor: exact, no guard
        be = q["bit_errors"]
        assert be.dtype == np.int32 and np.all(be[~ok] == -1)
        pc = M.popcount_rows(dec[ok], payload[ref[ok]], n_sym, k)
        assert np.array_equal(be[ok], pc), (c["name"], tag, n_rows, n_sym)
        se = (S.unpack(dec[ok], n_sym, k) != S.unpack(payload[ref[ok]], n_sym, k)).sum()
        assert (t["bit_errors"], t["symbol_errors"], t["row_errors"], t["bits"]) == (int(pc.sum()), int(se), int((pc > 0).sum()), int(ok.sum()) * n_sym * k)
        assert np.all(np.abs(be[ok] - want["bit_errors"][ok]) <= k * ung[ok]), (c["name"], tag)
    else:
        assert "bit_errors" not in q and t["bits"] == t["bit_errors"] == t["symbol_errors"] == t["row_errors"] == 0
    p2 = np.abs(c["points"].astype(np.complex128)) ** 2
    allow = (p2.max() - p2.min()) * ung if payload is None else 0 * ung
    fin = ok & np.isfinite(want["err_power"])
    for key, extra in (("err_power", 0 * ung), ("ref_power", allow)):
        err = np.abs(q[key].astype(np.float64) - want[key])
        rows = fin if key == "err_power" else ok
        assert np.all(err[rows] <= M.BUDGET * want[key][rows] + extra[rows]), (c["name"], tag, key, float(np.max(err[rows] / want[key][rows])))
        clean = rows & (extra == 0) & (want[key] > 0)
        if clean.any():
            WORST["share"] = max(WORST["share"], float(np.max(err[clean] / want[key][clean])) / M.BUDGET)
    assert not np.isfinite(q["err_power"][ok & ~fin]).any()
    return q, t


@pytest.mark.parametrize("name", M.noisy_names())
def test_every_shape(name, meters, mappers):
    """k = 1, 2, 2, 3, 4, 6, 8 by n_sym 1 .. 4097 by 1 and 7 rows, data-aided and decision-directed"""
    lm, mp = meters[name], mappers[name]
    points, rule = S.constellations()[name]
    assert lm.decision_rule() == rule == mp.decision_rule() and lm.bits_per_symbol() == S.bits_per_symbol(points)
    for n_rows, n_sym in S.shapes():
        c = S.case(name, n_rows, n_sym)
        assert lm.row_bytes(n_sym) == c["data"].shape[1]
        _check(lm, mp, c)
        _check(lm, mp, c, payload=None, tag="decision-directed ")
    print("%s: worst share of the power budget so far %.3f" % (name, WORST["share"]))


@pytest.mark.parametrize("name", S.MANY_ROWS_NAMES)
def test_many_rows(name, meters, mappers):
    """5000 rows of 3 symbols and 32768 + 7 rows of 5: several hundred rows per tile, finished by the tile, every tile boundary inside a row
    or between two"""
    for n_rows, n_sym in S.MANY_ROWS:
        c = S.case(name, n_rows, n_sym)
        _check(meters[name], mappers[name], c)
        _check(meters[name], mappers[name], c, payload=None)


@pytest.mark.parametrize("n_sym", (65, 4097))
def test_ref_row(n_sym, meters, mappers):
    """a permutation; entries -1, n_ref and n_ref + 5 (unmeasured: -1 / 0 / 0, their symbols NaN to show they are not read); two rows
    against one payload row; no ref_row with fewer payload rows than rows"""
    lm, mp = meters["qam16"], mappers["qam16"]
    c = S.case("qam16", 7, n_sym)
    rng = np.random.default_rng(n_sym)
    perm = rng.permutation(7).astype(np.int64)
    payload = np.empty_like(c["data"])
    payload[perm] = c["data"]                                               # row r was sent as payload row perm[r]
    q, _ = _check(lm, mp, c, payload=payload, ref_row=perm, tag="permutation ")
    base, _ = _check(lm, mp, c)
    for key in base:
        assert np.array_equal(q[key].view(np.uint8), base[key].view(np.uint8)), key
    x = c["x"].copy()
    ref = np.array([0, -1, 2, 7, 4, 12, 6], np.int64)
    x[[1, 3, 5]] = complex(np.nan, np.nan)
    q, t = _check(lm, mp, c, x=x, ref_row=ref, tag="unmeasured ")
    assert q["bit_errors"].tolist()[1::2] == [-1, -1, -1] and t["rows"] == 4 and np.all(np.isfinite(q["err_power"]))
    for key in base:
        assert np.array_equal(q[key][::2].copy().view(np.uint8), base[key][::2].copy().view(np.uint8)), key
    q, _ = _check(lm, mp, c, ref_row=np.array([3, 3, 2, 3, 0, 0, 6], np.int64), tag="repeated ")
    assert q["bit_errors"][3] == base["bit_errors"][3] and q["bit_errors"][0] > base["bit_errors"][0]
    x = c["x"].copy()
    x[4:] = complex(np.nan, np.nan)
    q, t = _check(lm, mp, c, x=x, payload=c["data"][:4], tag="short payload ")
    assert q["bit_errors"].tolist()[4:] == [-1, -1, -1] and t["rows"] == 4
    q, t = _check(lm, mp, c, x=np.full_like(c["x"], complex(np.nan, np.nan)), payload=c["data"][:0], tag="empty payload ")
    assert q["bit_errors"].tolist() == [-1] * 7 and t == M.zero_totals()
    # decision-directed: ref_row only says which rows count
    q, t = _check(lm, mp, c, x=x, payload=None, ref_row=np.array([5, 0, 99, 1, -1, -1, -3], np.int64), tag="decision-directed ")
    assert t["rows"] == 4


def test_spare_payload_bits_change_nothing(meters, mappers):
    for name, n_sym in (("psk8", 65), ("qam64", 257), ("gr_bpsk", 3)):
        c = S.case(name, 7, n_sym)
        mask = S.spare_mask(n_sym, c["k"])
        assert (mask != 0xFF).any()
        a, ta = _check(meters[name], mappers[name], c)
        b, tb = _check(meters[name], mappers[name], c, payload=c["data"] | ~mask)
        assert ta == tb and all(np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)) for key in a)


@pytest.mark.parametrize("name", ("gr_qpsk", "qam64"))
def test_count(name, meters, mappers):
    """count below, at and beyond n_rows and negative, as an int and as a device tensor; the rows from n_live on hold NaN"""
    import torch
    c = S.case(name, 7, 257)
    for cnt in (0, 3, 7, 12, -1):
        x = c["x"].copy()
        x[S.live(cnt, 7):] = complex(np.nan, np.nan)
        for count in (cnt, _t([cnt], torch.int64)):
            lm = meters[name]
            lm.reset()
            q = lm.measure(_t(x), _t(c["data"]), count=count)
            got = ({key: _h(v) for key, v in q.items()}, lm.totals())
            _check(lm, mappers[name], c, x=x, count=cnt, got=got)
            assert got[1]["rows"] == S.live(cnt, 7)


@pytest.mark.parametrize("case", (("qam16", 7, 65), ("psk8", 7, 4097), ("qam64", 5000, 3)))
def test_every_alignment(case, meters, mappers):
    """symbols at 8 but not 16 bytes, the payload at every byte offset 0 .. 3, outputs at 4 but not 16 bytes, ref_row at 8 but not 16: the
    outputs are those of the aligned call to the bit (the tiling follows the symbols, not the addresses) and no canary is touched"""
    name, n_rows, n_sym = case
    lm, mp = meters[name], mappers[name]
    c = S.case(name, n_rows, n_sym)
    base, tb = _check(lm, mp, c)
    ident = np.arange(n_rows, dtype=np.int64)
    for shift in range(4):
        x = Window(np.complex64, n_rows * n_sym, 1, c["x"])
        data = Window(np.uint8, c["data"].size, shift, c["data"])
        ref = Window(np.int64, n_rows, 1, ident)
        outs = {"bit_errors": Window(np.int32, n_rows, 1 + shift % 3), "err_power": Window(np.float32, n_rows, 3 - shift % 3),
                "ref_power": Window(np.float32, n_rows, 1 + (shift + 1) % 3)}
        lm.reset()
        q = lm.measure(x.view.view(n_rows, n_sym), data.view.view(n_rows, -1), ref_row=ref.view, out={k: w.view for k, w in outs.items()})
        assert all(q[k] is outs[k].view for k in outs)
        for key, w in outs.items():
            assert np.array_equal(w.result().view(np.uint8), base[key].view(np.uint8)), (key, shift)
        assert lm.totals() == tb
        assert np.array_equal(x.result(), c["x"].ravel()) and np.array_equal(data.result(), c["data"].ravel()) and np.array_equal(ref.result(), ident)


@pytest.mark.parametrize("name", ("gr_qpsk", "psk8", "grid256"))
def test_poison_stays_in_its_row(name, meters, mappers):
    """a NaN and an infinity in one row: that row's err_power is non-finite, its ref_power the definition's sum over points (finite), its
    bit_errors the contract's (NaN and, under NEAREST, infinity decide as index 0; the sign rules take an infinity by its sign); every
    other row is bit-equal to the clean run; the totals stay finite integers"""
    lm, mp = meters[name], mappers[name]
    for n_rows, n_sym in ((7, 65), (7, 4097)):
        c = S.case(name, n_rows, n_sym)
        base, _ = _check(lm, mp, c)
        x = c["x"].copy()
        x[2, 17 % n_sym], x[2, n_sym - 1] = complex(np.nan, 0.25), complex(0.5, -np.inf)
        q, t = _check(lm, mp, c, x=x, tag="poison ")
        assert not np.isfinite(q["err_power"][2]) and np.isfinite(q["ref_power"][2])
        want = M.measure(x, c["points"], c["rule"], c["data"])
        assert q["bit_errors"][2] == want["bit_errors"][2] or c["rule"] == "nearest"       # (NEAREST: up to the guard, held by _check)
        others = np.arange(n_rows) != 2
        for key in base:
            assert np.array_equal(q[key][others].view(np.uint8), base[key][others].view(np.uint8)), key
        assert all(isinstance(v, int) and 0 <= v < 1 << 40 for v in t.values())
        dd, _ = _check(lm, mp, c, x=x, payload=None, tag="poison, decision-directed ")
        assert not np.isfinite(dd["err_power"][2]) and np.all(np.isfinite(dd["err_power"][others]))


def test_determinism(meters):
    """the same call twice gives bit-equal float outputs: rows of 4097 symbols (partial records summed in tile order) and 32768 + 7 rows"""
    for name, n_rows, n_sym in (("qam64", 7, 4097), ("psk8", 32768 + 7, 5)):
        c = S.case(name, n_rows, n_sym)
        dx, dp = _t(c["x"]), _t(c["data"])
        runs = [{k: _h(v) for k, v in meters[name].measure(dx, dp).items()} for _ in range(3)]
        for other in runs[1:]:
            for key in runs[0]:
                assert np.array_equal(runs[0][key].view(np.uint8), other[key].view(np.uint8)), (name, key)


def test_accumulation(meters):
    """two measure calls plus one match call, then totals() is the sum; reset() gives zeros; two handles do not share totals"""
    import gfdm_amd
    lm = meters["qam16"]
    other = gfdm_amd.LinkMeter(S.constellations()["qam16"][0])
    a, b = S.case("qam16", 7, 257), S.case("qam16", 1, 4097)
    fs, sent, tol, offset = M.match_case()
    lm.reset()
    lm.measure(_t(a["x"]), _t(a["data"]))
    lm.measure(_t(b["x"]), _t(b["data"]))
    lm.match(_t(fs), _t(sent), tol, offset=offset)
    other.measure(_t(b["x"]), _t(b["data"]))
    parts = [M.measure(k["x"], k["points"], k["rule"], k["data"])["totals"] for k in (a, b)] + [M.match(fs, sent, tol, offset)[2]]
    want = M.add_totals(*parts)
    got = lm.totals()
    for f in ("rows", "symbols", "bits", "detections", "matched", "missed", "false_alarms"):
        assert got[f] == want[f], f
    # the error counts are those of the two calls alone (decisions on the device: compared with decode in test_every_shape)
    lm.reset()
    lm.measure(_t(a["x"]), _t(a["data"]))
    ta = lm.totals()
    lm.reset()
    lm.measure(_t(b["x"]), _t(b["data"]))
    tb = lm.totals()
    for f in ("bit_errors", "symbol_errors", "row_errors"):
        assert got[f] == ta[f] + tb[f] and ta[f] > 0, f
    assert other.totals() == tb
    assert lm.ber() == tb["bit_errors"] / tb["bits"] and lm.fer() == tb["row_errors"] / tb["rows"]
    lm.reset()
    assert lm.totals() == M.zero_totals() and np.isnan(lm.ber()) and np.isnan(lm.fer())
    assert other.totals() == tb
    lm.match(_t(fs), _t(sent), tol, offset=offset)
    t = lm.totals()
    assert lm.fer() == 1.0 and t["missed"] > 0 and t["rows"] == 0


def test_match(meters):
    """the CPU file's known answers on the device, then 320 detections against 300 sent bursts, tol = 3: ref_row, sent_row and the four
    totals exactly; canaries around both outputs"""
    import torch
    lm = meters["gr_qpsk"]
    for (fs, sent, tol, offset, count), (ref_row, sent_row, totals) in M.KNOWN_MATCHES:
        for cnt in ((count,) if count is None else (count, _t([count], torch.int64))):
            lm.reset()
            m = lm.match(_t(fs, torch.int64), _t(sent, torch.int64), tol, offset=offset, count=cnt)
            t = lm.totals()
            assert _h(m["ref_row"]).tolist() == ref_row and _h(m["sent_row"]).tolist() == sent_row, (fs, sent)
            assert (t["detections"], t["matched"], t["missed"], t["false_alarms"]) == totals and t["rows"] == t["bits"] == 0
    fs, sent, tol, offset = M.match_case()
    want_ref, want_sent, want_t = M.match(fs, sent, tol, offset)
    for shift in (0, 1):
        outs = {"ref_row": Window(np.int64, fs.size, shift), "sent_row": Window(np.int64, sent.size, 1 - shift)}
        lm.reset()
        lm.match(Window(np.int64, fs.size, 1 - shift, fs).view, Window(np.int64, sent.size, shift, sent).view, tol, offset=offset,
                 out={k: w.view for k, w in outs.items()})
        assert np.array_equal(outs["ref_row"].result(), want_ref) and np.array_equal(outs["sent_row"].result(), want_sent)
        assert lm.totals() == want_t
    for cnt in (100, 0):
        lm.reset()
        m = lm.match(_t(fs), _t(sent), tol, offset=offset, count=cnt)
        w = M.match(fs, sent, tol, offset, cnt)
        assert np.array_equal(_h(m["ref_row"]), w[0]) and np.array_equal(_h(m["sent_row"]), w[1]) and lm.totals() == w[2]


def test_host_flavour_equals_device_flavour(meters):
    lm = meters["psk8"]
    c = S.case("psk8", 7, 4097)
    ref = np.array([1, 0, -1, 3, 9, 5, 5], np.int64)
    fs, sent, tol, offset = M.match_case()
    for count in (None, 5):
        lm.reset()
        dev = lm.measure(_t(c["x"]), _t(c["data"]), ref_row=_t(ref), count=count)
        dev_dd = lm.measure(_t(c["x"]), count=count)
        dev_m = lm.match(_t(fs), _t(sent), tol, offset=offset, count=count)
        td = lm.totals()
        lm.reset()
        host = lm.measure(c["x"], c["data"], ref_row=ref, count=count)
        host_dd = lm.measure(c["x"], count=count)
        host_m = lm.match(fs, sent, tol, offset=offset, count=count)
        assert lm.totals() == td
        for h, d in ((host, dev), (host_dd, dev_dd), (host_m, dev_m)):
            assert sorted(h) == sorted(d)
            for key in h:
                assert isinstance(h[key], np.ndarray) and np.array_equal(h[key].view(np.uint8), _h(d[key]).view(np.uint8)), key
    assert host["bit_errors"].dtype == np.int32 and host["err_power"].dtype == np.float32 and host_m["ref_row"].dtype == np.int64
    # the raw C calls with single outputs left out (the wrapper always passes both powers and both rows of match): what is asked for equals
    # the all-outputs call above (count = 5) bit for bit, and so do the totals
    import gfdm_amd
    L = gfdm_amd.lib()
    x, data, cnt = np.ascontiguousarray(c["x"]), np.ascontiguousarray(c["data"]), np.array([5], np.int64)
    fs, sent = np.ascontiguousarray(fs, np.int64), np.ascontiguousarray(sent, np.int64)
    lm.reset()
    lm.measure(c["x"], c["data"], ref_row=ref, count=5)
    t_measure = lm.totals()
    lm.reset()
    lm.match(fs, sent, tol, offset=offset, count=5)
    t_match = lm.totals()
    for keep in ("bit_errors", "err_power", "ref_power"):
        got = np.zeros(7, host[keep].dtype)
        ptr = {k: got.ctypes.data if k == keep else None for k in ("bit_errors", "err_power", "ref_power")}
        lm.reset()
        assert L.gfdm_hip_link_meter_measure_host(lm._h, ptr["bit_errors"], ptr["err_power"], ptr["ref_power"], x.ctypes.data, data.ctypes.data, 7,
                                                  ref.ctypes.data, cnt.ctypes.data, 4097, 7) == 0
        assert np.array_equal(got.view(np.uint8), host[keep].view(np.uint8)) and lm.totals() == t_measure, keep
    for keep in ("ref_row", "sent_row"):
        got = np.zeros(host_m[keep].size, np.int64)
        lm.reset()
        assert L.gfdm_hip_link_meter_match_host(lm._h, got.ctypes.data if keep == "ref_row" else None, got.ctypes.data if keep == "sent_row" else None,
                                                fs.ctypes.data, cnt.ctypes.data, fs.size, sent.ctypes.data, sent.size, offset, tol) == 0
        assert np.array_equal(got, host_m[keep]) and lm.totals() == t_match, keep
    assert lm.measure(c["x"][:0], c["data"][:0])["err_power"].shape == (0,)
    with pytest.raises(TypeError):
        lm.measure(_t(c["x"]), c["data"])
    with pytest.raises(ValueError):
        lm.measure(c["x"], out={"bit_errors": np.zeros(7, np.int32)})
    with pytest.raises(RuntimeError):
        lm.measure(c["x"], c["data"][:, :-1])


def test_graph_replay(meters, mappers):
    """reset + match + measure captured once as a single chain and replayed with a changed count, changed frame_start and changed symbols:
    outputs and totals are right after every replay (no memset in front of an output, every element written by the call's own kernels)"""
    import torch
    name, n_rows, n_sym = "qam64", 7, 4097
    lm, mp = meters[name], mappers[name]
    c = S.case(name, n_rows, n_sym)
    sent = np.array([100, 200, 300, 400, 500], np.int64)
    x = torch.zeros(n_rows, n_sym, dtype=torch.complex64, device="cuda:0")
    payload = _t(c["data"][:5])
    fs = torch.zeros(n_rows, dtype=torch.int64, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_sent = _t(sent)
    outs = {"ref_row": torch.zeros(n_rows, dtype=torch.int64, device="cuda:0"), "sent_row": torch.zeros(5, dtype=torch.int64, device="cuda:0"),
            "bit_errors": torch.zeros(n_rows, dtype=torch.int32, device="cuda:0"), "err_power": torch.zeros(n_rows, dtype=torch.float32, device="cuda:0"),
            "ref_power": torch.zeros(n_rows, dtype=torch.float32, device="cuda:0")}
    ws_m = torch.empty(lm.match_workspace_bytes(5), dtype=torch.uint8, device="cuda:0")
    ws_q = torch.empty(lm.measure_workspace_bytes(n_sym, n_rows), dtype=torch.uint8, device="cuda:0")

    def chain():
        lm.reset()
        lm.match(fs, d_sent, 2, offset=7, count=count, out=outs, workspace=ws_m)
        lm.measure(x, payload, ref_row=outs["ref_row"], count=count, out=outs, workspace=ws_q)

    x.copy_(_t(c["x"]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    replays = ((7, [107, 207, 308, 405, 507, 999, -1], 0), (4, [507, 407, 307, 207, 107, 107, 107], 1), (12, [-1, 106, 108, 107, 310, 407, 505], 2),
               (0, [107, 207, 307, 407, 507, 0, 0], 0))
    for cnt, starts, seed in replays:
        xs = S.case(name, n_rows, n_sym, seed)["x"]
        x.copy_(_t(xs))
        fs.copy_(_t(np.array(starts, np.int64)))
        count.fill_(cnt)
        graph.replay()
        torch.cuda.synchronize()
        want_ref, want_sent, want_t = M.match(starts, sent, 2, 7, cnt)
        assert np.array_equal(_h(outs["ref_row"]), want_ref) and np.array_equal(_h(outs["sent_row"]), want_sent), (cnt, starts)
        t = lm.totals()
        for f in ("detections", "matched", "missed", "false_alarms"):
            assert t[f] == want_t[f], (f, cnt)
        got = ({k: _h(outs[k]) for k in ("bit_errors", "err_power", "ref_power")}, dict(t, detections=0, matched=0, missed=0, false_alarms=0))
        _check(lm, mp, c, x=xs, payload=c["data"][:5], ref_row=want_ref, count=cnt, tag="replay %d " % cnt, got=got)


def test_loop(meters):
    """burst_shaper_ref.loop_case() through map, transmit, place, the channel, detect and demodulate_bursts exactly as
    tests/test_channel_model_gpu.py::test_loop_with_a_channel builds it (complex64), then match and measure: every burst is found and
    matched to itself, no bit is wrong, the spare rows are unmeasured; a sent position dropped makes its detection a false alarm, one
    added where nothing was sent is missed; and the data-aided EVM of every burst is below 1.5 times that of the float64 chain on the CPU
    for the same stream (computed here from the restatements, not fixed)."""
    import gfdm_amd
    c = B.loop_case()
    M_, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym = A * M_
    pts = R.qpsk_points().astype(np.complex64)
    payload = S.pack(S.indices(c["sym"], pts, "qpsk"), 2)
    m = gfdm_amd.SymbolMapper(pts)
    lm = meters["gr_qpsk"]
    sym = m.map(_t(payload), n_sym)
    tx = gfdm_amd.Transmitter(M_, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    assert len(frames) == 1 and rel_err(_h(frames[0]), c["frames"]) < 1e-5
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(frames, _t(c["starts"]), c["out_len"])[0]
    ch = gfdm_amd.ChannelModel(C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    ds = ch.apply(placed)
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    est = gfdm_amd.ChannelEstimator(M_, K, A, True, 1, c["preamble"])
    # the float64 chain on the CPU for the same stream
    _, y, _ = C.loop_stream()
    s = y.astype(np.complex64)
    d = ref_detect(s, c["preamble"], K, c["pcp"], c["window_len"], B.LOOP_THRESHOLD, c["min_distance"], c["lead"])
    e = virtual_bursts(s, d["frame_start"], d["sc_rot"], 0, c["F"])
    sent = c["sym"].astype(np.complex128)
    dpay, starts = _t(payload), _t(c["starts"])
    receivers = ((gfdm_amd.Demodulator(M_, K, L, c["taps"]), None), (gfdm_amd.AdvancedReceiver(M_, K, L, c["taps"], c["smap"], 2, R.qpsk_points()), 2))
    for rx, rounds in receivers:
        rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
        rx.set_channel_estimator(est)
        demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
        lm.reset()
        mt = lm.match(r["frame_start"], starts, 0, offset=c["pcp"], count=r["count"])
        q = lm.measure(demod, dpay, ref_row=mt["ref_row"], count=r["count"])
        t = lm.totals()
        assert (t["matched"], t["missed"], t["false_alarms"], t["bit_errors"], t["rows"], t["detections"]) == (nb, 0, 0, 0, nb, nb)
        assert t["bits"] == nb * n_sym * 2 and lm.ber() == 0.0 and lm.fer() == 0.0
        assert _h(mt["ref_row"]).tolist() == list(range(nb)) + [-1] * 3 and _h(mt["sent_row"]).tolist() == list(range(nb))
        be, ep, rp = _h(q["bit_errors"]), _h(q["err_power"]).astype(np.float64), _h(q["ref_power"]).astype(np.float64)
        assert be.tolist() == [0] * nb + [-1] * 3 and not ep[nb:].any() and not rp[nb:].any()
        ref_out, _ = restatement(c, e, rounds)
        evm_cpu = np.sqrt((np.abs(ref_out - sent) ** 2).sum(axis=1) / (np.abs(sent) ** 2).sum(axis=1))
        evm = np.sqrt(ep[:nb] / rp[:nb])
        print("rounds %s: EVM per burst %s, float64 chain %s" % (rounds, np.round(evm, 4), np.round(evm_cpu, 4)))
        assert np.all(evm < 1.5 * evm_cpu) and np.all(evm > 0)
        # decision-directed: no decision is wrong, so the noise estimate is the data-aided one
        dd = lm.measure(demod, None, count=r["count"])
        assert np.allclose(_h(dd["err_power"])[:nb], ep[:nb], rtol=1e-6) and not _h(dd["err_power"])[nb:].any()
        llr = _h(m.soft(demod, scale=n_sym / dd["err_power"], count=r["count"]))
        assert np.array_equal(np.packbits(llr[:nb] < 0, axis=1), payload) and not llr[nb:].any()
        # one sent position dropped: its detection is a false alarm and its row is not measured
        keep = np.array([j for j in range(nb) if j != 2])
        lm.reset()
        mt = lm.match(r["frame_start"], _t(c["starts"][keep]), 0, offset=c["pcp"], count=r["count"])
        q = lm.measure(demod, _t(payload[keep]), ref_row=mt["ref_row"], count=r["count"])
        t = lm.totals()
        assert (t["matched"], t["missed"], t["false_alarms"], t["rows"], t["bit_errors"]) == (nb - 1, 0, 1, nb - 1, 0)
        assert _h(mt["ref_row"])[2] == -1 and _h(q["bit_errors"])[2] == -1
        # one sent position where nothing was sent: missed
        extra = np.sort(np.append(c["starts"], c["starts"][-1] + 3 * c["frame_len"])).astype(np.int64)
        lm.reset()
        mt = lm.match(r["frame_start"], _t(extra), 0, offset=c["pcp"], count=r["count"])
        t = lm.totals()
        assert (t["matched"], t["missed"], t["false_alarms"]) == (nb, 1, 0) and _h(mt["sent_row"]).tolist() == list(range(nb)) + [-1]
        assert lm.fer() == 1.0                                              # rows == 0: the one missed burst is the only frame
