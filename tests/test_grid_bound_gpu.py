"""GPU tests of the device modules past their bounded grid (the cases and their arithmetic: tests/grid_bound_cases.py, held on the CPU by
tests/test_grid_bound.py).  Every module since the symbol mapper launches at most G workgroups and strides over the remaining tiles; the
other GPU tests stay far below G tiles, so a workgroup's second trip through its tile loop -- LDS reused behind a barrier, counters
and maxima carried from tile to tile, index arithmetic at tile numbers of 8192 and above, `count` ending the live rows in a later trip
-- runs here and nowhere else.  Every case has 2 G + 3 or 2 G + 4 tiles with a ragged last one and makes three checks:
  1. against the module's numpy restatement (tests/*_ref.py) under the comparison rule and the error budget of that module's own GPU
     tests, on windows: the rows or sample ranges under the tiles 0, G - 1 | G, 2 G - 1 | 2 G and the last two, and 64 seeded rows or
     ranges of 4096 samples;
  2. against the same handle called in three pieces that each stay below G tiles -- the regime the other tests hold to the restatement
     -- over the WHOLE output, on the device, bit for bit (the link meter's per-row floats excepted: the order of a crossing row's sum
     depends on where the tiles fall; its integers and totals are exact);
  3. canaries on both sides of every output, and, where a case has a count, zeros behind the live rows, which end in a third trip.
The inputs are made on the device from a fixed seed; only the windows travel to the host."""
import gc

import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import conv_code_ref as V
import grid_bound_cases as G
import link_meter_ref as M
import resampler_ref as Q
import symbol_mapper_ref as S
from conftest import have_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16                                  # canary elements on either side of a buffer: a multiple of 16 bytes for every dtype
FILL = {"uint8": 0xA5, "int16": 0x5A5A, "int32": -777, "float32": 777.0, "complex64": 7 + 7j}
CHUNK = 1 << 22                             # elements made at a time where an input needs temporaries


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


def _gen(salt):
    import torch
    g = torch.Generator(device=DEV)
    g.manual_seed(G.SEED + salt)
    return g


def _h(t):
    return t.cpu().numpy()


def _index(rows):
    import torch
    return torch.tensor(rows, dtype=torch.int64, device=DEV)


def _bits(t):
    """a tensor as integers: what torch.equal compares bit for bit"""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


class Guarded:
    """n elements of `dtype` inside a larger device buffer, `shift` elements past a 16-byte boundary, canaries on either side that are
    checked on the device"""

    def __init__(self, dtype, n, shift=0):
        import torch
        self.fill, self.lo, self.n = FILL[dtype], GUARD + shift, n
        self.buf = torch.full((self.lo + n + GUARD,), self.fill, dtype=getattr(torch, dtype), device=DEV)
        self.view = self.buf[self.lo:self.lo + n]
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * self.buf.element_size()) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())


def _live_part(count, a, b):
    """the count of the piece [a, b) of a call with `count` live rows"""
    return None if count is None else max(min(count - a, b - a), 0)


def _noisy_symbols(points, n, gen, shift):
    """n seeded points plus noise of a third of the smallest distance (errors happen, ties do not), complex64 in a Guarded buffer"""
    import torch
    x = Guarded("complex64", n, shift)
    pts = torch.tensor(points, device=DEV)
    sg = S.noise_sigma(points)
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        idx = torch.randint(0, len(points), (m,), device=DEV, generator=gen)
        x.view[a:a + m] = pts[idx] + sg * torch.view_as_complex(torch.randn((m, 2), device=DEV, generator=gen))
    return x


# ---------------------------------------------------------------- symbol mapper ----
def _mapper_case(case):
    import gfdm_amd
    geo = G.mapper_geometry(case)
    points, rule = S.constellations()[case["name"]]
    rows = G.window_rows(geo["tiling"], geo["unit"], geo["n_rows"], 1)
    count = geo["n_live"] if case["count"] else None
    return geo, points, rule, gfdm_amd.SymbolMapper(points), np.array(rows), count


@pytest.mark.parametrize("case", G.MAP_CASES, ids=G.case_id)
def test_symbols_map(case):
    import torch
    geo, points, rule, m, rows, count = _mapper_case(case)
    n_rows, n_sym, n_live = geo["n_rows"], case["n_sym"], geo["n_live"]
    data = torch.randint(0, 256, (n_rows, geo["row_bytes"]), dtype=torch.uint8, device=DEV, generator=_gen(10))
    out = Guarded("complex64", n_rows * n_sym, case["mis"])
    m.map(data, n_sym, count=count, out=out.view)
    whole = out.view.view(n_rows, n_sym)
    # 1. the restatement on the windows: equal, bit for bit
    want = S.map(_h(data[_index(rows)]), n_sym, points)
    want[rows >= n_live] = 0
    assert np.array_equal(_h(whole[_index(rows)]).view(np.uint32), want.view(np.uint32))
    # 2. the same handle in pieces
    again = Guarded("complex64", n_rows * n_sym, 0)
    parts = again.view.view(n_rows, n_sym)
    for a, b in G.pieces(n_rows):
        m.map(data[a:b], n_sym, count=_live_part(count, a, b), out=parts[a:b])
    assert _same(whole, parts)
    # 3. extents
    assert out.intact() and again.intact()
    assert n_live == n_rows or (not _bits(whole[n_live:]).any() and _bits(whole[:n_live]).any())


@pytest.mark.parametrize("case", G.DECODE_CASES, ids=G.case_id)
def test_symbols_decode(case):
    geo, points, rule, m, rows, count = _mapper_case(case)
    n_rows, n_sym, k, rb, n_live = geo["n_rows"], case["n_sym"], case["k"], geo["row_bytes"], geo["n_live"]
    x = _noisy_symbols(points, n_rows * n_sym, _gen(11), case["mis"])
    xv = x.view.view(n_rows, n_sym)
    out = Guarded("uint8", n_rows * rb, case["mis"])
    m.decode(xv, count=count, out=out.view)
    whole = out.view.view(n_rows, rb)
    # 1. sign rules equal everywhere; NEAREST equal on every symbol outside the mapper's guard, at most 0.1 % inside it
    live = rows[rows < n_live]
    xw, got = _h(xv[_index(live)]), _h(whole[_index(live)])
    want, margin = S.decode(xw, points, rule)
    if rule != "nearest":
        assert np.array_equal(got, want)
    else:
        ok = S.guarded(xw, margin)
        left_out = int(np.count_nonzero(~ok))
        print("%s: %d of %d window symbols inside the guard" % (case["id"], left_out, xw.size))
        assert left_out <= S.GUARD_CAP * xw.size
        assert np.array_equal(S.unpack(got, n_sym, k)[ok], S.unpack(want, n_sym, k)[ok])
        assert not (got & ~S.spare_mask(n_sym, k)).any()
    # 2.
    again = Guarded("uint8", n_rows * rb, 0)
    parts = again.view.view(n_rows, rb)
    for a, b in G.pieces(n_rows):
        m.decode(xv[a:b], count=_live_part(count, a, b), out=parts[a:b])
    assert _same(whole, parts)
    # 3.
    assert out.intact() and again.intact() and x.intact()
    assert n_live == n_rows or (not whole[n_live:].any() and whole[:n_live].any())


@pytest.mark.parametrize("case", G.SOFT_CASES, ids=G.case_id)
def test_symbols_soft(case):
    import torch
    geo, points, rule, m, rows, count = _mapper_case(case)
    n_rows, n_sym, k, n_live = geo["n_rows"], case["n_sym"], case["k"], geo["n_live"]
    gen = _gen(12)
    x = _noisy_symbols(points, n_rows * n_sym, gen, 1)
    xv = x.view.view(n_rows, n_sym)
    scale = 0.25 + 4 * torch.rand(n_rows, device=DEV, generator=gen)
    out = Guarded("float32", n_rows * n_sym * k, case["mis"])
    m.soft(xv, scale, count=count, out=out.view)
    whole = out.view.view(n_rows, n_sym * k)
    # 1. per element |got - ref| <= 8 * 2^-24 * |s_r| * (d0 + d1)
    live = rows[rows < n_live]
    sw = _h(scale[_index(live)])
    want, d0, d1 = S.soft(_h(xv[_index(live)]), points, sw)
    err, bound = np.abs(_h(whole[_index(live)]).astype(np.float64) - want), S.soft_bound(sw, d0, d1)
    print("%s: worst error %.3f of the bound" % (case["id"], float(np.max(err / bound))))
    assert np.all(err <= bound)
    # 2.
    again = Guarded("float32", n_rows * n_sym * k, 0)
    parts = again.view.view(n_rows, n_sym * k)
    for a, b in G.pieces(n_rows):
        m.soft(xv[a:b], scale[a:b], count=_live_part(count, a, b), out=parts[a:b])
    assert _same(whole, parts)
    # 3.
    assert out.intact() and again.intact()
    assert n_live == n_rows or (not _bits(whole[n_live:]).any() and _bits(whole[:n_live]).any())


# ---------------------------------------------------------------- link meter ----
def _unguarded(points, rule, x):
    """per row: the symbols whose float64 decision margin is inside the mapper's guard (none under the sign rules, which are exact)"""
    if rule != "nearest":
        return np.zeros(x.shape[0], np.int64)
    _, margin = S.decode(x, points, rule)
    return (~S.guarded(x, margin)).sum(axis=1)


@pytest.mark.parametrize("case", G.METER_CASES, ids=G.case_id)
def test_meter_measure(case):
    """bit_errors against the mapper's decode of the same window rows and against the restatement, both powers within 2^-19 relative
    (tests/test_link_meter_gpu.py's rule); the integer outputs and the totals of the pieces against the one call, exactly"""
    import torch
    import gfdm_amd
    geo = G.meter_geometry(case)
    n_rows, n_sym, k, rb, n_live = geo["n_rows"], case["n_sym"], case["k"], geo["row_bytes"], geo["n_live"]
    points, rule = S.constellations()[case["name"]]
    lm, mp = gfdm_amd.LinkMeter(points), gfdm_amd.SymbolMapper(points)
    gen = _gen(20)
    count = n_live if case["count"] else None
    payload = torch.randint(0, 256, (n_rows, rb), dtype=torch.uint8, device=DEV, generator=gen)
    ref = sent = None
    if case["ref_row"]:                     # row r was sent as payload row sent[r]; some rows are not measured: -1, and beyond the payload
        sent = torch.randperm(n_rows, device=DEV, generator=gen)
        ref = sent.clone()
        ref[::97] = -1
        ref[5::1013] = n_rows + 7
    # the symbols: the sent payload mapped in pieces below G tiles, plus noise
    x = Guarded("complex64", n_rows * n_sym, case["mis"])
    xv = x.view.view(n_rows, n_sym)
    sg = S.noise_sigma(points)
    for a, b in G.pieces(n_rows, 4):
        mp.map(payload[a:b] if sent is None else payload[sent[a:b]], n_sym, out=xv[a:b])
        xv[a:b] += sg * torch.view_as_complex(torch.randn((b - a, n_sym, 2), device=DEV, generator=gen))
    outs = {"bit_errors": Guarded("int32", n_rows, case["mis"]), "err_power": Guarded("float32", n_rows, case["mis"]),
            "ref_power": Guarded("float32", n_rows, case["mis"])}
    lm.reset()
    q = lm.measure(xv, payload, ref_row=ref, count=count, out={key: w.view for key, w in outs.items()})
    totals = lm.totals()
    be = q["bit_errors"]
    # 1. the windows
    rows = np.array(G.window_rows(geo["tiling"], n_sym, n_rows, 2))
    at = _index(rows)
    xw = _h(xv[at])
    rw = rows if ref is None else _h(ref[at])
    ok = (rows < n_live) & (rw >= 0) & (rw < n_rows)
    assert ok.sum() > len(rows) // 2
    pw = _h(payload[_index(np.where(ok, rw, 0))])
    want = M.measure(xw, points, rule, pw, np.where(ok, np.arange(len(rows)), -1))
    got = {key: _h(v[at]) for key, v in q.items()}
    assert np.all(got["bit_errors"][~ok] == -1) and not got["err_power"][~ok].any() and not got["ref_power"][~ok].any()
    dec = _h(mp.decode(xv[at]))                                                 # the same symbols on the device: exact, no guard
    assert np.array_equal(got["bit_errors"][ok], M.popcount_rows(dec[ok], pw[ok], n_sym, k))
    ung = _unguarded(points, rule, xw[ok])
    assert np.all(np.abs(got["bit_errors"][ok] - want["bit_errors"][ok]) <= k * ung)
    for key in ("err_power", "ref_power"):
        err = np.abs(got[key][ok].astype(np.float64) - want[key][ok])
        print("%s %s: worst error %.3f of the budget" % (case["id"], key, float(np.max(err / want[key][ok])) / M.BUDGET))
        assert np.all(err <= M.BUDGET * want[key][ok])
    # 2. the pieces: integer outputs and totals
    again = Guarded("int32", n_rows, 0)
    sums = []
    for a, b in G.pieces(n_rows):
        lm.reset()
        if ref is None:
            lm.measure(xv[a:b], payload[a:b], count=_live_part(count, a, b), out={"bit_errors": again.view[a:b]})
        else:
            lm.measure(xv[a:b], payload, ref_row=ref[a:b], count=_live_part(count, a, b), out={"bit_errors": again.view[a:b]})
        sums.append(lm.totals())
    assert _same(be, again.view)
    assert M.add_totals(*sums) == totals
    measured = int((be >= 0).sum())
    expect = int(((ref >= 0) & (ref < n_rows)).sum()) if ref is not None else n_live
    assert measured == expect and totals["rows"] == measured and totals["symbols"] == measured * n_sym and totals["bits"] == measured * n_sym * k
    assert totals["bit_errors"] == int(be.clamp_min(0).sum()) and totals["row_errors"] == int((be > 0).sum()) and 0 < totals["symbol_errors"] <= totals["bit_errors"]
    # 3.
    assert all(w.intact() for w in outs.values()) and again.intact() and x.intact()
    if count is not None:
        assert bool((be[n_live:] == -1).all()) and not q["err_power"][n_live:].any() and not q["ref_power"][n_live:].any()


# ---------------------------------------------------------------- channel model ----
def _check_sc16(got, y, budget, gain):
    """equal to q of the restatement except inside the guard band, where it may be one LSB off (tests/test_channel_model_gpu.py)"""
    want, guard = C.sc16(y, budget, gain)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert np.array_equal(got[~guard], want[~guard]) and d.max(initial=0) <= 1
    return int(guard.sum())


@pytest.mark.parametrize("case", G.CHANNEL_CASES, ids=G.case_id)
def test_channel(case):
    import torch
    import gfdm_amd
    geo = G.channel_geometry(case)
    n, T, sc16, offset = geo["n"], case["T"], case["sc16"], G.CHANNEL_OFFSET
    taps = np.array([1, 0.5, -0.25], np.complex64) if case["real"] else C.taps_for(T)
    assert taps.size == T and (not taps.imag.any()) == case["real"]
    gain = C.sc16_gain(T) if sc16 else 1.0
    ch = gfdm_amd.ChannelModel(case["s"], case["f"], 1.0, taps, case["seed"])
    hist = T - 1
    x = Guarded("complex64", hist + n, case["mis"])
    x.view.copy_(torch.view_as_complex(torch.randn((hist + n, 2), device=DEV, generator=_gen(case["seed"]))))
    per = 2 if sc16 else 1
    out = Guarded("int16" if sc16 else "complex64", n * per, case["mis"] * per)
    ch.apply(x.view, hist, offset, sc16=sc16, gain=gain, out=out.view)
    # 1. every window from the stream's own contract: its history and its offset
    worst, in_guard = 0.0, 0
    for a, b in G.stream_windows(geo["tiling"], 3):
        hw = min(T - 1, hist + a)
        y, budget = C.apply(_h(x.view[hist + a - hw:hist + b]), hw, taps, case["f"], case["s"], case["seed"], offset + a)
        got = _h(out.view[a * per:b * per])
        if sc16:
            in_guard += _check_sc16(got.reshape(-1, 2), y, budget, gain)
        else:
            share = C.share_of_budget(got, y, budget)
            worst = max(worst, share)
            assert share <= 1.0, (a, b, share)
    print("%s: worst error %.3f of the budget, %d components inside the sc16 guard band" % (case["id"], worst, in_guard))
    # 2. the stream cut by offset
    again = Guarded("int16" if sc16 else "complex64", n * per, 0)
    for a, b in G.pieces(n):
        hp = min(T - 1, hist + a)
        ch.apply(x.view[hist + a - hp:hist + b], hp, offset + a, sc16=sc16, gain=gain, out=again.view[a * per:b * per])
    assert _same(out.view, again.view)
    # 3.
    assert out.intact() and again.intact() and x.intact()


# ---------------------------------------------------------------- burst shaper ----
def _shaper_inputs(case, gen):
    """frames (n_frames, F) and their starts b S + jitter: every seventh frame back to back with its successor, zero fill elsewhere"""
    import torch
    geo = G.shaper_geometry(case)
    nF, F = geo["n_frames"], G.SHAPER_F
    frames = torch.view_as_complex(torch.randn((nF, F, 2), device=DEV, generator=gen))
    jitter = torch.randint(0, case["gap"] + 1, (nF,), device=DEV, generator=gen)
    jitter[3::7] = case["gap"]
    jitter[4::7] = 0
    starts = torch.arange(nF, device=DEV, dtype=torch.int64) * geo["S"] + jitter
    return geo, frames, starts


@pytest.mark.parametrize("case", G.SHAPER_CASES, ids=G.case_id)
def test_shaper_place(case):
    import gfdm_amd
    geo, frames, starts = _shaper_inputs(case, _gen(40))
    F, S_, nF, out_len, sc16, scale = G.SHAPER_F, geo["S"], geo["n_frames"], geo["out_len"], case["sc16"], case["scale"]
    n_live = int((starts < geo["tiling"].third_trip_cut()).sum()) if case["count"] else nF
    count = n_live if case["count"] else None
    sh = gfdm_amd.BurstShaper(F, scale=scale)
    per = 2 if sc16 else 1
    out = Guarded("int16" if sc16 else "complex64", out_len * per, case["mis"] * per)
    sh.place(frames, starts, out_len, count=count, sc16=sc16, out=out.view)
    # 1. the restatement on the windows: a real scale and a fixed gain, so equal
    for a, b in G.stream_windows(geo["tiling"], 4):
        b0, b1 = max(a // S_ - 1, 0), min(b // S_ + 1, nF)
        want = B.place_c64(_h(frames[b0:b1]), F, _h(starts[b0:b1]) - a, b - a, scale, _live_part(n_live, b0, b1))
        got = _h(out.view[a * per:b * per])
        assert np.array_equal(got.reshape(-1, 2), B.to_sc16_out(want, 1)) if sc16 else np.array_equal(got, want), (a, b)
    # 2. the stream cut between two slots
    again = Guarded("int16" if sc16 else "complex64", out_len * per, 0)
    for b0, b1 in G.pieces(nF):
        lo, hi = b0 * S_, out_len if b1 == nF else b1 * S_
        sh.place(frames[b0:b1], starts[b0:b1] - lo, hi - lo, count=_live_part(count, b0, b1), sc16=sc16, out=again.view[lo * per:hi * per])
    assert _same(out.view, again.view)
    # 3.
    assert out.intact() and again.intact()
    if count is not None:
        end = int(starts[n_live - 1]) + F
        assert 0 < n_live < nF and not _bits(out.view[end * per:]).any() and _bits(out.view[(end - 1) * per:end * per]).all()


@pytest.mark.parametrize("where", ["seeded", "first-trip", "last-trip-count"])
def test_shaper_peak(where):
    """the largest component of the live scaled frames, which normalised sc16 output leaves in the workspace, against torch's maximum in
    float64 over the same frames: a maximum is exact.  A lane keeps a running maximum over some ninety trips, so the value that decides
    lies in a trip of its own in every case: wherever the seeded data has it (printed), in a workgroup's first trip with ordinary
    values in all the later ones, and in the last live sample with a larger value right behind the count."""
    import torch
    import gfdm_amd
    case = G.SHAPER_CASES[0]
    geo, frames, starts = _shaper_inputs(case, _gen(41))
    nF, F = geo["n_frames"], G.SHAPER_F
    tiling = G.peak_geometry(nF)
    assert tiling.ntiles >= 2 * tiling.G + 1
    per_trip = tiling.G * tiling.t
    counted = where == "last-trip-count"
    n_live = 2 * nF // 3 + 1 if counted else nF
    if where == "first-trip":
        frames[0, 5] = complex(3.0, -40.0)
    elif counted:
        frames[n_live - 1, F - 1] = complex(3.0, -40.0)
        frames[n_live, 0] = complex(-1000.0, 2.0)
    sh = gfdm_amd.BurstShaper(F, scale=0.5)                                      # a power of two: the scaled values are exact
    out_len = 4099
    ws = Guarded("uint8", sh.workspace_bytes(nF, out_len))
    sh.place(frames, starts, out_len, count=n_live if counted else None, sc16=True, peak=30000.0, out=Guarded("int16", 2 * out_len).view, workspace=ws.view)
    res = ws.view[:8].view(torch.float32)
    size = (0.5 * torch.view_as_real(frames[:n_live]).double()).abs().amax(dim=2).view(-1)      # per live sample: the larger component of y
    top, at = float(size.max()), int(size.argmax())
    trips = -(-n_live * F // per_trip)
    print("%s: the maximum %.6f is sample %d of %d, trip %d of %d" % (where, top, at, n_live * F, at // per_trip, trips))
    assert {"seeded": 0 < at // per_trip < trips - 1, "first-trip": at == 5 and top == 20.0, "last-trip-count": at == n_live * F - 1 and top == 20.0}[where]
    assert float(res[1]) == top and float(res[0]) == float(B.gain(30000.0, np.float32(top)))
    assert ws.intact()


# ---------------------------------------------------------------- resampler ----
@pytest.mark.parametrize("case", G.RESAMPLER_CASES, ids=G.case_id)
def test_resampler(case):
    import torch
    import gfdm_amd
    geo = G.resampler_geometry(case)
    n_in, n_out, T, step, sc16 = geo["n_in"], geo["n_out"], case["T"], case["step"], case["sc16"]
    taps = Q.table_for(G.RESAMPLER_L, T)
    rs = gfdm_amd.Resampler(step, taps, interp="linear" if case["interp"] else "nearest")
    assert rs.plan(n_in, case["pos"])[0] == n_out
    per = 2 if sc16 else 1
    x = Guarded("int16" if sc16 else "complex64", n_in * per, case["mis"] * per)
    if sc16:
        x.view.copy_(torch.randint(-32768, 32768, (2 * n_in,), device=DEV, generator=_gen(50)).to(torch.int16))
    else:
        x.view.copy_(torch.view_as_complex(torch.randn((n_in, 2), device=DEV, generator=_gen(50))))
    out = Guarded("complex64", n_out, case["mis"])
    rs.resample(x.view, 0, case["pos"], out=out.view)
    # 1. every window from the stream's own contract: its pos and its history
    worst = 0.0
    for a, b in G.stream_windows(geo["tiling"], 5):
        b = min(b, n_out)
        first, hw, n, pos = G.resampler_window(case, a, b)
        xs = _h(x.view[first * per:min(first + n, n_in) * per])
        y, budget = Q.resample(Q.widen(xs) if sc16 else xs, hw, taps, case["interp"], step, pos, b - a)
        share = Q.share_of_budget(_h(out.view[a:b]), y, budget)
        worst = max(worst, share)
        assert share <= 1.0, (a, b, share)
    print("%s: worst error %.3f of the budget" % (case["id"], worst))
    # 2. the stream cut by plan()
    again = Guarded("complex64", n_out, 0)
    o = 0
    for start, hp, n, pos, n_piece, flush in G.resampler_chain(case, n_in):
        assert rs.plan(n, pos, flush)[0] == n_piece
        rs.resample(x.view[(start - hp) * per:(start + n) * per], hp, pos, flush=flush, out=again.view[o:o + n_piece])
        o += n_piece
    assert o == n_out and _same(out.view, again.view)
    # 3.
    assert out.intact() and again.intact() and x.intact()


# ---------------------------------------------------------------- convolutional code ----
@pytest.mark.parametrize("case", G.ENCODE_CASES, ids=G.case_id)
def test_cc_encode(case):
    import torch
    import gfdm_amd
    geo = G.encode_geometry(case)
    n_rows, n_info, unit, n_live = geo["n_rows"], case["n_info"], geo["unit"], geo["n_live"]
    count = n_live if case["count"] else None
    cc = gfdm_amd.ConvolutionalCode()
    assert cc.coded_bytes(n_info) == unit
    data = torch.randint(0, 256, (n_rows, geo["info_bytes"]), dtype=torch.uint8, device=DEV, generator=_gen(60))
    out = Guarded("uint8", n_rows * unit, case["mis"])
    cc.encode(data, n_info, count=count, out=out.view)
    whole = out.view.view(n_rows, unit)
    # 1.
    rows = np.array(G.window_rows(geo["tiling"], unit, n_rows, 6))
    want = V.encode(_h(data[_index(rows)]), n_info)
    want[rows >= n_live] = 0
    assert np.array_equal(_h(whole[_index(rows)]), want)
    # 2.
    again = Guarded("uint8", n_rows * unit, 0)
    parts = again.view.view(n_rows, unit)
    for a, b in G.pieces(n_rows):
        cc.encode(data[a:b], n_info, count=_live_part(count, a, b), out=parts[a:b])
    assert _same(whole, parts)
    # 3.
    assert out.intact() and again.intact()
    assert n_live == n_rows or (not whole[n_live:].any() and whole[:n_live].any())


@pytest.mark.parametrize("case", G.WS_DECODE_CASES, ids=G.case_id)
def test_cc_decode_in_the_workspace(case):
    """more rows than the workspace has slots: a wave decodes its second and third row into the slot of its first.  Soft input terminated,
    hard input truncated; integer arithmetic, so bytes and path_metric are equal or wrong.  The restatement is the window rule of check
    1: every row takes it ten seconds and more a case (2049 steps of array operations on 4101 x 64 states), the window rows -- under the
    waves 0, G - 1 | G, 2 G - 1 | 2 G, the last two, and 64 seeded ones -- a fraction of one."""
    import torch
    import gfdm_amd
    geo = G.ws_decode_geometry(case)
    n_rows, n_info, n_live, mode, hard = geo["n_rows"], geo["n_info"], geo["n_live"], case["mode"], case["hard"]
    count = n_live if case["count"] else None
    cc = gfdm_amd.ConvolutionalCode(V.POLYS, mode)
    assert cc.steps(n_info) == geo["steps"] and cc.workspace_bytes(n_info, n_rows) == 8 * geo["tpad"] * G.C("fec", "kWsWaves")
    gen = _gen(61)
    data = torch.randint(0, 256, (n_rows, (n_info + 7) // 8), dtype=torch.uint8, device=DEV, generator=gen)
    coded = cc.encode(data, n_info)                                             # a few hundred tiles: far below the encoder's bound
    weights = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=DEV)
    if hard:                                                                    # three coded bits in a hundred flipped
        flips = (torch.rand(coded.shape + (8,), device=DEV, generator=gen) < 0.03).to(torch.uint8)
        x = coded ^ (flips * weights).sum(dim=2).to(torch.uint8)
    else:                                                                       # test_conv_code_gpu.py's noisy LLRs: a good part saturates at gain 16
        bits = ((coded[:, :, None] & weights) != 0).view(n_rows, -1)[:, :2 * geo["steps"]]
        x = (4.0 * (1.0 - 2.0 * bits.float()) + 2.5 * torch.randn(bits.shape, device=DEV, generator=gen)).contiguous()
    ws = Guarded("uint8", cc.workspace_bytes(n_info, n_rows))
    out, pm = Guarded("uint8", n_rows * data.shape[1], 3), Guarded("int32", n_rows, 1)

    def decode(rows, cnt, o, p, workspace=None):
        if hard:
            cc.decode_hard(rows, n_info, count=cnt, out=o, path_metric=p, workspace=workspace)
        else:
            cc.decode(rows, n_info, 16.0, count=cnt, out=o, path_metric=p, workspace=workspace)

    decode(x, count, out.view, pm.view, ws.view)
    whole = out.view.view(n_rows, -1)
    # 1.
    rows = np.array(G.window_rows(geo["tiling"], 1, n_rows, 7))
    live = rows[rows < n_live]
    xw = _h(x[_index(live)])
    want, metric = V.decode_hard(xw, n_info, V.POLYS, mode) if hard else V.decode(xw, n_info, 16.0, V.POLYS, mode)
    assert np.array_equal(_h(pm.view[_index(live)]), metric) and np.array_equal(_h(whole[_index(live)]), want)
    errors = np.unpackbits(want ^ V.clean(_h(data[_index(live)]), n_info)).sum()
    print("%s: %d of %d information bits of the window rows wrong after decoding" % (case["id"], errors, live.size * n_info))
    # 2.
    again, pm2 = Guarded("uint8", n_rows * data.shape[1], 0), Guarded("int32", n_rows, 0)
    for a, b in G.pieces(n_rows):
        decode(x[a:b], _live_part(count, a, b), again.view.view(n_rows, -1)[a:b], pm2.view[a:b])
    assert _same(out.view, again.view) and _same(pm.view, pm2.view)
    # 3. the workspace ends where workspace_bytes says
    assert ws.intact() and out.intact() and pm.intact() and again.intact() and pm2.intact()
    if count is not None:
        assert not whole[n_live:].any() and not pm.view[n_live:].any() and whole[:n_live].any()
