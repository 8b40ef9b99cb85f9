"""CPU half of the grid-bound tests: the constants tests/grid_bound_cases.py mirrors still equal the `constexpr` of the sources, and every
case of tests/test_grid_bound_gpu.py, from those constants alone, makes its launch stride -- at least 2 G + 3 tiles, a short last
tile, three trips for the first workgroups and two for the rest -- with the tile edges G and 2 G inside the windows that are held to
the restatement.  Where the host picks the tile size (the resampler) the choice is restated and checked against its own rule."""
import numpy as np
import pytest

import grid_bound_cases as G
import resampler_ref as Q


@pytest.mark.parametrize("source", sorted(G.SOURCES))
def test_mirrored_constants_equal_the_sources(source):
    found = G.source_constants(source)
    mirrored = {name: value for (src, name), value in G.CONSTANTS.items() if src == source}
    assert mirrored, source
    for name, value in mirrored.items():
        assert name in found, "%s no longer defines %s as an integer constant" % (G.SOURCES[source], name)
        assert found[name] == value, "%s: %s is %d in the source, %d in tests/grid_bound_cases.py" % (G.SOURCES[source], name, found[name], value)


def test_the_issue_s_constants_are_all_mirrored():
    names = {name for (_, name) in G.CONSTANTS}
    assert {"kMaxTiles", "kMaxGroups", "kWsWaves", "kPeakParts", "kTile", "kTileSyms", "kTileVec", "GFDM_HIP_CC_LDS_STEPS"} <= names
    for source in ("symbols", "linkmeter", "channel", "shaper", "fec"):
        assert (source, "kMaxTiles") in G.CONSTANTS


def _strides(t, full=True):
    """what every case owes: enough tiles, a ragged end, three trips in front and two behind"""
    assert t.ntiles >= 2 * t.G + 1
    if full:
        assert 2 * t.G + 3 <= t.ntiles <= 2 * t.G + 4
        assert t.trips(0) == 3 and t.trips(t.ntiles - 2 * t.G - 1) == 3 and t.trips(t.ntiles - 2 * t.G) == 2 and t.trips(t.G - 1) == 2
    lo, hi = t.span(t.ntiles - 1)
    assert 0 < hi - lo < t.t and hi == t.total
    assert t.span(0)[0] == 0 and all(t.span(j)[1] == t.span(j + 1)[0] for j in (0, t.G - 1, t.G, 2 * t.G - 1, 2 * t.G))


def _edges_inside(ranges, t):
    """the elements on both sides of the tile edges G and 2 G lie in one of the ranges"""
    for m in (1, 2):
        e = t.edge(m)
        assert any(lo <= e - 1 and e < hi for lo, hi in ranges), (m, e)


def _row_case(geo, salt):
    t, unit, n_rows = geo["tiling"], geo["unit"], geo["n_rows"]
    _strides(t)
    straddles = geo.get("straddles", True)
    assert not straddles or (t.t % unit and unit % t.t), "a row length must not divide the tile"
    rows = G.window_rows(t, unit, n_rows, salt)
    _edges_inside(_merged(rows, unit), t)
    for m in (1, 2):
        assert not straddles or t.edge(m) % unit, "the edge %d G falls between two rows: no row straddles it" % m
        r = t.edge(m) // unit
        assert r in rows
    assert len(rows) >= G.N_RANDOM // 2 and rows[-1] == n_rows - 1 and rows[0] == 0
    if geo["n_live"] != n_rows:
        cut = geo["n_live"] * unit                      # the first element behind the live rows: in a third trip, spare rows behind it
        tile = (cut + t.mis) // t.t
        assert 2 * t.G <= tile < t.ntiles and 0 < geo["n_live"] < n_rows
    for a, b in G.pieces(n_rows):
        assert -(-((b - a) * unit + 16) // t.t) < t.G, "a piece must stay below G tiles"


def _merged(rows, unit):
    """runs of consecutive rows as element ranges"""
    out = []
    for r in rows:
        if out and out[-1][1] == r * unit:
            out[-1] = (out[-1][0], (r + 1) * unit)
        else:
            out.append((r * unit, (r + 1) * unit))
    return out


@pytest.mark.parametrize("case", G.MAP_CASES + G.DECODE_CASES + G.SOFT_CASES, ids=G.case_id)
def test_mapper_cases_stride(case):
    geo = G.mapper_geometry(case)
    _row_case(geo, 1)
    assert geo["straddles"] or (case["op"], case["n_sym"]) == ("decode", 5)
    assert geo["n_rows"] * geo["unit"] * (8 if case["op"] == "map" else 4 if case["op"] == "soft" else 1) < 2 ** 29      # <= 512 MiB an output


def test_mapper_cases_cover_the_templates():
    assert {(c["op"], c["k"]) for c in G.MAP_CASES + G.DECODE_CASES + G.SOFT_CASES} == {("map", 2), ("map", 6), ("decode", 2), ("decode", 6), ("soft", 2),
                                                                                        ("soft", 4)}
    for cases in (G.MAP_CASES, G.DECODE_CASES, G.SOFT_CASES):
        assert {c["n_sym"] for c in cases} >= {4099, 5} and any(c["mis"] for c in cases) and any(c["count"] for c in cases)


@pytest.mark.parametrize("case", G.METER_CASES, ids=G.case_id)
def test_meter_cases_stride(case):
    geo = G.meter_geometry(case)
    _row_case(geo, 2)
    assert geo["n_rows"] * case["n_sym"] < 2 ** 26


@pytest.mark.parametrize("case", G.CHANNEL_CASES, ids=G.case_id)
def test_channel_cases_stride(case):
    geo = G.channel_geometry(case)
    t = geo["tiling"]
    _strides(t)
    _edges_inside(G.stream_windows(t, 3), t)
    assert (G.CHANNEL_OFFSET + t.edge(1)) >> 1 > 2 ** 32                  # the Philox counter's high word is in use at the edges
    for a, b in G.pieces(geo["n"]):
        assert -(-(b - a + 4) // t.t) < t.G
    assert geo["n"] * 8 < 2 ** 29


@pytest.mark.parametrize("case", G.SHAPER_CASES, ids=G.case_id)
def test_shaper_cases_stride(case):
    geo = G.shaper_geometry(case)
    t = geo["tiling"]
    _strides(t)
    _edges_inside(G.stream_windows(t, 4), t)
    assert t.t > geo["S"] > G.SHAPER_F and t.t % geo["S"]                 # frames and zero fill alternate inside every tile
    for a, b in G.pieces(geo["n_frames"]):
        assert -(-((b - a) * geo["S"] + 4) // t.t) < t.G
    peak = G.peak_geometry(geo["n_frames"])
    assert peak.G == G.C("shaper", "kPeakParts") and peak.ntiles >= 2 * peak.G + 1 and geo["n_frames"] * G.SHAPER_F >= 2 ** 21
    assert geo["n_frames"] * G.SHAPER_F * 8 < 2 ** 29 and geo["out_len"] * (4 if case["sc16"] else 8) < 2 ** 29


@pytest.mark.parametrize("case", G.RESAMPLER_CASES, ids=G.case_id)
def test_resampler_cases_stride(case):
    geo = G.resampler_geometry(case)
    t = geo["tiling"]
    _strides(t)
    _edges_inside(G.stream_windows(t, 5), t)
    # the host's choice of the tile, restated: the input span of a tile fits the stage, one vector more would not (or the cap is reached)
    tv, T, step, stage = t.t // 2, case["T"], case["step"], G.C("resample", "kStage")
    span = lambda outputs: (((outputs - 1) * step + (1 << 32) - 1) >> 32) + 1 + (T - 1) + 1          # noqa: E731 (positions, windows, alignment)
    assert span(2 * tv) <= stage and (tv == G.C("resample", "kTileVecMax") or span(2 * (tv + 1)) > stage - 2)
    chain = G.resampler_chain(case, geo["n_in"])
    assert sum(p[4] for p in chain) == geo["n_out"] and all(-(-(p[4] + 2) // t.t) < t.G for p in chain)
    a, b = t.edge(1) - 100, t.edge(1) + 100
    first, hist, n, pos = G.resampler_window(case, a, b)
    idx, frac = Q.positions(step, pos, b - a)                              # the window's own positions, from its first sample on
    P = [case["pos"] + i * step for i in (a, b - 1)]
    assert [first + hist + int(idx[i]) for i in (0, -1)] == [p >> 32 for p in P] and [int(frac[i]) for i in (0, -1)] == [p & (Q.ONE - 1) for p in P]
    assert hist == min((T - 1) // 2, P[0] >> 32) and first + n == (P[1] >> 32) - (T - 1) // 2 + T


def test_resampler_cases_cover_the_templates():
    assert [(c["T"], c["interp"]) for c in G.RESAMPLER_CASES] == [(8, 0), (16, 1), (64, 1), (3, 0)]
    assert {2 * G.resampler_tile_vec(c["step"], c["T"]) for c in G.RESAMPLER_CASES} == {2048, 256}      # both tile sizes the host picks
    assert any(c["sc16"] for c in G.RESAMPLER_CASES) and any(c["mis"] for c in G.RESAMPLER_CASES)


@pytest.mark.parametrize("case", G.ENCODE_CASES, ids=G.case_id)
def test_encode_cases_stride(case):
    geo = G.encode_geometry(case)
    _row_case(geo, 6)
    assert geo["n_rows"] * geo["unit"] <= (2 * G.C("fec", "kMaxTiles") + 3) * 4096


@pytest.mark.parametrize("case", G.WS_DECODE_CASES, ids=G.case_id)
def test_workspace_decode_cases_stride(case):
    geo = G.ws_decode_geometry(case)
    t = geo["tiling"]
    assert geo["steps"] == G.C("header", "GFDM_HIP_CC_LDS_STEPS") + 1           # the shortest row that needs the workspace
    assert t.G == G.C("fec", "kWsWaves") and t.ntiles == case["trips"] * t.G + 5
    assert t.trips(0) == case["trips"] + 1 and t.trips(4) == case["trips"] + 1 and t.trips(5) == case["trips"]
    rows = G.window_rows(t, 1, geo["n_rows"], 7)
    assert all({m * t.G - 1, m * t.G} <= set(rows) for m in range(1, case["trips"] + 1)) and {0, geo["n_rows"] - 2, geo["n_rows"] - 1} <= set(rows)
    if case["count"]:
        assert case["trips"] * t.G < geo["n_live"] < geo["n_rows"]
    for a, b in G.pieces(geo["n_rows"], 3):
        assert b - a < t.G
    assert {(c["mode"], c["hard"]) for c in G.WS_DECODE_CASES} == {("terminated", False), ("truncated", True)}


def test_random_windows_are_seeded():
    assert G.random_rows(10 ** 6, 1) == G.random_rows(10 ** 6, 1) != G.random_rows(10 ** 6, 2)
    r = G.random_ranges(10 ** 7, 3)
    assert len(r) == G.N_RANDOM and all(b - a == G.RANGE for a, b in r) and r == G.random_ranges(10 ** 7, 3)
    assert np.all(np.diff([a for a, _ in r]) >= 0)
