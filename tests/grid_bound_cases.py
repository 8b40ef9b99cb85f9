"""Cases of the grid-bound tests (tests/test_grid_bound.py on the CPU, tests/test_grid_bound_gpu.py on the device): the device modules
bound their launch grid and stride over the rest of the work, and these cases are sized so that every workgroup takes a second tile and
the first ones a third.  Everything here is host arithmetic on the kernels' constants, which are MIRRORED below with their source; the
CPU test holds every one of them to the `constexpr` in that source, so a raised bound can never turn these tests back into single-trip
tests without notice, and it holds every case to "at least 2 G + 1 tiles, the windows contain the tile edges G and 2 G" from the
constants alone.  Nothing here calls the library.

A launch is described by a Tiling(G, t, total, mis): G workgroups, tiles of t output elements, `total` elements, the tile grid shifted
by `mis` elements against the data (the kernels tile 16-byte vectors aligned in MEMORY, so an output that starts mis elements behind a
16-byte boundary has its tile j at the elements [t j - mis, t (j + 1) - mis))."""
import ast
import operator
import os
import re

import numpy as np

import resampler_ref as Q

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SOURCES = {
    "symbols": "gr-gfdm_amd/csrc/gfdm_symbols.hip",
    "linkmeter": "gr-gfdm_amd/csrc/gfdm_linkmeter.hip",
    "channel": "gr-gfdm_amd/csrc/gfdm_channel.hip",
    "shaper": "gr-gfdm_amd/csrc/gfdm_shaper.hip",
    "resample": "gr-gfdm_amd/csrc/gfdm_resample.hip",
    "fec": "gr-gfdm_amd/csrc/gfdm_fec.hip",
    "header": "include/gfdm_hip.h",
}
# (source, name) -> value: what the cases below are built on
CONSTANTS = {
    ("symbols", "kLanes"): 256,                  # decode: a tile is kLanes * k bytes
    ("symbols", "kTileVec"): 1024,               # map, soft: 16-byte vectors per tile
    ("symbols", "kMaxTiles"): 8192,
    ("linkmeter", "kTileSyms"): 2048,
    ("linkmeter", "kMaxTiles"): 8192,
    ("channel", "kTile"): 2044,
    ("channel", "kMaxTiles"): 8192,
    ("shaper", "kLanes"): 256,
    ("shaper", "kTileVec"): 1024,
    ("shaper", "kMaxTiles"): 8192,
    ("shaper", "kPeakParts"): 1024,
    ("shaper", "kPeakPer"): 8,
    ("resample", "kTileVecMax"): 1024,
    ("resample", "kStage"): 2116,
    ("resample", "kMaxGroups"): 2048,
    ("fec", "kWaves"): 4,
    ("fec", "kTileVec"): 256,                    # encode: 16-byte vectors per tile
    ("fec", "kMaxTiles"): 8192,
    ("fec", "kWsWaves"): 2048,
    ("header", "GFDM_HIP_CC_LDS_STEPS"): 2048,
}


def C(source, name):
    return CONSTANTS[(source, name)]


_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.Div: operator.floordiv, ast.Mod: operator.mod,
        ast.LShift: operator.lshift, ast.RShift: operator.rshift}


class NotAnInteger(ValueError):
    """the expression is not integer arithmetic on known names"""


def int_expr(node, names):
    """the value of a parsed C integer expression: literals, known names, + - * / % << >> and a unary minus; / is C's division of
    non-negative integers"""
    if isinstance(node, ast.Expression):
        return int_expr(node.body, names)
    if isinstance(node, ast.Constant) and type(node.value) is int:
        return node.value
    if isinstance(node, ast.Name) and node.id in names:
        return names[node.id]
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
        return -int_expr(node.operand, names)
    if isinstance(node, ast.BinOp) and type(node.op) in _OPS:
        return _OPS[type(node.op)](int_expr(node.left, names), int_expr(node.right, names))
    raise NotAnInteger(ast.dump(node))


def parse_constants(text):
    """name -> int for every `constexpr <integer type> name = <expression>;` and `#define NAME <integer>` of a source whose expression is
    integer arithmetic on earlier ones (integer casts dropped); what is anything else (a sizeof, a call, a float) is left out, and a
    mirrored constant that is left out fails the CPU test by name"""
    found = {}
    for m in re.finditer(r"^\s*(?:static\s+)?constexpr\s+(?:unsigned\s+)?(?:int|int64_t|uint64_t|size_t|unsigned)\s+(\w+)\s*=\s*([^;]+);", text, re.M):
        expr = re.sub(r"\((?:u?int64_t|size_t|int|unsigned)\)", "", m.group(2)).strip()
        try:
            found[m.group(1)] = int_expr(ast.parse(expr, mode="eval"), found)
        except (SyntaxError, NotAnInteger):
            continue
    for m in re.finditer(r"^#define\s+(\w+)\s+(\d+)\b", text, re.M):
        found[m.group(1)] = int(m.group(2))
    return found


def source_constants(source):
    with open(os.path.join(ROOT, SOURCES[source])) as f:
        return parse_constants(f.read())


SEED = 20240         # of the random windows and of the device inputs
N_RANDOM = 64        # random rows, or random ranges of RANGE samples
RANGE = 4096


class Tiling:
    """G workgroups striding over ceil((total + mis) / t) tiles of t elements"""

    def __init__(self, G, t, total, mis=0):
        self.G, self.t, self.total, self.mis = int(G), int(t), int(total), int(mis)
        self.ntiles = -(-(self.total + self.mis) // self.t)

    def span(self, j):
        """the elements [lo, hi) of tile j"""
        return max(self.t * j - self.mis, 0), min(self.t * (j + 1) - self.mis, self.total)

    def trips(self, workgroup):
        return len(range(workgroup, self.ntiles, self.G))

    def edge(self, m):
        """the first element of tile m G: the edge between a workgroup's trips m and m + 1"""
        return self.t * self.G * m - self.mis

    def edge_tiles(self):
        return [0, self.G - 1, self.G, 2 * self.G - 1, 2 * self.G, self.ntiles - 2, self.ntiles - 1]

    def edge_ranges(self):
        """the element ranges of tiles 0, G - 1 and G, 2 G - 1 and 2 G and the last two, neighbours merged"""
        out = []
        for j in sorted(set(j for j in self.edge_tiles() if 0 <= j < self.ntiles)):
            lo, hi = self.span(j)
            if out and out[-1][1] >= lo:
                out[-1] = (out[-1][0], max(hi, out[-1][1]))
            else:
                out.append((lo, hi))
        return out

    def third_trip_cut(self):
        """an element inside tile 2 G + 1: where `count` ends the live rows, in a workgroup's third trip"""
        lo, hi = self.span(2 * self.G + 1)
        return (lo + hi) // 2


def sized(G, t, unit, mis=0):
    """the number of rows of `unit` elements that fills 2 G + 3 tiles less a ragged remainder; a row longer than the remainder is kept,
    so that there are never fewer than 2 G + 3 tiles (a row of 4099 symbols makes it 2 G + 4 where a tile is 2048)"""
    n = ((2 * G + 3) * t - mis - 1) // unit
    return n if n * unit + mis > (2 * G + 2) * t else n + 1


def rows_of(ranges, unit, n_rows):
    """the rows that the element ranges touch, ascending"""
    rows = set()
    for lo, hi in ranges:
        rows.update(range(lo // unit, min((hi - 1) // unit, n_rows - 1) + 1))
    return sorted(rows)


def random_rows(n_rows, salt):
    rng = np.random.default_rng([SEED, salt])
    return sorted(set(int(r) for r in rng.integers(0, n_rows, N_RANDOM)))


def random_ranges(n, salt, length=RANGE):
    rng = np.random.default_rng([SEED, salt])
    return [(int(a), int(a) + length) for a in sorted(rng.integers(0, n - length, N_RANDOM))]


def window_rows(tiling, unit, n_rows, salt):
    """check 1 of a row module: the rows under the edge tiles and N_RANDOM seeded ones"""
    return sorted(set(rows_of(tiling.edge_ranges(), unit, n_rows)) | set(random_rows(n_rows, salt)))


def pieces(n, parts=3):
    """[a, b) of `parts` nearly equal pieces of n rows or samples"""
    cuts = [n * p // parts for p in range(parts + 1)]
    return list(zip(cuts[:-1], cuts[1:]))


def case_id(c):
    return c["id"]


# ---- symbol mapper: gfdm_symbols.hip ----
def _mapper(op, name, k, n_sym, mis=0, count=False):
    return dict(id="%s-%s-n%d%s%s" % (op, name, n_sym, "-mis" if mis else "", "-count" if count else ""), op=op, name=name, k=k, n_sym=n_sym,
                mis=mis, count=count)


# map and decode at k = 2 (a sign rule) and k = 6 (NEAREST); soft at k = 2 and k = 4.  4099 symbols a row straddle tiles, 5 a row are the
# many-rows geometry; the latter carry the count and, but for map, the shifted output (2^24 - 1 is a multiple of 5: shifted by one symbol,
# map's edge G would fall between two rows).
MAP_CASES = [_mapper("map", "gr_qpsk", 2, 4099, 1), _mapper("map", "qam64", 6, 5, 0, True)]
# decode's rows of 5 symbols are 2 or 4 bytes, which divide its tile of 256 k bytes: a third case, rows of 9 symbols (7 bytes), gives the
# many-rows geometry rows that straddle the edges.
DECODE_CASES = [_mapper("decode", "gr_qpsk", 2, 4099), _mapper("decode", "qam64", 6, 5, 1, True), _mapper("decode", "qam64", 6, 9, 1, True)]
SOFT_CASES = [_mapper("soft", "gr_qpsk", 2, 4099), _mapper("soft", "qam16", 4, 5, 1, True)]


def mapper_geometry(c):
    """n_rows, the output row's elements (`unit`), its Tiling and the live rows of a mapper case.  map tiles the symbols (two a vector), soft
    the LLRs (four a vector), both aligned in memory; decode tiles the output bytes from the first one on, kLanes * k a tile."""
    k, n_sym = c["k"], c["n_sym"]
    G = C("symbols", "kMaxTiles")
    rb = (n_sym * k + 7) // 8
    if c["op"] == "map":
        unit, t, mis = n_sym, 2 * C("symbols", "kTileVec"), c["mis"]
    elif c["op"] == "soft":
        unit, t, mis = n_sym * k, 4 * C("symbols", "kTileVec"), c["mis"]
    else:
        unit, t, mis = rb, C("symbols", "kLanes") * k, 0
    n_rows = sized(G, t, unit, mis)
    tiling = Tiling(G, t, n_rows * unit, mis)
    n_live = tiling.third_trip_cut() // unit if c["count"] else n_rows
    # decode's rows of 5 symbols are 2 or 4 bytes, which divide every tile: there the edges fall between two rows whatever the shift
    return dict(n_rows=n_rows, unit=unit, row_bytes=rb, tiling=tiling, n_live=n_live, straddles=t % unit != 0)


# ---- link meter: gfdm_linkmeter.hip (tiles the flat symbol array from its first symbol on) ----
METER_CASES = [
    dict(id="qam16-n4099-ref_row", name="qam16", k=4, n_sym=4099, ref_row=True, mis=0, count=False),
    dict(id="gr_qpsk-n5-mis-count", name="gr_qpsk", k=2, n_sym=5, ref_row=False, mis=1, count=True),
]


def meter_geometry(c):
    G, t = C("linkmeter", "kMaxTiles"), C("linkmeter", "kTileSyms")
    n_rows = sized(G, t, c["n_sym"])
    tiling = Tiling(G, t, n_rows * c["n_sym"])
    n_live = tiling.third_trip_cut() // c["n_sym"] if c["count"] else n_rows
    return dict(n_rows=n_rows, unit=c["n_sym"], row_bytes=(c["n_sym"] * c["k"] + 7) // 8, tiling=tiling, n_live=n_live)


# ---- channel model: gfdm_channel.hip ----
CHANNEL_OFFSET = 2 ** 33 - 3
CHANNEL_CASES = [
    dict(id="c64-T3-real", sc16=False, T=3, real=True, f=0.002, s=1.0, mis=0, seed=31),
    dict(id="sc16-T64-complex-mis", sc16=True, T=64, real=False, f=1.0 / 3.0, s=1.0, mis=1, seed=32),
]


def channel_geometry(c):
    G, t = C("channel", "kMaxTiles"), C("channel", "kTile")
    n = sized(G, t, 1, c["mis"]) - t // 3
    return dict(n=n, tiling=Tiling(G, t, n, c["mis"]))


def stream_windows(tiling, salt):
    """check 1 of a stream module: the sample ranges of the edge tiles and N_RANDOM seeded ranges of RANGE samples"""
    return tiling.edge_ranges() + random_ranges(tiling.total, salt)


# ---- burst shaper: gfdm_shaper.hip ----
SHAPER_F = 257
SHAPER_CASES = [
    dict(id="c64-count", sc16=False, gap=100, mis=0, count=True, scale=0.5),
    dict(id="sc16-mis", sc16=True, gap=457, mis=1, count=False, scale=2048.0),
]


def shaper_geometry(c):
    """out_len and the slots of a place case: frame b starts at b S + jitter, jitter in [0, gap], S = F + gap, so zero fill and frames
    alternate in every tile and the stream can be cut at any b S"""
    G = C("shaper", "kMaxTiles")
    t = C("shaper", "kTileVec") * (4 if c["sc16"] else 2)
    out_len = sized(G, t, 1, c["mis"]) - t // 3
    S = SHAPER_F + c["gap"]
    return dict(out_len=out_len, S=S, n_frames=out_len // S, tiling=Tiling(G, t, out_len, c["mis"]))


def peak_geometry(n_frames):
    """k_shaper_peak: kPeakParts workgroups of kLanes lanes stride over the live frame samples, one sample a lane and trip"""
    parts, per = C("shaper", "kPeakParts"), C("shaper", "kLanes") * C("shaper", "kPeakPer")
    total = n_frames * SHAPER_F
    nparts = max(1, min(parts, -(-total // per)))
    return Tiling(nparts, C("shaper", "kLanes"), total)


# ---- resampler: gfdm_resample.hip ----
RESAMPLER_L = 128
RESAMPLER_CASES = [
    dict(id="T8-nearest-step1", T=8, interp=0, step=1 << 32, sc16=False, mis=0, pos=0),
    dict(id="T16-linear-step1.0001-mis", T=16, interp=1, step=round(1.0001 * 2 ** 32), sc16=False, mis=1, pos=(1 << 31) + 12345),
    dict(id="T64-linear-step8-sc16", T=64, interp=1, step=1 << 35, sc16=True, mis=0, pos=(3 << 32) + 77),
    dict(id="T3-nearest-step1over8", T=3, interp=0, step=1 << 29, sc16=False, mis=0, pos=5),
]


def resampler_tile_vec(step, T):
    """tile_vec_for of the host code, restated: the most output vectors whose input span fits kStage samples, at most kTileVecMax"""
    m = ((C("resample", "kStage") - T - 2) << 32) // step
    return int(max(1, min((m + 1) // 2, C("resample", "kTileVecMax"))))


def resampler_geometry(c):
    """n_in (flushed) and n_out = plan(n_in, pos) of a case, and the Tiling of its output"""
    G = C("resample", "kMaxGroups")
    t = 2 * resampler_tile_vec(c["step"], c["T"])
    want = sized(G, t, 1, c["mis"]) - t // 3
    n_in = (c["pos"] + want * c["step"]) >> 32
    n_out = Q.plan(c["step"], c["T"], c["pos"], n_in, True)[0]
    return dict(n_in=n_in, n_out=n_out, tiling=Tiling(G, t, n_out, c["mis"]))


def resampler_chain(c, n_in, parts=3):
    """the stream cut into `parts` pieces chained through plan: [(first sample, history, n_in, pos, n_out, flush)]"""
    D = (c["T"] - 1) // 2
    out, start, pos = [], 0, c["pos"]
    for p in range(parts):
        end = n_in if p == parts - 1 else n_in * (p + 1) // parts
        n = end - start
        n_out, advance, nxt = Q.plan(c["step"], c["T"], pos, n, p == parts - 1)
        out.append((start, min(D, start), n, pos, n_out, p == parts - 1))
        start, pos = start + advance, nxt
    return out


def resampler_window(c, a, b):
    """outputs [a, b) from the stream's own contract: (first input sample to pull, history, samples to pull, pos) such that
    resample(x[first:first + n], history, pos, n_out=b - a) is outputs a .. b - 1 of the call -- as far as the call's input reaches"""
    T = c["T"]
    D = (T - 1) // 2
    P = c["pos"] + a * c["step"]
    base = P >> 32
    history = min(D, base)
    last = (c["pos"] + (b - 1) * c["step"]) >> 32
    return base - history, history, last - D + T - (base - history), P - (base << 32)


# ---- convolutional code: gfdm_fec.hip ----
ENCODE_CASES = [
    dict(id="n456-mis", n_info=456, mis=1, count=False),
    dict(id="n3-count", n_info=3, mis=0, count=True),              # (2^26 - 1 is a multiple of 3: shifted by a byte, the edge 2 G would fall between two rows)
]


def encode_geometry(c):
    """terminated rows at their own width: the flat coded output is tiled in 16-byte vectors aligned in memory, kTileVec a tile"""
    G, t = C("fec", "kMaxTiles"), 16 * C("fec", "kTileVec")
    unit = (2 * (c["n_info"] + 6) + 7) // 8
    n_rows = sized(G, t, unit, c["mis"])
    tiling = Tiling(G, t, n_rows * unit, c["mis"])
    n_live = tiling.third_trip_cut() // unit if c["count"] else n_rows
    return dict(n_rows=n_rows, unit=unit, info_bytes=(c["n_info"] + 7) // 8, tiling=tiling, n_live=n_live)


WS_DECODE_CASES = [
    dict(id="terminated-soft-2053", mode="terminated", hard=False, trips=1, count=False),
    dict(id="terminated-soft-4101-count", mode="terminated", hard=False, trips=2, count=True),
    dict(id="truncated-hard-2053", mode="truncated", hard=True, trips=1, count=False),
    dict(id="truncated-hard-4101", mode="truncated", hard=True, trips=2, count=False),
]


def ws_decode_geometry(c):
    """the workspace variant: one wave and one workspace slot a row, kWsWaves of them, at the shortest row that needs the workspace"""
    G = C("fec", "kWsWaves")
    steps = C("header", "GFDM_HIP_CC_LDS_STEPS") + 1
    n_info = steps - (6 if c["mode"] == "terminated" else 0)
    n_rows = c["trips"] * G + 5
    tiling = Tiling(G, 1, n_rows)
    n_live = n_rows - 3 if c["count"] else n_rows              # ends inside the last trip
    return dict(n_rows=n_rows, n_info=n_info, steps=steps, tpad=-(-steps // 64) * 64, tiling=tiling, n_live=n_live)
