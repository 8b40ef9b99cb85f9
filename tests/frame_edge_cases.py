"""Frame geometries, subcarrier maps and frame layouts at the edges of the fused transmitter store stage (csrc/gfdm_tx.h) and of the
receivers' frame load / demapper store (RxIo), shared by tests/test_frame_edges.py (CPU: the expectations agree with each other and the
table covers every edge it claims) and tests/test_frame_edges_gpu.py (GPU: every kernel route, canaries around every output).

Routes, shapes, kernel names and creation contexts come from poison_cases.ROUTES; only the blocks per launch are this module's:
B = 2 bpw + 1, so that the first workgroup of a row-lane launch is full and the last one holds a single block.

Data as poison_cases.make_case: QPSK on the map, RRC taps, the three-tap channel H as f_eq, IC_ITER cancellation rounds."""
import functools

import numpy as np

import gfdm_ref as R
import poison_cases as P
from gfdm_amd.filters import get_frequency_domain_filter

TOL = P.TOL
ROW_WG = 256                                                     # GFDM_ROW_WG: threads of a row-lane workgroup below K = 128

TX_ROUTES = sorted(r for r in P.ROUTES if P.ROUTES[r]["modes"] == P.ALL)
RX_ROUTES = sorted(P.ROUTES)                                     # the two *_ic_mx routes run the IC receiver only
CPU_SHAPES = [(5, 32, 2), (7, 12, 2), (9, 64, 2)]


def bpw(route):
    """blocks per workgroup of the route's kernels: rowgeom::bpw(K) = wg(K) / K on the row-lane routes, one block per workgroup elsewhere"""
    K = P.ROUTES[route]["shape"][1]
    if not P.ROUTES[route]["kernel"].startswith("rowlane"):
        return 1
    return 1 if K >= 128 else ROW_WG // K


def blocks(route):
    return 2 * bpw(route) + 1


# ---------------------------------------------------------------- subcarrier maps

MAPS = ("tq", "one", "all", "ends")


def smap_of(name, K):
    """as passed to the constructors (`ends` unsorted: the library sorts it like the reference does)"""
    return {"tq": P.subcarrier_map(K), "one": np.array([K - 1]), "all": np.arange(K), "ends": np.array([K - 1, 0])}[name]


def active_map(K):
    """the symmetric three-quarter map the estimator tests use: A active subcarriers around DC, DC itself free"""
    A = 2 * ((3 * K // 4) // 2)
    return A, np.concatenate((np.arange(1, 1 + A // 2), np.arange(K - A // 2, K)))


# ---------------------------------------------------------------- transmitter geometries

def geometry(name, N):
    """cp, cs, ramp, plen, shifts and whether the window is given as its 2 * ramp taps only"""
    g = {
        "bare": dict(cp=0, cs=0, ramp=0, plen=0, shifts=[0], short_window=False),
        "ports8": dict(cp=5, cs=7, ramp=3, plen=11, shifts=list(range(8)), short_window=False),
        "seams": dict(cp=4, cs=2, ramp=9, plen=0, shifts=[0, 2], short_window=True),
        "wrap": dict(cp=0, cs=N, ramp=N, plen=1, shifts=[0, 3, N], short_window=True),
        "fullcp": dict(cp=N - 2, cs=2, ramp=1, plen=2, shifts=[0, 2], short_window=False),
    }[name]
    return dict(g, name=name)


GEOMETRIES = ("bare", "ports8", "seams", "wrap", "fullcp")


def tx_cases():
    """(geometry, map, per_timeslot, nin kind) of every transmitter case; nin kind: "one" 1, "short" A M - 1, "full" A M"""
    cases = [(g, "tq", True, "full") for g in GEOMETRIES if g != "ports8"]
    cases += [("ports8", m, per_ts, nin) for m in ("one", "all", "ends") for per_ts in (True, False) for nin in ("one", "short", "full")]
    return cases


def case_id(case):
    return "%s-%s-%s-%s" % (case[0], case[1], "ts" if case[2] else "sc", case[3])


def _c64_exact(rng, n):
    """n random complex numbers that float32 holds exactly"""
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64).astype(np.complex128)


def qpsk(rng, shape):
    return ((1 - 2 * rng.integers(0, 2, shape)) + 1j * (1 - 2 * rng.integers(0, 2, shape))) / np.sqrt(2)


@functools.lru_cache(maxsize=None)
def taps_of(M, K, L):
    taps = get_frequency_domain_filter("rrc", 0.4, M, K, L)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def tx_case(M, K, L, B, case):
    """constructor arguments, symbols and the float64 frames of every port of one transmitter case; shared, read-only"""
    gname, mname, per_ts, nin_kind = case
    N = M * K
    g = geometry(gname, N)
    rng = np.random.default_rng(1000 * K + 10 * M + GEOMETRIES.index(gname) + 7 * MAPS.index(mname))
    smap = smap_of(mname, K)
    A = len(smap)
    nin = {"one": 1, "short": A * M - 1, "full": A * M}[nin_kind]
    window_len = g["cp"] + N + g["cs"]
    window = _c64_exact(rng, 2 * g["ramp"] if g["short_window"] else window_len)
    preambles = [_c64_exact(rng, g["plen"]) for _ in g["shifts"]]
    sym = qpsk(rng, (B, nin))
    taps = taps_of(M, K, L)
    nt = R.normalize_taps(taps, M)
    block = R.modulate(R.map_to_resources(sym, M, K, smap, per_ts), nt, M, K, L)
    frames = [R.transmit(sym, nt, M, K, L, smap, per_ts, g["cp"], g["cs"], g["ramp"], window, s, preambles[p]) for p, s in enumerate(g["shifts"])]
    return P._freeze(dict(g, M=M, K=K, L=L, N=N, B=B, A=A, smap=smap, per_ts=per_ts, nin=nin, window=window, window_len=window_len,
                          preambles=preambles, sym=sym, taps=taps, nt=nt, block=block, frames=frames, F=g["plen"] + window_len))


def segments(c, port):
    """prefix, body and suffix of a frame of `port` as slices into the frame (behind the preamble)"""
    s = c["shifts"][port]
    scp, scs = c["cp"] + s, c["cs"] - s
    a = c["plen"]
    return {"prefix": slice(a, a + scp), "body": slice(a + scp, a + scp + c["N"]), "suffix": slice(a + scp + c["N"], a + scp + c["N"] + scs)}


def frames_by_definition(block, cp, cs, ramp, front, back, shift, preamble):
    """One frame per block, by definition (lib/add_cyclic_prefix_cc.cc:78-98, lib/transmitter_kernel.cc:92-107): the last cp + shift samples
    of the block, the block, its first cs - shift samples; the first `ramp` samples of that times `front`, the last `ramp` times `back`;
    the preamble in front.  Three slices and two multiplies, written out without oracle/gfdm_ref.py's add_cyclic_prefix."""
    x = np.asarray(block, dtype=np.complex128)
    N = x.shape[-1]
    scp, scs = cp + shift, cs - shift
    assert 0 <= scp <= N and 0 <= scs <= N and 2 * ramp <= cp + N + cs
    body = np.concatenate((x[..., N - scp:N], x[..., 0:N], x[..., 0:scs]), axis=-1)
    FL = body.shape[-1]
    assert FL == cp + N + cs
    body[..., 0:ramp] = body[..., 0:ramp] * np.asarray(front, dtype=np.complex128)
    body[..., FL - ramp:FL] = body[..., FL - ramp:FL] * np.asarray(back, dtype=np.complex128)
    pre = np.broadcast_to(np.asarray(preamble, dtype=np.complex128), body.shape[:-1] + (len(preamble),))
    return np.concatenate((pre, body), axis=-1)


def tx_predicates(c):
    """the edges one transmitter case reaches (names as in the coverage assertion of tests/test_frame_edges.py)"""
    N, K, smap = c["N"], c["K"], set(int(k) for k in c["smap"])
    scp = [c["cp"] + s for s in c["shifts"]]
    scs = [c["cs"] - s for s in c["shifts"]]
    return {
        "scs == 0": 0 in scs,
        "scp == N": N in scp,
        "scs == N": N in scs,
        "2*ramp == window_len": c["ramp"] > 0 and 2 * c["ramp"] == c["window_len"],
        "ramp > cp + shift": any(c["ramp"] > v for v in scp),
        "ramp > cs - shift": any(c["ramp"] > v for v in scs),
        "plen == 0": c["plen"] == 0,
        "F odd": c["F"] % 2 == 1,
        "nports == 8": len(c["shifts"]) == 8,
        "cp == 0 and cs == 0": c["cp"] == 0 and c["cs"] == 0,
        "A == 1": c["A"] == 1,
        "A == K": c["A"] == K,
        "0 in smap and K-1 in smap": 0 in smap and K - 1 in smap,
        "nin == 1": c["nin"] == 1,
    }


# ---------------------------------------------------------------- receiver frame layouts

def layout(name, N):
    """cp_len and frame_len of a receiver frame layout"""
    return {"plain": (0, N), "tight": (1, N + 1), "deep": (2 * N + 1, 2 * N + 1 + N + 2)}[name]


LAYOUTS = ("plain", "tight", "deep")


def rx_cases(mname):
    """(layout, use_map, per_timeslot, nout kind) of every receiver case on data of the map `mname`; nout kind: "one" 1, "short" A M - 1,
    "all".  The three-quarter map runs every layout, with and without the demapper; the other maps run `tight` with both symbol orders
    and every output size."""
    if mname == "tq":
        return [(lay, use_map, True, "all") for lay in LAYOUTS for use_map in (True, False)]
    return [("tight", True, per_ts, nout) for per_ts in (True, False) for nout in ("one", "short", "all")]


def rx_case_id(case):
    return "%s-%s-%s-%s" % (case[0], "map" if case[1] else "nomap", "ts" if case[2] else "sc", case[3])


def nout_of(kind, A, M):
    """(noutput_size argument or None, symbols per frame)"""
    return {"one": (1, 1), "short": (A * M - 1, A * M - 1), "all": (None, A * M)}[kind]


@functools.lru_cache(maxsize=None)
def rx_data(M, K, L, B, mname):
    """blocks behind the channel, f_eq and the float64 results of both receivers for QPSK on the map `mname`; shared, read-only"""
    if mname == "tq":
        c = P.make_case(M, K, L, B)
        return P._freeze(dict(M=M, K=K, L=L, N=c["N"], B=B, A=len(c["smap"]), smap=c["smap"], taps=c["taps"], nt=c["nt"], xe=c["xe"], feq=c["feq"],
                              ref_zf=c["ref_zf"], ref_ic=c["ref_ic"], keep_ic=c["keep_ic"]))
    rng = np.random.default_rng(100 * K + 10 * M + L + 1000 * MAPS.index(mname))
    N = M * K
    taps = taps_of(M, K, L)
    nt = R.normalize_taps(taps, M)
    smap = smap_of(mname, K)
    d = np.zeros((B, K, M), complex)
    d[:, smap, :] = qpsk(rng, (B, len(smap), M))
    x = R.modulate(d.reshape(B, N), nt, M, K, L)
    feq = np.fft.fft(P.H, N)[None, :] * np.ones((B, 1))
    xe = np.fft.ifft(np.fft.fft(x, axis=-1) * feq, axis=-1)
    ref_ic, st = R.advanced_receive(xe, nt, M, K, L, smap, R.qpsk_points(), P.IC_ITER, f_eq=feq, kind="qpsk", return_stages=True)
    return P._freeze(dict(M=M, K=K, L=L, N=N, B=B, A=len(smap), smap=smap, taps=taps, nt=nt, xe=xe, feq=feq,
                          ref_zf=R.demodulate(xe, nt, M, K, L, feq), ref_ic=ref_ic, keep_ic=P.guarded(st, smap, K, M)))


def rx_expected(d, ref, case):
    """what a receiver writes for `case`: (B, nout) from the (B, N) float64 result `ref`"""
    _, use_map, per_ts, kind = case
    if not use_map:
        return ref
    _, n = nout_of(kind, d["A"], d["M"])
    return R.demap_from_resources(ref, d["M"], d["K"], d["smap"], per_ts, n)


def rx_predicates(d, case):
    cp, frame_len = layout(case[0], d["N"])
    smap = set(int(k) for k in d["smap"])
    return {
        "frame_len == cp + N": frame_len == cp + d["N"],
        "cp == 0": cp == 0,
        "cp > N": cp > d["N"],
        "noutput_size == 1": case[1] and case[3] == "one",
        "A == 1": case[1] and d["A"] == 1,
        "A == K": case[1] and d["A"] == d["K"],
        "0 in smap and K-1 in smap": case[1] and 0 in smap and d["K"] - 1 in smap,
    }


# ---------------------------------------------------------------- estimated layouts

EST_LAYOUTS = ("pre_front", "pre_back", "packed")


def estimator_inputs(M, K, B, rng):
    """known preamble (flat spectrum, two identical halves) and every block's received preamble behind the channel H, complex64"""
    pre = np.tile(np.fft.ifft(np.exp(2j * np.pi * rng.random(K))) * np.sqrt(K), 2)
    gains = np.exp(0.3j * np.arange(B)) * (1 + 0.02 * np.arange(B))
    rx_pre = np.tile(np.fft.ifft(np.fft.fft(pre[:K]) * np.fft.fft(P.H, K)), 2)[None, :] * gains[:, None]
    return pre, (rx_pre + 1e-3 * (rng.standard_normal((B, 2 * K)) + 1j * rng.standard_normal((B, 2 * K)))).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def est_data(M, K, L, B):
    """the case's blocks, the preambles, the estimated equaliser and both receivers' float64 results on the symmetric map; read-only"""
    c = P.make_case(M, K, L, B)
    A, smap = active_map(K)
    pre, rx_pre = estimator_inputs(M, K, B, np.random.default_rng(K + M))
    feq = R.estimate_frame(rx_pre, pre.astype(np.complex64), M, K, A, True)
    ref_ic, st = R.advanced_receive(c["xe"], c["nt"], M, K, L, smap, R.qpsk_points(), P.IC_ITER, f_eq=feq, kind="qpsk", return_stages=True)
    ref_zf = R.demodulate(c["xe"], c["nt"], M, K, L, feq)
    dm = lambda r: R.demap_from_resources(r, M, K, smap, True)
    return P._freeze(dict(M=M, K=K, L=L, N=c["N"], B=B, A=A, smap=smap, taps=c["taps"], xe=c["xe"], pre=pre, rx_pre=rx_pre,
                          want_zf=dm(ref_zf), want_ic=dm(ref_ic), keep_ic=P.guarded(st, smap, K, M)))


def est_frames(d, name, rng):
    """(frames (B, frame_len) complex64, cp_len, frame_len, offset of preamble 0 in the flat frames or None, preamble_stride) of an
    estimated layout; the single cp sample of every frame is random junk"""
    B, N, K = d["B"], d["N"], d["K"]
    xe, rx_pre = np.asarray(d["xe"]).astype(np.complex64), np.asarray(d["rx_pre"])
    junk = (rng.standard_normal((B, 1)) + 1j * rng.standard_normal((B, 1))).astype(np.complex64)
    if name == "pre_front":                                       # [pre 2K | cp = 1 | block], rx_preamble = frames
        return np.concatenate((rx_pre, junk, xe), axis=1), 2 * K + 1, 2 * K + 1 + N, 0, 2 * K + 1 + N
    if name == "pre_back":                                        # [cp = 1 | block | pre 2K]: the last preamble ends the buffer
        return np.concatenate((junk, xe, rx_pre), axis=1), 1, 1 + N + 2 * K, 1 + N, 1 + N + 2 * K
    return np.concatenate((junk, xe), axis=1), 1, 1 + N, None, 0  # packed, separate preambles
