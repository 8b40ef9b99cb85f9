"""GPU tests of the burst synchroniser and extractor at the shapes their kernels treat differently (gfdm_burst.hip): odd and extreme
fft_len, cp_len of 0, around and well above the 256-position tile, windows of one live position, below one tile and of whole tiles,
and more than 32768 windows or bursts in one call (the kernels' second pass over blockIdx.y).  The expectation is the float64
restatement of the contract (ref_sync, ref_extract in tests/test_burst_gpu.py), which tests/test_burst.py holds against the pygfdm
fixtures at these shapes; the bounds are those of tests/test_burst_gpu.py.

A comparison of argmax positions counts only where the reference itself is decided: its best ic leads the second best by more than
1e-4, likewise its best |pcc| ic, and its nc is the planted core start -- asserted on the reference before the library is called."""
import functools

import numpy as np
import pytest

from burst_detect_ref import click_burst, top_margin
from conftest import have_gpu
from test_burst_gpu import ref_extract, ref_sync

pytestmark = pytest.mark.gpu
OUT = ("frame_start", "coarse", "cfo", "metric", "sc_rot")
MARGIN = 1e-4
TILE, MAX_GRID_Y = 256, 32768          # kTile, kMaxGridY


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def planted_window(K, cp, W, start, seed, cfo=0.2, clicks=True):
    """(window, core): noise 26 dB below a click_burst whose core preamble starts at `start`, with a CFO, rounded to complex64"""
    rng = np.random.default_rng(seed)
    burst, core = click_burst(K, cp, rng)
    if not clicks:
        burst = burst[1:-1]
    b0 = start - cp - (1 if clicks else 0)
    assert b0 >= 0 and b0 + burst.size <= W
    sigma = np.sqrt(10 ** -2.6 / 2)
    s = sigma * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    s[b0:b0 + burst.size] += burst * np.exp(1j * (2 * np.pi * rng.random() + 2 * np.pi * cfo / K * np.arange(burst.size)))
    return s.astype(np.complex64), core


def decided(ref, start, live=None):
    """the precondition on the reference alone; a window with one live position has nothing to decide"""
    if live == 1:
        return ref["nc"] == start
    return top_margin(ref["ic"]) > MARGIN and top_margin(ref["score"]) > MARGIN and ref["nc"] == start


def check_window(ref, K, ac, ic, r, i, first):
    """the bounds of tests/test_burst_gpu.py for window i of a result r against the restatement of that window"""
    if ac is not None:
        e_ac, e_ic = np.max(np.abs(ac - ref["ac"])), np.max(np.abs(ic - ref["ic"]))
        print("   ac err %.3e  ic err %.3e" % (e_ac, e_ic))
        assert e_ac < 1e-5 and e_ic < 1e-5
    print("   frame_start %d (%d) coarse %d (%d) cfo %+.6f (%+.6f) metric %.6f (%.6f)" % (
        r["frame_start"][i] - first, ref["nc"], r["coarse"][i] - first, ref["nm"], r["cfo"][i], ref["cfo"], r["metric"][i], ref["metric"]))
    assert int(r["frame_start"][i]) == first + ref["nc"] and int(r["coarse"][i]) == first + ref["nm"]
    assert abs(float(r["cfo"][i]) - ref["cfo"]) < 1e-4
    assert abs(float(r["metric"][i]) - ref["metric"]) < 1e-5
    rot = complex(r["sc_rot"][i])
    assert abs(abs(rot) - 1) < 1e-5 and abs(np.angle(rot) * K / (2 * np.pi) - float(r["cfo"][i])) < 1e-5


# K, cp_len, window_len, core start.  The start puts the cp_len positions before the maximum across as many tiles as the case is about.
SHAPES = [
    # odd and extreme fft_len
    (15, 7, 300, 131), (31, 16, 400, 260), (589, 100, 2100, 517), (2, 1, 90, 41), (1024, 512, 4300, 1290),
    # cp_len around the tile: 0 (ic = |ac|), either side of cp_len == tile, and halos of two and three segments
    (64, 0, 500, 261), (64, 255, 900, 513), (64, 256, 900, 513), (64, 257, 900, 513), (64, 300, 1000, 560), (64, 600, 1500, 1130),
    # window geometry at K = 16, cp_len = 8: one live position, P = 200 < tile, P = 256, 257, 512
    (16, 8, 41, 8), (16, 8, 232, 100), (16, 8, 288, 255), (16, 8, 289, 256), (16, 8, 544, 256),
]


@functools.lru_cache(maxsize=None)
def shape_case(K, cp, W, start):
    s, core = planted_window(K, cp, W, start, seed=1000 * K + cp + W, clicks=W > 2 * K + cp + 1)
    s.setflags(write=False)
    return s, core, ref_sync(s, core, K, cp)


@pytest.mark.parametrize("K,cp,W,start", SHAPES)
def test_sync_matches_restatement(K, cp, W, start):
    import torch
    import gfdm_amd
    s, core, ref = shape_case(K, cp, W, start)
    P = W - 2 * K
    print("K %d cp %d W %d: P %d, %d tile(s), ic margin %.2e, score margin %.2e, nc %d" % (
        K, cp, W, P, -(-P // TILE), top_margin(ref["ic"]), top_margin(ref["score"]), ref["nc"]))
    assert decided(ref, start, live=P - cp)
    sync = gfdm_amd.BurstSync(K, cp, core, W)
    assert sync.corr_len() == P
    ac, ic = sync.auto_correlate(s)
    r = sync.find_frame_start(s)
    check_window(ref, K, ac[0], ic[0], r, 0, 0)
    assert np.all(ic[0][:cp] == 0)
    ds = torch.tensor(s, device="cuda:0")
    dac, dic = sync.auto_correlate(ds)
    d = sync.find_frame_start(ds)
    torch.cuda.synchronize()
    assert np.array_equal(dac.cpu().numpy(), ac) and np.array_equal(dic.cpu().numpy(), ic)
    for k in OUT:
        assert np.array_equal(d[k].cpu().numpy(), r[k]), k


def test_window_in_a_stream_equals_the_window_alone():
    """the long-halo shape once more inside a longer stream at an odd first: tile_ic's halo segments stay inside the window"""
    import gfdm_amd
    K, cp, W, start = 64, 600, 1500, 1130
    s, core, ref = shape_case(K, cp, W, start)
    rng = np.random.default_rng(9)
    pad = (3.0 * (rng.standard_normal(777 + 333) + 1j * rng.standard_normal(777 + 333))).astype(np.complex64)      # loud neighbours
    stream = np.concatenate((pad[:777], s, pad[777:]))
    sync = gfdm_amd.BurstSync(K, cp, core, W)
    ac, ic = sync.auto_correlate(stream, first=777)
    ac1, ic1 = sync.auto_correlate(s)
    assert np.array_equal(ac, ac1) and np.array_equal(ic, ic1)
    r, r1 = sync.find_frame_start(stream, first=777), sync.find_frame_start(s)
    assert int(r["frame_start"][0]) == 777 + start
    for k in OUT:
        assert np.array_equal(r[k], r1[k] + (777 if k in ("frame_start", "coarse") else 0)), k


# ---- more than 32768 windows in one call ----
BIG = dict(K=8, cp=4, W=64, stride=3, n=MAX_GRID_Y + 37)


@functools.lru_cache(maxsize=None)
def big_stream():
    """(stream, core, core starts): about 98 500 samples, a short burst (the same core, its own CFO and phase) every 150 to 300 samples, and
    one every 44 samples around window 32768 and to the end: a window of 64 holds at most one whole burst of 22"""
    K, cp, W, stride, n = (BIG[k] for k in ("K", "cp", "W", "stride", "n"))
    rng = np.random.default_rng(11)
    N = (n - 1) * stride + W
    burst, core = click_burst(K, cp, rng)
    tail0 = MAX_GRID_Y * stride
    at = list(np.cumsum(rng.integers(150, 300, N // 150)))
    at = [int(a) for a in at if a + burst.size < tail0 - 500] + list(range(tail0 + 3 - 10 * 44, N - burst.size, 44))
    sigma = np.sqrt(10 ** -2.6 / 2)
    s = sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    for a in at:
        assert a + burst.size <= N
        s[a:a + burst.size] += burst * np.exp(1j * (2 * np.pi * rng.random() + 2 * np.pi * rng.uniform(-0.25, 0.25) / K * np.arange(burst.size)))
    s = s.astype(np.complex64)
    s.setflags(write=False)
    return s, core, np.array(at) + 1 + cp          # core starts


def _windows_to_check(s, core, starts):
    """up to 32 windows on either side of window 32768, nearest first, each holding one whole burst and decided in the reference"""
    K, cp, W, stride, n = (BIG[k] for k in ("K", "cp", "W", "stride", "n"))
    picked = []
    for side in (range(MAX_GRID_Y - 1, MAX_GRID_Y - 400, -1), range(MAX_GRID_Y, n)):
        got = 0
        for w in side:
            st = w * stride
            inside = starts[(starts - cp - 1 >= st) & (starts + 2 * K + 1 <= st + W)]
            if inside.size != 1 or got == 32:
                continue
            ref = ref_sync(s[st:st + W], core, K, cp)
            if decided(ref, int(inside[0]) - st):
                picked.append((w, ref))
                got += 1
    return picked


def test_more_windows_than_grid_rows():
    """n_windows > kMaxGridY: k_sync_ic and k_sync_fine stride over blockIdx.y, reusing their LDS tiles and block_argmax's slot"""
    import torch
    import gfdm_amd
    K, cp, W, stride, n = (BIG[k] for k in ("K", "cp", "W", "stride", "n"))
    s, core, starts = big_stream()
    sync = gfdm_amd.BurstSync(K, cp, core, W)
    ds = torch.tensor(s, device="cuda:0")
    big = sync.find_frame_start(s, stride=stride, n_windows=n)
    ac, ic = sync.auto_correlate(s, stride=stride, n_windows=n)
    # the same windows in calls that fit the grid
    lo = sync.find_frame_start(s, stride=stride, n_windows=MAX_GRID_Y)
    hi = sync.find_frame_start(s, first=MAX_GRID_Y * stride, stride=stride, n_windows=n - MAX_GRID_Y)
    ac_lo, ic_lo = sync.auto_correlate(s, stride=stride, n_windows=MAX_GRID_Y)
    ac_hi, ic_hi = sync.auto_correlate(s, first=MAX_GRID_Y * stride, stride=stride, n_windows=n - MAX_GRID_Y)
    for k in OUT:
        assert np.array_equal(big[k][:MAX_GRID_Y], lo[k]), k
        assert np.array_equal(big[k][MAX_GRID_Y:], hi[k]), k
    assert np.array_equal(ac[:MAX_GRID_Y], ac_lo) and np.array_equal(ic[:MAX_GRID_Y], ic_lo)
    assert np.array_equal(ac[MAX_GRID_Y:], ac_hi) and np.array_equal(ic[MAX_GRID_Y:], ic_hi)
    dev = sync.find_frame_start(ds, stride=stride, n_windows=n)
    dac, dic = sync.auto_correlate(ds, stride=stride, n_windows=n)
    torch.cuda.synchronize()
    for k in OUT:
        assert np.array_equal(dev[k].cpu().numpy(), big[k]), k
    assert np.array_equal(dac.cpu().numpy(), ac) and np.array_equal(dic.cpu().numpy(), ic)
    picked = _windows_to_check(s, core, starts)
    print("windows checked against the restatement:", len(picked), [w for w, _ in picked])
    assert len(picked) >= 48 and min(w for w, _ in picked) < MAX_GRID_Y <= max(w for w, _ in picked)
    for w, ref in picked:
        print("window", w)
        check_window(ref, K, ac[w], ic[w], big, w, w * stride)


def test_more_start_array_windows_than_grid_rows():
    """find_frame_start_at with 32768 + 37 starts: every window bit-equal to the regular-grid call on its start, on both paths and split"""
    import torch
    import gfdm_amd
    K, cp, W, stride, n = (BIG[k] for k in ("K", "cp", "W", "stride", "n"))
    s, core, _ = big_stream()
    sync = gfdm_amd.BurstSync(K, cp, core, W)
    perm = np.random.default_rng(5).permutation(n)
    st = (perm * stride).astype(np.int64)                       # the grid's windows in another order
    grid = sync.find_frame_start(s, stride=stride, n_windows=n)
    ds, dst = torch.tensor(s, device="cuda:0"), torch.tensor(st, device="cuda:0")
    at = sync.find_frame_start_at(ds, dst)
    at_lo = sync.find_frame_start_at(ds, dst[:MAX_GRID_Y].contiguous())
    at_hi = sync.find_frame_start_at(ds, dst[MAX_GRID_Y:].contiguous())
    torch.cuda.synchronize()
    host = sync.find_frame_start_at(s, st)
    for k in OUT:
        a = at[k].cpu().numpy()
        assert np.array_equal(a, grid[k][perm]), k
        assert np.array_equal(a[:MAX_GRID_Y], at_lo[k].cpu().numpy()) and np.array_equal(a[MAX_GRID_Y:], at_hi[k].cpu().numpy()), k
        assert np.array_equal(a, host[k]), k


# ---- extractor: more than 32768 bursts, burst_len == 1 ----
def _extract_inputs(n_s, nb, burst_len, seed):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(n_s) + 1j * rng.standard_normal(n_s)).astype(np.complex64)
    offsets = rng.integers(-burst_len - 5, n_s + burst_len + 5, nb).astype(np.int64)      # some bursts hang over either end, some lie outside
    scale = (0.5 + rng.random(nb)).astype(np.float32)
    rot = (np.exp(1j * 2 * np.pi * rng.uniform(-0.45, 0.45, nb) / 8) * (0.3 + rng.random(nb))).astype(np.complex64)
    rot[::97] = 0                                                                        # |r| = 0: no rotation
    return s, offsets, scale, rot


def test_extract_more_bursts_than_grid_rows():
    """n_bursts > kMaxGridY: k_extract strides over blockIdx.y and rewrites phi / rotate in LDS for every burst of a workgroup"""
    import torch
    import gfdm_amd
    burst_len, backoff, nb = 33, 5, MAX_GRID_Y + 7
    s, offsets, scale, rot = _extract_inputs(20000, nb, burst_len, 33)
    # the bursts that share a workgroup (b and b + 32768) differ in whether they rotate at all
    rot[:7] = 0
    assert np.all(rot[MAX_GRID_Y:] != 0)
    ex = gfdm_amd.BurstExtractor(burst_len, backoff, True)
    got = ex.extract(s, offsets, scale, rot)
    ref = ref_extract(s, offsets, burst_len, backoff, scale, rot, True)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("extract %d bursts of %d: rel err %.3e" % (nb, burst_len, err))
    assert got.shape == (nb, burst_len) and err < 2e-5
    past = ex.extract(s, offsets[MAX_GRID_Y:], scale[MAX_GRID_Y:], rot[MAX_GRID_Y:])
    first = ex.extract(s, offsets[:MAX_GRID_Y], scale[:MAX_GRID_Y], rot[:MAX_GRID_Y])
    assert np.array_equal(got[MAX_GRID_Y:], past) and np.array_equal(got[:MAX_GRID_Y], first)
    dev = ex.extract(torch.tensor(s, device="cuda:0"), torch.tensor(offsets, device="cuda:0"), torch.tensor(scale, device="cuda:0"),
                     torch.tensor(rot, device="cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), got)


def test_extract_burst_len_one():
    import torch
    import gfdm_amd
    nb = 300
    s, offsets, scale, rot = _extract_inputs(100, nb, 1, 1)
    for backoff in (0, 3):
        ex = gfdm_amd.BurstExtractor(1, backoff, True)
        got = ex.extract(s, offsets, scale, rot)
        ref = ref_extract(s, offsets, 1, backoff, scale, rot, True)
        assert got.shape == (nb, 1) and np.max(np.abs(got - ref)) / np.max(np.abs(ref)) < 2e-5
        outside = (offsets - backoff < 0) | (offsets - backoff >= s.size)
        assert outside.any() and np.all(got[outside] == 0) and np.all(got[~outside] != 0)
        dev = ex.extract(torch.tensor(s, device="cuda:0"), torch.tensor(offsets, device="cuda:0"), torch.tensor(scale, device="cuda:0"),
                         torch.tensor(rot, device="cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), got)


@pytest.mark.parametrize("sc16", [False, True])
def test_auto_correlate_host_with_one_output(sc16):
    """the raw C call with ac or ic left out (the Python wrapper always passes both): the output that is asked for equals the one of the
    both-outputs call bit for bit, nothing is written behind it (8-byte canary), and a call without any output is EINVAL"""
    import gfdm_amd
    K, cp, W, first, stride, nw = 4, 2, 24, 3, 5, 4
    P = W - 2 * K
    rng = np.random.default_rng(77)
    s = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex64)
    core = (rng.standard_normal(2 * K) + 1j * rng.standard_normal(2 * K)).astype(np.complex64)
    if sc16:
        s = gfdm_amd.to_sc16(s)
    s = np.ascontiguousarray(s)
    sync = gfdm_amd.BurstSync(K, cp, core, W)
    fn = getattr(gfdm_amd.capi.lib(), "gfdm_hip_burst_sync_auto_correlate%s_host" % ("_sc16" if sc16 else ""))
    CANARY = 0x5A

    def call(want_ac, want_ic):
        ac = np.full(nw * P * 8 + 8, CANARY, np.uint8)
        ic = np.full(nw * P * 4 + 8, CANARY, np.uint8)
        rc = fn(sync._h, ac.ctypes.data if want_ac else None, ic.ctypes.data if want_ic else None, s.ctypes.data, 64, first, stride, nw)
        assert np.all(ac[-8:] == CANARY) and np.all(ic[-8:] == CANARY)
        return rc, ac[:-8], ic[:-8]

    rc, ac, ic = call(True, True)
    assert rc == 0
    assert np.any(ac != CANARY) and np.any(ic != CANARY)
    wac, wic = sync.auto_correlate(s, first=first, stride=stride, n_windows=nw)          # ... and the wrapper's view of the same call
    assert np.array_equal(ac.view(np.complex64).reshape(nw, P), wac) and np.array_equal(ic.view(np.float32).reshape(nw, P), wic)
    rc, ac1, ic1 = call(True, False)
    assert rc == 0 and np.array_equal(ac1, ac) and np.all(ic1 == CANARY)
    rc, ac2, ic2 = call(False, True)
    assert rc == 0 and np.array_equal(ic2, ic) and np.all(ac2 == CANARY)
    rc, ac3, ic3 = call(False, False)
    assert rc == gfdm_amd.capi.EINVAL and np.all(ac3 == CANARY) and np.all(ic3 == CANARY)
