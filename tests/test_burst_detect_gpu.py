"""GPU tests of the burst detector (gfdm_hip_burst_sync_detect) and of find_frame_start_at: against the pygfdm fixtures of
tests/golden/detect (make_golden_detect.py) and the float64 restatement of the contract (tests/burst_detect_ref.py), against the
existing regular-grid calls (bit-equal), under a different tiling, with too few and too many output slots, and in front of the
extractor and the estimated IC receiver with every step on the device; and on synthetic streams at odd fft_len, at cp_len of 0 and on
either side of the 256-position segment (where the scan changes from segment_ic to tile_ic), and with a +-min_distance halo of eight
segments, against the restatement alone, which tests/test_burst.py holds against pygfdm at such shapes."""
import functools

import numpy as np
import pytest

import gfdm_ref as R
from burst_detect_ref import click_burst, detect_names, load_detect, nms_maxima, ref_ac_ic, ref_detect, ref_peaks, top_margin
from conftest import have_gpu
from gfdm_amd.filters import get_frequency_domain_filter

pytestmark = pytest.mark.gpu
OUT = ("frame_start", "coarse", "cfo", "metric", "sc_rot")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _sync(g):
    import gfdm_amd
    return gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], g["window_len"])


def _detect(sync, g, s=None, **kw):
    return sync.detect(g["stream"] if s is None else s, g["threshold"], g["min_distance"], g["lead"], **kw)


def _to_host(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


def _assert_sentinels(r, lo):
    assert np.all(r["frame_start"][lo:] == -1) and np.all(r["coarse"][lo:] == -1)
    assert np.all(r["cfo"][lo:] == 0) and np.all(r["metric"][lo:] == 0) and np.all(r["sc_rot"][lo:] == 0)


@pytest.mark.parametrize("name", detect_names())
def test_detect_matches_pygfdm(name):
    g = load_detect(name)
    sync = _sync(g)
    r = _detect(sync, g)
    P = g["stream"].size - 2 * g["K"]
    assert r["frame_start"].size == -(-P // (g["min_distance"] + 1))          # the default max_bursts
    ref = ref_detect(g["stream"], g["preamble"], g["K"], g["cp_len"], g["window_len"], g["threshold"], g["min_distance"], g["lead"])
    n = g["peaks"].size
    print(name, "count", r["count"], "coarse", r["coarse"][:n], "reference", g["peaks"])
    assert r["count"] == n
    _assert_sentinels(r, n)
    for i in range(n):
        d, d_ref = int(r["coarse"][i]), int(g["peaks"][i])
        if d != d_ref:                  # as for the synchroniser: a neighbour only where the reference ic is flat to 1e-5
            assert abs(d - d_ref) == 1 and abs(ref["ic"][d] - ref["ic"][d_ref]) < 1e-5
        assert int(r["frame_start"][i]) == int(g["core_starts"][i])
        print("  burst %d: cfo %+.6f (pygfdm %+.6f)  metric %.6f (pygfdm %.6f)" % (i, r["cfo"][i], g["cfo"][i], r["metric"][i], g["metric"][i]))
        assert abs(float(r["cfo"][i]) - float(g["cfo"][i])) < 1e-4
        assert abs(float(r["metric"][i]) - float(g["metric"][i])) < 1e-5
        rot = complex(r["sc_rot"][i])
        assert abs(abs(rot) - 1) < 1e-5 and abs(np.angle(rot) * g["K"] / (2 * np.pi) - float(r["cfo"][i])) < 1e-5
    if n == 0:
        assert r["frame_start"].size > 0          # noise only: every slot at its sentinel (checked above)


@pytest.mark.parametrize("name", detect_names())
def test_peaks_are_the_rule_on_the_librarys_own_ic(name):
    """the scan's ic is auto_correlate's, bit for bit: the peak rule applied to that fp32 ic gives exactly detect's positions"""
    g = load_detect(name)
    import gfdm_amd
    s = g["stream"]
    whole = gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], s.size)          # the stream as one window
    _, ic = whole.auto_correlate(s)
    last = s.size - g["window_len"]
    for thr in (g["threshold"], 0.2, 0.12):                                          # lower thresholds: noise peaks too
        r = _sync(g).detect(s, thr, g["min_distance"], g["lead"])
        peaks = ref_peaks(ic[0].astype(np.float64), float(np.float32(thr)), g["min_distance"])
        assert r["count"] == peaks.size, thr
        free = np.flatnonzero((peaks >= g["lead"]) & (peaks - g["lead"] <= last))      # coarse == peak is promised away from a clamped window only
        assert free.size >= peaks.size - 2
        assert np.array_equal(r["coarse"][free], peaks[free]) and np.array_equal(r["metric"][free], ic[0][peaks[free]]), thr


@pytest.mark.parametrize("name", detect_names())
def test_host_and_device_paths_are_bit_equal(name):
    import torch
    g = load_detect(name)
    sync = _sync(g)
    r = _detect(sync, g)
    d = _detect(sync, g, torch.tensor(g["stream"], device="cuda:0"))
    torch.cuda.synchronize()
    assert d["count"].dtype == torch.int64 and int(d["count"][0]) == r["count"]
    d = _to_host(d)
    for k in OUT:
        assert np.array_equal(d[k], r[k]), k


@pytest.mark.parametrize("name", detect_names())
def test_detect_equals_the_existing_calls(name):
    import torch
    g = load_detect(name)
    sync = _sync(g)
    r = _detect(sync, g)
    n = r["count"]
    if n == 0:
        return
    starts = r["coarse"][:n] - g["lead"]                            # find_frame_start_at clamps them as detect does
    at = sync.find_frame_start_at(g["stream"], starts)
    ds = torch.tensor(g["stream"], device="cuda:0")
    at_dev = _to_host(sync.find_frame_start_at(ds, torch.tensor(starts, device="cuda:0")))
    last = g["stream"].size - g["window_len"]
    for k in OUT:
        assert np.array_equal(at[k], r[k][:n]), k
        assert np.array_equal(at_dev[k], at[k]), k
    for w in range(n):
        one = sync.find_frame_start(g["stream"], first=int(np.clip(starts[w], 0, last)))
        for k in OUT:
            assert np.array_equal(one[k], at[k][w:w + 1]), (w, k)


@pytest.mark.parametrize("name", ["k64_12b", "k32_cp32_14b", "k256_4b"])
def test_detect_does_not_depend_on_tiling(name):
    """a sub-span starts its tiles elsewhere: the detections whose windows lie R + cp_len inside it are those of the whole stream"""
    g = load_detect(name)
    sync = _sync(g)
    whole = _detect(sync, g)
    W, edge = g["window_len"], g["min_distance"] + g["cp_len"]
    n = g["stream"].size
    checked = 0
    for a, b in ((301, n - 77), (n // 3 + 5, n), (0, 2 * n // 3 + 1), (1111, n // 2 + 1500)):
        sub = _detect(sync, g, g["stream"][a:b])

        def inside(r, shift):
            st = r["coarse"][:min(r["count"], r["coarse"].size)] + shift - g["lead"]
            return np.flatnonzero((st >= a + edge) & (st + W <= b - edge))
        iw, isub = inside(whole, 0), inside(sub, a)
        assert iw.size == isub.size
        checked += iw.size
        for k in OUT:
            shift = a if k in ("frame_start", "coarse") else 0
            assert np.array_equal(sub[k][isub] + shift, whole[k][iw]), (a, b, k)
    assert checked >= 3


@pytest.mark.parametrize("per", [8, 16])
def test_detect_on_a_long_stream(per):
    """The scan gives a lane 4 to 16 positions of a tile, by the stream length: per = clamp(ceil(P / (256 * 4096)), 4, 16) (detect_geom,
    kScanTiles in gfdm_burst.hip).  The fixtures run at 4; these streams of about 8 and 16 million samples, bursts throughout, run at 8 and
    16 -- against the peak rule on auto_correlate's ic, and every copy's true core starts."""
    import torch
    import gfdm_amd
    g = load_detect("k64_12b")
    K, cp, Rd, lead = g["K"], g["cp_len"], g["min_distance"], g["lead"]
    seg = 256 * 4096
    reps = ((per - 1) * seg + seg // 2) // g["stream"].size + 1
    rng = np.random.default_rng(5)
    s = np.tile(g["stream"], reps)
    s += (0.05 * (rng.standard_normal(s.size, np.float32) + 1j * rng.standard_normal(s.size, np.float32))).astype(np.complex64)
    P = s.size - 2 * K
    assert min(16, max(4, -(-P // seg))) == per
    ds = torch.tensor(s, device="cuda:0")
    whole = gfdm_amd.BurstSync(K, cp, g["preamble"], s.size)
    _, ic = whole.auto_correlate(ds)
    ic = ic[0].cpu().numpy()
    sync = _sync(g)
    r = _to_host(sync.detect(ds, g["threshold"], Rd, lead))
    peaks = ref_peaks(ic.astype(np.float64), float(np.float32(g["threshold"])), Rd)
    n = int(r["count"][0])
    print("per", per, "samples", s.size, "count", n, "rule", peaks.size, "bursts", reps * g["peaks"].size)
    assert n == peaks.size == reps * g["peaks"].size
    assert np.array_equal(r["coarse"][:n], peaks) and np.array_equal(r["metric"][:n], ic[peaks])
    _assert_sentinels(r, n)
    # the true core starts of every copy (the copies' seams and the extra noise do not move the fine timing)
    truth = (np.arange(reps)[:, None] * g["stream"].size + g["core_starts"][None, :]).ravel()
    bad = np.flatnonzero(r["frame_start"][:n] != truth)
    print("frame starts off the truth:", bad.size, r["frame_start"][:n][bad][:10], truth[bad][:10])
    assert bad.size == 0


@pytest.mark.parametrize("period,n", [(50, 5000), (300, 9000)])
def test_equal_values_first_index_wins(period, n):
    """A stream that repeats with `period` has bit-equal ic at every distance of a period.  With min_distance = period each maximum is
    beaten by its equal one period before (>= on the left) and the very first one is not beaten by its equals after it (> on the right):
    one peak.  With min_distance = period - 1 the equals are out of reach: a peak every period.  Ties fall across segments and tiles."""
    import gfdm_amd
    K, cp, lead = 64, 32, 40
    rng = np.random.default_rng(period)
    blockv = (rng.standard_normal(period) + 1j * rng.standard_normal(period)).astype(np.complex64)
    s = np.tile(blockv, n // period + 1)[:n]
    pre = np.tile(np.exp(2j * np.pi * rng.random(K)), 2)
    whole = gfdm_amd.BurstSync(K, cp, pre, n)
    _, ic = whole.auto_correlate(s)
    ic = ic[0]
    P = n - 2 * K
    assert np.array_equal(ic[cp:P - period], ic[cp + period:P]) and ic[cp:].min() > 1e-3          # the ties are exact
    sync = gfdm_amd.BurstSync(K, cp, pre, 2 * K + lead + period - 1)                               # W - 2K - lead - 1 == period - 2
    thr = 1e-3
    first = cp + int(np.argmax(ic[cp:cp + period]))
    assert np.count_nonzero(ic[cp:cp + period] == ic[first]) == 1
    one = sync.detect(s, thr, period, lead)
    assert one["count"] == 1 and one["metric"][0] == ic[first]
    assert list(ref_peaks(ic.astype(np.float64), thr, period)) == [first]
    if first >= lead:
        assert int(one["coarse"][0]) == first
    many = sync.detect(s, thr, period - 1, lead)
    expect = ref_peaks(ic.astype(np.float64), thr, period - 1)
    assert np.array_equal(expect[:-1], first + period * np.arange(expect.size - 1)) and expect.size >= (P - cp) // period
    assert many["count"] == expect.size
    free = np.flatnonzero((expect >= lead) & (expect - lead <= n - sync.window_len()))
    assert free.size >= expect.size - 2 and np.array_equal(many["coarse"][free], expect[free])
    assert np.all(many["metric"][free] == ic[first])


def test_overflow_and_spare_slots():
    import torch
    g = load_detect("k64_12b")
    sync = _sync(g)
    full = _detect(sync, g)
    n = full["count"]
    assert n == 12
    ds = torch.tensor(g["stream"], device="cuda:0")
    for s in (g["stream"], ds):
        few = _to_host(_detect(sync, g, s, max_bursts=n - 3))
        assert int(np.asarray(few["count"]).ravel()[0]) == n            # the total, though only n - 3 fit
        for k in OUT:
            assert few[k].size == n - 3 and np.array_equal(few[k], full[k][:n - 3]), k      # the lowest positions, in order
        spare = _to_host(_detect(sync, g, s, max_bursts=n + 5))
        assert int(np.asarray(spare["count"]).ravel()[0]) == n
        for k in OUT:
            assert np.array_equal(spare[k][:n], full[k][:n]), k
        _assert_sentinels(spare, n)
        none = _to_host(_detect(sync, g, s, max_bursts=0))
        assert int(np.asarray(none["count"]).ravel()[0]) == n and none["frame_start"].size == 0
    huge = _detect(sync, g, max_bursts=100000)                           # more slots than the stream has positions
    assert huge["count"] == n and np.array_equal(huge["coarse"][:n], full["coarse"][:n])
    _assert_sentinels(huge, n)


def test_find_frame_start_at_clamps_its_starts():
    import torch
    g = load_detect("k64_cut_10b")
    sync = _sync(g)
    s = g["stream"]
    last = s.size - g["window_len"]
    starts = np.array([-1, -10 ** 12, 0, 5, last, last + 1, last + 4000, 10 ** 15, 700, np.iinfo(np.int64).min, np.iinfo(np.int64).max], np.int64)
    got = sync.find_frame_start_at(s, starts)
    ref = sync.find_frame_start_at(s, np.clip(starts, 0, last))
    dev = _to_host(sync.find_frame_start_at(torch.tensor(s, device="cuda:0"), torch.tensor(starts, device="cuda:0")))
    for k in OUT:
        assert np.array_equal(got[k], ref[k]) and np.array_equal(dev[k], ref[k]), k
    assert np.all(got["coarse"] >= 0) and np.all(got["coarse"] < s.size)
    for w, st in enumerate(np.clip(starts, 0, last)):
        one = sync.find_frame_start(s, first=int(st))
        for k in OUT:
            assert np.array_equal(one[k], got[k][w:w + 1]), (w, k)
    assert sync.find_frame_start_at(s, np.zeros(0, np.int64))["frame_start"].size == 0
    with pytest.raises(ValueError, match="stream_len"):
        sync.find_frame_start_at(s[:g["window_len"] - 1], [0])
    with pytest.raises(TypeError, match="starts"):
        sync.find_frame_start_at(torch.tensor(s, device="cuda:0"), torch.tensor([0], dtype=torch.int32, device="cuda:0"))


def test_detect_argument_errors():
    import gfdm_amd
    g = load_detect("k64_12b")
    sync = _sync(g)
    s, W, K, cp = g["stream"], g["window_len"], g["K"], g["cp_len"]
    for kw, match in ((dict(threshold=0.45, min_distance=256, lead=cp - 1), "lead"),
                      (dict(threshold=0.45, min_distance=256, lead=257), "lead"),
                      (dict(threshold=0.45, min_distance=W - 2 * K - 64 - 2, lead=64), "min_distance"),
                      (dict(threshold=0.0, min_distance=256, lead=64), "threshold"),
                      (dict(threshold=0.45, min_distance=256, lead=64, max_bursts=-1), "max_bursts")):
        with pytest.raises(ValueError, match=match):
            sync.detect(s, **kw)
    with pytest.raises(ValueError, match="stream_len"):
        sync.detect(s[:W - 1], 0.45, 256, 64)
    L = gfdm_amd.lib()
    assert L.gfdm_hip_burst_sync_detect_workspace_bytes(sync._h, s.size) > 0
    assert L.gfdm_hip_burst_sync_detect_workspace_bytes(sync._h, W - 1) == gfdm_amd.capi.EINVAL
    assert sync.detect(s[:W], 0.45, W - 2 * K - 64 - 1, 64)["count"] in (0, 1)          # the smallest stream and min_distance


# ---- synthetic streams at the shapes the fixtures leave out ----
# K, cp_len, min_distance, bursts, stream_len.  lead = cp_len + K // 2 (the default) and W = lead + 3 K + cp_len, so W - 2K - lead - 1 = K + cp_len - 1
EDGE_STREAMS = [
    (15, 7, 150, 10, 20000), (93, 40, 400, 8, 30000), (64, 0, 300, 9, 24000),
    (64, 256, 500, 7, 28000), (64, 257, 500, 7, 28001), (64, 300, 500, 6, 27000),      # segment_ic up to cp_len 256, tile_ic per segment above
    (64, 600, 2100, 8, 40000),                                                          # +-R spans 9 segments either side, the cp halo 3
]
EDGE_THRESHOLD = 0.8
MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def edge_stream(K, cp, Rd, nb, n):
    """dict: the stream (noise 26 dB below nb click_bursts of one core, each with its own gain, phase and CFO, more than Rd apart), the
    core, the planted core starts, lead, W and ref_detect of it"""
    rng = np.random.default_rng(K * 1000 + cp)
    burst, core = click_burst(K, cp, rng)
    lead = cp + K // 2
    W = lead + 3 * K + cp
    slot = (n - 2 * W) // nb
    assert slot > Rd + burst.size + W
    at = W + slot * np.arange(nb) + rng.integers(0, slot - Rd - burst.size, nb)       # gaps above Rd
    sigma = np.sqrt(10 ** -2.6 / 2)
    s = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for a in at:
        # (CFO within +-0.2: towards +-0.3 the fine timing locks to a +-K side peak, in the restatement as in pygfdm -- include/gfdm_hip.h)
        rot = (0.5 + rng.random()) * np.exp(1j * (2 * np.pi * rng.random() + 2 * np.pi * rng.uniform(-0.2, 0.2) / K * np.arange(burst.size)))
        s[a:a + burst.size] += burst * rot
    s = s.astype(np.complex64)
    s.setflags(write=False)
    return dict(stream=s, preamble=core, core_starts=at + 1 + cp, lead=lead, window_len=W,
                ref=ref_detect(s, core, K, cp, W, EDGE_THRESHOLD, Rd, lead))


def _assert_reference_is_decided(c, Rd):
    """on the reference alone: every maximum of the +-Rd rule is more than MARGIN off the threshold, every peak leads its +-Rd
    neighbourhood by more than MARGIN and is a planted burst, and in every peak's window the ic and |pcc| ic maxima lead by MARGIN"""
    ref = c["ref"]
    ic, peaks = ref["ic"], ref["peaks"]
    maxima = nms_maxima(ic, Rd)
    assert np.all(np.abs(ic[maxima] - EDGE_THRESHOLD) > MARGIN)
    assert np.array_equal(peaks, c["core_starts"]) and np.array_equal(ref["frame_start"], c["core_starts"])
    for i, d in enumerate(peaks):
        around = np.concatenate((ic[max(0, d - Rd):d], ic[d + 1:d + Rd + 1]))
        assert ic[d] - around.max() > MARGIN, (d, ic[d] - around.max())
        assert top_margin(ref["ic_win"][i]) > MARGIN and top_margin(ref["score_win"][i]) > MARGIN, d


@pytest.mark.parametrize("K,cp,Rd,nb,n", EDGE_STREAMS)
def test_edge_stream_peaks_are_the_rule_on_the_librarys_own_ic(K, cp, Rd, nb, n):
    import gfdm_amd
    c = edge_stream(K, cp, Rd, nb, n)
    s, lead, W = c["stream"], c["lead"], c["window_len"]
    whole = gfdm_amd.BurstSync(K, cp, c["preamble"], n)                              # the stream as one window
    ac, ic = whole.auto_correlate(s)
    rac, _ = ref_ac_ic(s, K, cp)
    e_ac, e_ic = np.max(np.abs(ac[0] - rac)), np.max(np.abs(ic[0] - c["ref"]["ic"]))
    print("K %d cp %d: ac err %.3e ic err %.3e" % (K, cp, e_ac, e_ic))
    assert e_ac < 1e-5 and e_ic < 1e-5
    sync = gfdm_amd.BurstSync(K, cp, c["preamble"], W)
    for thr in (EDGE_THRESHOLD, 0.5, 0.3):                                           # lower thresholds: noise peaks too
        r = sync.detect(s, thr, Rd, lead)
        peaks = ref_peaks(ic[0].astype(np.float64), float(np.float32(thr)), Rd)
        print("   threshold %.2f: count %d, rule %d" % (thr, r["count"], peaks.size))
        assert r["count"] == peaks.size and peaks.size >= nb, thr
        free = np.flatnonzero((peaks >= lead) & (peaks - lead <= n - W))             # coarse == peak is promised away from a clamped window only
        assert free.size >= peaks.size - 2
        assert np.array_equal(r["coarse"][free], peaks[free]) and np.array_equal(r["metric"][free], ic[0][peaks[free]]), thr
        _assert_sentinels(r, peaks.size)


@pytest.mark.parametrize("K,cp,Rd,nb,n", EDGE_STREAMS)
def test_edge_stream_matches_restatement(K, cp, Rd, nb, n):
    import torch
    import gfdm_amd
    c = edge_stream(K, cp, Rd, nb, n)
    ref = c["ref"]
    _assert_reference_is_decided(c, Rd)
    sync = gfdm_amd.BurstSync(K, cp, c["preamble"], c["window_len"])
    r = sync.detect(c["stream"], EDGE_THRESHOLD, Rd, c["lead"])
    print("K %d cp %d R %d: count %d (%d) coarse %s" % (K, cp, Rd, r["count"], nb, r["coarse"][:nb]))
    assert r["count"] == nb
    _assert_sentinels(r, nb)
    assert np.array_equal(r["frame_start"][:nb], ref["frame_start"]) and np.array_equal(r["coarse"][:nb], ref["coarse"])
    e_cfo, e_met = np.max(np.abs(r["cfo"][:nb] - ref["cfo"])), np.max(np.abs(r["metric"][:nb] - ref["metric"]))
    print("   cfo err %.3e metric err %.3e" % (e_cfo, e_met))
    assert e_cfo < 1e-4 and e_met < 1e-5
    rot = r["sc_rot"][:nb]
    assert np.max(np.abs(np.abs(rot) - 1)) < 1e-5 and np.max(np.abs(np.angle(rot) * K / (2 * np.pi) - r["cfo"][:nb])) < 1e-5
    d = _to_host(sync.detect(torch.tensor(c["stream"], device="cuda:0"), EDGE_THRESHOLD, Rd, c["lead"]))
    assert int(d["count"][0]) == nb
    for k in OUT:
        assert np.array_equal(d[k], r[k]), k


# ---- end to end on the device: detect -> extractor -> estimated IC receiver (the stream of tests/test_burst_gpu.py's chain test) ----
@pytest.mark.parametrize("M,K,L,A,slots", [(9, 64, 2, 52, 64), (15, 128, 4, 110, 16)])
def test_detect_extract_receive_on_device(M, K, L, A, slots):
    import torch
    import gfdm_amd
    rng = np.random.default_rng(M * K + L)
    dev = torch.device("cuda:0")
    N, pcp, cp = M * K, K // 2, K // 2
    smap = np.concatenate((np.arange(1, A // 2 + 1), np.arange(K - A // 2, K)))
    spec = np.zeros(K, complex)
    spec[smap] = np.exp(1j * np.pi / 2 * rng.integers(0, 4, A)) * np.sqrt(K / A)
    core = np.tile(np.fft.ifft(spec) * np.sqrt(A), 2) / np.sqrt(K)      # the data blocks' average power, A / K^2
    full = np.concatenate((core[-pcp:], core))                     # preamble with its cyclic prefix
    taps = get_frequency_domain_filter("rrc", 0.2, M, K, L)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, smap, True, L, taps, np.zeros(0, complex), [0], [full])
    F = tx.output_vector_size()
    assert F == pcp + 2 * K + cp + N
    bits = rng.integers(0, 2, (slots, A * M, 2))
    sym = ((1 - 2 * bits[..., 0]) + 1j * (1 - 2 * bits[..., 1])) / np.sqrt(2)
    frames = tx.transmit(torch.tensor(sym.astype(np.complex64), device=dev))[0].cpu().numpy()
    # one burst per slot at a random offset, its own CFO (within +-0.25 subcarrier spacings), phase and gain (+-2 dB); noise 25 dB below the frames
    S = 2 * F
    offs = rng.integers(K, S - F - K, slots)
    cfo = rng.uniform(-0.25, 0.25, slots)
    sig_pow = np.mean(np.abs(frames) ** 2)
    sigma = np.sqrt(sig_pow / 10 ** 2.5 / 2)
    s = sigma * (rng.standard_normal(slots * S) + 1j * rng.standard_normal(slots * S))
    for b in range(slots):
        rot = (0.8 + 0.45 * rng.random()) * np.exp(1j * (2 * np.pi * rng.random() + 2 * np.pi * cfo[b] / K * np.arange(F)))
        s[b * S + offs[b]:b * S + offs[b] + F] += frames[b] * rot
    truth = np.arange(slots) * S + offs + pcp                       # core preamble starts
    ds = torch.tensor(s.astype(np.complex64), device=dev)

    # the detector knows nothing of the slot grid: half a burst between detections, windows of a preamble and a bit
    lead = pcp + K // 2
    sync = gfdm_amd.BurstSync(K, pcp, core, lead + 3 * K + pcp)
    r = sync.detect(ds, 0.5, F // 2, lead, max_bursts=slots)
    burst_len = 2 * K + cp + N
    ex = gfdm_amd.BurstExtractor(burst_len, 0, True)
    bursts = ex.extract(ds, r["frame_start"], None, r["sc_rot"])
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, core)
    adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, smap, 2, R.qpsk_points())
    adv.configure_frames(burst_len, 2 * K + cp, smap, True)
    adv.set_channel_estimator(est)
    out = adv.demodulate_estimated(bursts, bursts, preamble_stride=burst_len)
    torch.cuda.synchronize()
    print("count", int(r["count"][0]), "of", slots)
    assert int(r["count"][0]) == slots
    assert np.array_equal(r["frame_start"].cpu().numpy(), truth)
    assert np.max(np.abs(r["cfo"].cpu().numpy() - cfo)) < 0.02
    o = out.cpu().numpy()
    assert o.shape == sym.shape
    assert np.array_equal(o.real > 0, sym.real > 0) and np.array_equal(o.imag > 0, sym.imag > 0)
