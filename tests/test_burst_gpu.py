"""GPU tests of burst acquisition: the synchroniser (gfdm_hip_burst_sync) against pygfdm's find_frame_start / auto_correlation_sync
(tests/golden/sync/*.npz, make_golden_sync.py), the extractor (gfdm_hip_burst_extractor) against a float64 restatement of
extract_burst_cc, and both in front of the estimated IC receiver, all on the device."""
import glob
import os

import numpy as np
import pytest

import gfdm_ref as R
from conftest import GOLDEN_DIR, have_gpu
from gfdm_amd.filters import get_frequency_domain_filter

pytestmark = pytest.mark.gpu
SYNC_DIR = os.path.join(GOLDEN_DIR, "sync")


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def sync_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(SYNC_DIR, "*.npz")))


def load_sync(name):
    z = np.load(os.path.join(SYNC_DIR, name + ".npz"))
    g = {k: z[k] for k in z.files}
    for k in ("K", "cp_len", "window_len", "first", "nm", "nc", "core_start"):
        g[k] = int(g[k])
    g["kind"] = str(g["kind"])
    return g


# ---- float64 restatement of the two contracts (include/gfdm_hip.h) ----
def ref_sync(s, preamble, K, cp):
    """find_frame_start on one window, with ac = 0 where the energy is 0"""
    s = np.asarray(s, np.complex128)
    P = s.size - 2 * K
    X = np.lib.stride_tricks.sliding_window_view(s, 2 * K)[:P]
    num = 2 * np.sum(np.conj(X[:, :K]) * X[:, K:], axis=1)
    en = np.sum(np.abs(X) ** 2, axis=1)
    ac = np.where(en > 0, num / np.where(en > 0, en, 1), 0)
    c = np.concatenate(([0.0], np.cumsum(np.abs(ac))))
    ic = np.zeros(P)
    n = np.arange(cp, P)
    ic[cp:] = (c[n + 1] - c[n - cp]) / (cp + 1)
    nm = int(np.argmax(ic))
    cfo = np.angle(ac[nm]) / (2 * np.pi)
    p = np.asarray(preamble, np.complex128)
    p = p / np.sqrt(np.mean(np.abs(p) ** 2))
    s2 = s * np.exp(1j * np.pi * cfo / K * np.arange(s.size))
    pcc = np.lib.stride_tricks.sliding_window_view(s2, 2 * K)[:P] @ np.conj(p) / (2 * K)
    nc = int(np.argmax(np.abs(pcc) * ic))
    return dict(ac=ac, ic=ic, nm=nm, cfo=cfo, nc=nc, metric=ic[nm], sc_rot=np.exp(1j * np.angle(ac[nm]) / K), score=np.abs(pcc) * ic)


def ref_extract(s, offsets, burst_len, backoff, scale=None, sc_rot=None, correct=True):
    s = np.asarray(s, np.complex128)
    out = np.zeros((len(offsets), burst_len), np.complex128)
    n = np.arange(burst_len)
    for b, off in enumerate(offsets):
        i = int(off) - backoff + n
        ok = (i >= 0) & (i < s.size)
        out[b, ok] = s[i[ok]]
        out[b] *= 1.0 if scale is None else float(np.float32(scale[b]))
        if correct and sc_rot is not None:
            r = complex(np.complex64(sc_rot[b]))
            if abs(r) > 0:
                out[b] *= np.exp(-1j * np.angle(r) * n)
    return out


# ---- synchroniser against pygfdm ----
@pytest.mark.parametrize("name", sync_names())
def test_auto_correlate_matches_pygfdm(name):
    import torch
    import gfdm_amd
    g = load_sync(name)
    sync = gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], g["window_len"])
    assert sync.corr_len() == g["ac"].size
    ac, ic = sync.auto_correlate(g["stream"], first=g["first"])
    assert ac.shape == (1, g["ac"].size) and ic.shape == (1, g["ac"].size)
    assert np.max(np.abs(ac[0] - g["ac"])) < 1e-5
    assert np.max(np.abs(ic[0] - g["ic"])) < 1e-5
    dac, dic = sync.auto_correlate(torch.tensor(g["stream"], device="cuda:0"), first=g["first"])
    assert np.array_equal(dac.cpu().numpy(), ac) and np.array_equal(dic.cpu().numpy(), ic)


def _check_fused(g, r, i=0):
    first = g["first"]
    assert abs(float(r["metric"][i]) - g["ic"][g["nm"]]) < 1e-5
    if g["kind"] == "noise":            # no burst: frame_start and cfo mean nothing
        return
    assert int(r["frame_start"][i]) == first + g["nc"]
    assert abs(float(r["cfo"][i]) - float(g["cfo"])) < 1e-4
    nm = int(r["coarse"][i]) - first
    if float(g["ic_margin"]) > 1e-5:
        assert nm == g["nm"]
    else:                               # the ic plateau is flat to 1e-5: a neighbour of pygfdm's nm is as good
        assert abs(nm - g["nm"]) <= 1 and g["ic"][g["nm"]] - g["ic"][nm] < 1e-5
    rot = complex(r["sc_rot"][i])
    assert abs(abs(rot) - 1) < 1e-5 and abs(np.angle(rot) * g["K"] / (2 * np.pi) - float(r["cfo"][i])) < 1e-5


@pytest.mark.parametrize("name", sync_names())
def test_find_frame_start_matches_pygfdm(name):
    import torch
    import gfdm_amd
    g = load_sync(name)
    sync = gfdm_amd.BurstSync(g["K"], g["cp_len"], g["preamble"], g["window_len"])
    r = sync.find_frame_start(g["stream"], first=g["first"])
    _check_fused(g, r)
    # the float64 restatement the other tests use is this same contract
    ref = ref_sync(g["stream"][g["first"]:g["first"] + g["window_len"]], g["preamble"], g["K"], g["cp_len"])
    assert np.max(np.abs(ref["ac"] - g["ac"])) < 1e-9 and np.max(np.abs(ref["ic"] - g["ic"])) < 1e-9
    assert ref["nm"] == g["nm"] and ref["nc"] == g["nc"] and abs(ref["cfo"] - g["cfo"]) < 1e-9
    d = sync.find_frame_start(torch.tensor(g["stream"], device="cuda:0"), first=g["first"])
    torch.cuda.synchronize()
    for k in r:
        assert np.array_equal(d[k].cpu().numpy(), r[k]), k
    if g["kind"] in ("burst", "tiled", "zeros"):        # (a window that cuts the CP plateau puts pygfdm's nc elsewhere: ic is 0 before cp_len)
        assert int(r["frame_start"][0]) == g["core_start"]


def test_batch_of_overlapping_windows_equals_one_call_per_window():
    import torch
    import gfdm_amd
    g = load_sync("k128_cfom02_15db")
    K, cp = g["K"], g["cp_len"]
    rng = np.random.default_rng(7)
    s = np.concatenate((g["stream"], (0.05 * (rng.standard_normal(3000) + 1j * rng.standard_normal(3000))).astype(np.complex64)))
    W, stride, first = 700, 97, 3
    n = (s.size - first - W) // stride + 1
    sync = gfdm_amd.BurstSync(K, cp, g["preamble"], W)
    batch = sync.find_frame_start(s, first=first, stride=stride, n_windows=n)
    ac_b, ic_b = sync.auto_correlate(s, first=first, stride=stride, n_windows=n)
    ds = torch.tensor(s, device="cuda:0")
    dev = sync.find_frame_start(ds, first=first, stride=stride, n_windows=n)
    for w in range(n):
        one = sync.find_frame_start(s, first=first + w * stride)
        for k in batch:
            assert np.array_equal(one[k], batch[k][w:w + 1]), (w, k)
            assert np.array_equal(one[k], dev[k][w:w + 1].cpu().numpy()), (w, k)
        ac1, ic1 = sync.auto_correlate(s, first=first + w * stride)
        assert np.array_equal(ac1[0], ac_b[w]) and np.array_equal(ic1[0], ic_b[w])
        ref = ref_sync(s[first + w * stride:first + w * stride + W], g["preamble"], K, cp)
        assert np.max(np.abs(ic_b[w] - ref["ic"])) < 1e-5
    with pytest.raises(ValueError, match="runs past"):
        sync.find_frame_start(s, first=first, stride=stride, n_windows=n + 1)
    with pytest.raises(ValueError, match="runs past"):
        sync.auto_correlate(ds, first=s.size - W + 1)


def test_zero_energy_gives_zero_ac_not_nan():
    """the one deviation from pygfdm: a run of 2K or more zeros has ac = 0 (pygfdm: NaN) -- against the restatement"""
    import gfdm_amd
    K, cp, W = 64, 32, 900
    rng = np.random.default_rng(3)
    pre = np.tile(np.exp(2j * np.pi * rng.random(K)), 2)
    s = (0.1 * (rng.standard_normal(W) + 1j * rng.standard_normal(W))).astype(np.complex64)
    s[100:100 + 3 * K] = 0
    s[500:500 + 2 * K] = pre                                        # a burst core after the gap
    s[500 - cp:500] = pre[-cp:]
    sync = gfdm_amd.BurstSync(K, cp, pre, W)
    ac, ic = sync.auto_correlate(s)
    ref = ref_sync(s, pre, K, cp)
    assert np.all(ac[0][100:100 + K + 1] == 0) and np.all(np.isfinite(ac)) and np.all(np.isfinite(ic))
    assert np.max(np.abs(ac[0] - ref["ac"])) < 1e-5 and np.max(np.abs(ic[0] - ref["ic"])) < 1e-5
    r = sync.find_frame_start(s)
    assert int(r["frame_start"][0]) == ref["nc"] == 500 and abs(float(r["metric"][0]) - ref["metric"]) < 1e-5
    z = sync.find_frame_start(np.zeros(W, np.complex64))          # all zero: every ic is 0, the first index wins
    assert int(z["frame_start"][0]) == 0 and int(z["coarse"][0]) == 0 and float(z["metric"][0]) == 0.0


# ---- extractor against the restatement ----
@pytest.mark.parametrize("burst_len,backoff", [(777, 40), (4096, 0), (65536, 17)])
def test_extract_matches_restatement(burst_len, backoff):
    import torch
    import gfdm_amd
    rng = np.random.default_rng(burst_len)
    n_s = 3 * burst_len
    s = (rng.standard_normal(n_s) + 1j * rng.standard_normal(n_s)).astype(np.complex64)
    # head before 0, inside, tail past the end, entirely outside
    offsets = np.array([5, backoff, burst_len, n_s - burst_len // 3, 2 * burst_len + backoff, n_s + burst_len + 9, -burst_len // 2 - 3], np.int64)
    nb = offsets.size
    scale = (0.5 + rng.random(nb)).astype(np.float32)
    rot = (np.exp(1j * 2 * np.pi * rng.uniform(-0.45, 0.45, nb) / 64) * (0.3 + rng.random(nb))).astype(np.complex64)
    rot[2] = 0                                                      # |r| = 0: no rotation
    ex = gfdm_amd.BurstExtractor(burst_len, backoff, True)
    assert ex.burst_len() == burst_len and ex.tag_backoff() == backoff and ex.cfo_correction()
    ds, doff = torch.tensor(s, device="cuda:0"), torch.tensor(offsets, device="cuda:0")
    dscale, drot = torch.tensor(scale, device="cuda:0"), torch.tensor(rot, device="cuda:0")
    for correct in (True, False):
        ex.activate_cfo_compensation(correct)
        assert ex.cfo_correction() == correct
        for sc, r in ((scale, rot), (None, rot), (scale, None), (None, None)):
            got = ex.extract(s, offsets, sc, r)
            ref = ref_extract(s, offsets, burst_len, backoff, sc, r, correct)
            assert got.shape == (nb, burst_len)
            err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
            assert err < 2e-5, (correct, sc is None, r is None, err)
            head = max(0, backoff - 5)
            assert np.all(got[0, :head] == 0) and np.all(got[5] == 0)                   # zero-filled head, burst entirely past the end
            tail = n_s - (offsets[3] - backoff)
            assert np.all(got[3, tail:] == 0) and np.all(got[3, :tail] != 0)             # zero-filled tail
            dev = ex.extract(ds, doff, None if sc is None else dscale, None if r is None else drot)
            torch.cuda.synchronize()
            assert np.array_equal(dev.cpu().numpy(), got)                               # host and device paths bit-equal


def test_extract_argument_errors():
    import torch
    import gfdm_amd
    ex = gfdm_amd.BurstExtractor(64, 0)
    s = np.zeros(100, np.complex64)
    with pytest.raises(RuntimeError, match="scale"):
        ex.extract(s, [0, 1], scale=[1.0])
    with pytest.raises(TypeError, match="offsets"):
        ex.extract(torch.tensor(s, device="cuda:0"), torch.tensor([0], dtype=torch.int32, device="cuda:0"))
    assert ex.extract(s, np.zeros(0, np.int64)).shape == (0, 64)
    L = gfdm_amd.lib()
    assert L.gfdm_hip_burst_extractor_extract_host(ex._h, None, s.ctypes.data, s.size, None, None, None, 1) == gfdm_amd.capi.EINVAL
    assert L.gfdm_hip_burst_extractor_extract_host(ex._h, None, s.ctypes.data, s.size, None, None, None, -1) == gfdm_amd.capi.EINVAL


# ---- end to end on the device: sync on the slot grid -> extractor -> estimated IC receiver ----
@pytest.mark.parametrize("M,K,L,A,slots", [(9, 64, 2, 52, 64), (15, 128, 4, 110, 16)])
def test_sync_extract_receive_on_device(M, K, L, A, slots):
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
    # one burst per slot at a random offset, its own CFO, phase and gain (+-2 dB); noise 25 dB below the frames.  The CFO stays within +-0.25 subcarrier
    # spacings: pygfdm's correction before the fine timing (kept for parity, include/gfdm_hip.h) leaves 1.5x the CFO in the signal, and
    # beyond about +-0.3 the 2K-sample correlation loses its main peak to the +-K side peaks of the two-half preamble -- the float64
    # restatement picks the side peak there as well (13 of 64 slots of this test's first case at +-0.4).
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

    sync = gfdm_amd.BurstSync(K, pcp, core, S)
    r = sync.find_frame_start(ds, first=0, stride=S, n_windows=slots)
    burst_len = 2 * K + cp + N
    ex = gfdm_amd.BurstExtractor(burst_len, 0, True)
    bursts = ex.extract(ds, r["frame_start"], None, r["sc_rot"])
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, core)
    adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, smap, 2, R.qpsk_points())
    adv.configure_frames(burst_len, 2 * K + cp, smap, True)
    adv.set_channel_estimator(est)
    out = adv.demodulate_estimated(bursts, bursts, preamble_stride=burst_len)
    torch.cuda.synchronize()
    assert np.array_equal(r["frame_start"].cpu().numpy(), truth)
    assert np.max(np.abs(r["cfo"].cpu().numpy() - cfo)) < 0.02
    o = out.cpu().numpy()
    assert o.shape == sym.shape
    assert np.array_equal(o.real > 0, sym.real > 0) and np.array_equal(o.imag > 0, sym.imag > 0)
