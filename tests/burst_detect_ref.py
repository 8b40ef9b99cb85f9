"""float64 restatement of the burst detector's contract (include/gfdm_hip.h, gfdm_hip_burst_sync_detect): ac / ic over the whole
stream as one window, the peak rule (threshold, first-index non-maximum suppression within +-min_distance) and, per peak, pygfdm's
find_frame_start on the window the contract assigns.  Shared by the CPU and GPU tests and by tests/golden/make_golden_detect.py."""
import glob
import os

import numpy as np

DETECT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect")
INT_KEYS = ("K", "cp_len", "window_len", "min_distance", "lead")


def detect_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(DETECT_DIR, "*.npz")))


def load_detect(name):
    z = np.load(os.path.join(DETECT_DIR, name + ".npz"))
    g = {k: z[k] for k in z.files}
    for k in INT_KEYS:
        g[k] = int(g[k])
    g["threshold"] = float(g["threshold"])
    return g


def ref_ac_ic(s, K, cp):
    """ac (0 where the energy is 0) and ic of one window"""
    s = np.asarray(s, np.complex128)
    P = s.size - 2 * K
    X = np.lib.stride_tricks.sliding_window_view(s, 2 * K)[:P]
    num = 2 * np.sum(np.conj(X[:, :K]) * X[:, K:], axis=1)
    en = np.sum(np.abs(X) ** 2, axis=1)
    ac = np.where(en > 0, num / np.where(en > 0, en, 1), 0)
    mag = np.abs(ac)
    ic = np.zeros(P)
    if P > cp:
        ic[cp:] = np.sum(np.lib.stride_tricks.sliding_window_view(mag, cp + 1), axis=1) / (cp + 1)
    return ac, ic


def nms_maxima(ic, R):
    """positions i with ic[j] < ic[i] for j in [i - R, i) and ic[j] <= ic[i] for j in (i, i + R] (ranges cut at the ends)"""
    ic = np.asarray(ic, float)
    P = ic.size
    if R == 0:
        return np.arange(P)
    # maximum of every R consecutive values in O(P): blocks of R, running maxima from both block ends (van Herk / Gil-Werman)
    nb = -(-(P + 2 * R) // R) + 1
    pad = np.full(nb * R, -np.inf)
    pad[R:R + P] = ic
    blk = pad.reshape(nb, R)
    fwd = np.maximum.accumulate(blk, axis=1).ravel()
    bwd = np.maximum.accumulate(blk[:, ::-1], axis=1)[:, ::-1].ravel()
    k = np.arange(P)
    left = np.maximum(bwd[k], fwd[k + R - 1])                       # max pad[k : k + R] = ic[i - R .. i - 1]
    right = np.maximum(bwd[k + R + 1], fwd[k + 2 * R])              # max pad[k + R + 1 : k + 2 R + 1] = ic[i + 1 .. i + R]
    return np.flatnonzero((left < ic) & (right <= ic))


def ref_peaks(ic, threshold, R):
    m = nms_maxima(ic, R)
    return m[np.asarray(ic)[m] >= threshold]


def ref_fine(win, preamble, K, cp):
    """find_frame_start on one window (tests/test_burst_gpu.py::ref_sync restated on ref_ac_ic)"""
    win = np.asarray(win, np.complex128)
    ac, ic = ref_ac_ic(win, K, cp)
    P = ic.size
    nm = int(np.argmax(ic))
    cfo = np.angle(ac[nm]) / (2 * np.pi)
    p = np.asarray(preamble, np.complex128)
    p = p / np.sqrt(np.mean(np.abs(p) ** 2))
    s2 = win * np.exp(1j * np.pi * cfo / K * np.arange(win.size))
    pcc = np.lib.stride_tricks.sliding_window_view(s2, 2 * K)[:P] @ np.conj(p) / (2 * K)
    nc = int(np.argmax(np.abs(pcc) * ic))
    return dict(ic=ic, nm=nm, nc=nc, cfo=cfo, metric=ic[nm], sc_rot=np.exp(1j * np.angle(ac[nm]) / K), score=np.abs(pcc) * ic)


def top_margin(v):
    """the largest value's lead over the second largest (inf for a single value)"""
    v = np.asarray(v, float)
    if v.size < 2:
        return np.inf
    top = np.partition(v, v.size - 2)[-2:]
    return float(top[1] - top[0])


def click_burst(K, cp, rng):
    """[click | prefix (cp) | core (2K) | click] and the core: a unit-amplitude random-phase half-symbol twice, the prefix the core's tail
    (tiled where cp > 2K), and one sample of power 2K on either side.  Without the clicks the ic maximum leads its neighbours by about
    1 / (2K (cp + 1)) only -- |ac| leaves its plateau in steps of 1 / 2K --, below what fp32 can be held to at a long prefix; a click
    entering the 2K window doubles its energy, so the lead is about 0.5 / (cp + 1) whatever K is."""
    core = np.tile(np.exp(2j * np.pi * rng.random(K)), 2)
    click = np.sqrt(2 * K) * np.exp(2j * np.pi * rng.random(2))
    return np.concatenate((click[:1], np.resize(core[::-1], cp)[::-1], core, click[1:])), core


def ref_detect(s, preamble, K, cp, W, threshold, R, lead):
    """dict: ic (global), peaks, starts, and per peak frame_start, coarse (stream indices), cfo, metric, sc_rot, ic_win and score_win
    (the window's ic and |pcc| ic)"""
    s = np.asarray(s)
    _, ic = ref_ac_ic(s, K, cp)
    peaks = ref_peaks(ic, threshold, R)
    starts = np.clip(peaks - lead, 0, s.size - W)
    out = dict(ic=ic, peaks=peaks, starts=starts, frame_start=[], coarse=[], cfo=[], metric=[], sc_rot=[], ic_win=[], score_win=[])
    for st in starts:
        f = ref_fine(s[st:st + W], preamble, K, cp)
        out["frame_start"].append(st + f["nc"])
        out["coarse"].append(st + f["nm"])
        out["ic_win"].append(f["ic"])
        out["score_win"].append(f["score"])
        for k in ("cfo", "metric", "sc_rot"):
            out[k].append(f[k])
    for k in ("frame_start", "coarse", "cfo", "metric", "sc_rot"):
        out[k] = np.array(out[k], dtype=np.int64 if k in ("frame_start", "coarse") else None)
    return out
