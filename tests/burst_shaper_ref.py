"""numpy restatement of the burst shaper's contract (include/gfdm_hip.h, gfdm_hip_burst_shaper): shape, place, the sc16 output rule and
the normalisation, in float32 where the contract says fp32 and float64 where it says double.  Shared by the CPU tests
(tests/test_burst_shaper.py) and the GPU tests (tests/test_burst_shaper_gpu.py), and the yardstick of both: nothing here calls the
library.  Also the loop-back case of the GPU test (transmit -> place -> detect -> demodulate_bursts), built on the oracle's transmitter so
that its preconditions can be checked without a device."""
import functools

import numpy as np

import gfdm_ref as R
from burst_receive_cases import CASES, active_bins
from gfdm_amd.filters import get_frequency_domain_filter


def scaled(frames, scale):
    """y = scale * frames as one fp32 complex product: (sr xr - si xi, sr xi + si xr), every operation rounded to float32.  For a real scale
    (si = 0) each component is a single product, so fused and unfused evaluation agree exactly on finite inputs."""
    x = np.asarray(frames, np.complex64)
    sr, si = np.float32(complex(scale).real), np.float32(complex(scale).imag)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.empty(x.shape, np.complex64)
        y.real = sr * xr - si * xi
        y.imag = sr * xi + si * xr
    return y


def shape_c64(frames, F, pre, post, scale):
    """the reference's three lines per burst (short_burst_shaper_impl.cc:174-181): zeros, scale * in, zeros"""
    y = scaled(np.asarray(frames).reshape(-1, F), scale)
    out = np.zeros((y.shape[0], pre + F + post), np.complex64)
    out[:, pre:pre + F] = y
    return out.ravel()


def place_c64(frames, F, starts, out_len, scale, count=None):
    """sample by sample from the definition: b = the last live burst with starts[b] <= i; y_b[i - starts[b]] inside the frame, else 0"""
    y = scaled(np.asarray(frames).reshape(-1, F), scale)
    n = y.shape[0]
    live = n if count is None else min(max(int(count), 0), n)
    st = np.asarray(starts, np.int64)[:live]
    out = np.zeros(out_len, np.complex64)
    if live == 0 or out_len == 0:
        return out
    i = np.arange(out_len, dtype=np.int64)
    b = np.searchsorted(st, i, side="right") - 1
    k = i - st[np.maximum(b, 0)]
    ok = (b >= 0) & (k >= 0) & (k < F)
    out[ok] = y[b[ok], k[ok]]
    return out


def live_top(frames, F, scale, count=None):
    """the largest |re| or |im| of y over the live frames (float32, exact: a maximum has no rounding)"""
    y = scaled(np.asarray(frames).reshape(-1, F), scale)
    live = y.shape[0] if count is None else min(max(int(count), 0), y.shape[0])
    y = y[:live]
    return np.float32(max(np.max(np.abs(y.real)), np.max(np.abs(y.imag)))) if y.size else np.float32(0)


def gain(peak, top):
    """g of the contract: 1 for peak == 0 (fixed) and for top == 0, else (float)((double)peak / (double)top)"""
    if not peak or not top > 0:
        return np.float32(1)
    return np.float32(float(peak) / float(top))


def q16(v):
    """truncation toward zero, saturated to int16, NaN -> 0"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.clip(np.where(np.isnan(v), np.float32(0), v), -32768.0, 32767.0))
    return t.astype(np.int16)


def to_sc16_out(stream, g):
    """q(y * g) per component, the product in float32: int16 (n, 2)"""
    s = np.asarray(stream, np.complex64)
    g = np.float32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack((q16(s.real.astype(np.float32) * g), q16(s.imag.astype(np.float32) * g)), axis=1)


def shape_sc16(frames, F, pre, post, scale, peak=0):
    return to_sc16_out(shape_c64(frames, F, pre, post, scale), gain(peak, live_top(frames, F, scale)))


def place_sc16(frames, F, starts, out_len, scale, count=None, peak=0):
    return to_sc16_out(place_c64(frames, F, starts, out_len, scale, count), gain(peak, live_top(frames, F, scale, count)))


# ---- the loop-back case: K = 64, M = 9, overlap 2 (burst_receive_cases' rowlane_7 shape), roll-off 0.1, no suffix, no ramp, unit window,
# preamble [last cp of core | core]; frames from the oracle's transmitter, placed at irregular starts ----
LOOP_GAPS = (101, 0, 1, 333, 37, 2 * 738 + 5, 64)        # silence in front of each burst: a lead-in, back to back, one sample, ..., several frames
LOOP_TAIL = 150
LOOP_THRESHOLD = 0.5
LOOP_SEED = 3
LOOP_SCALE = 0.5
LOOP_PEAK = 0.9 * 2048                                   # to_sc16's default: 0.9 of a 12-bit converter's full scale


@functools.lru_cache(maxsize=None)
def loop_case(seed=LOOP_SEED):
    """dict: the transmitter's arguments, symbols, frames (complex64, what Transmitter.transmit yields up to fp32 rounding), starts,
    out_len, and what burst_receive_cases.restatement reads (M, K, L, A, N, cp, pre_off, preamble, nt, smap, sym)"""
    M, K, L, A, nb, _ = CASES["rowlane_7"]
    rng = np.random.default_rng(seed)
    N, cp = M * K, K // 4 + 1                                   # burst_receive_cases' prefix: the frame behind the preamble's own prefix has 721 samples
    smap = active_bins(K, A)
    spec = np.zeros(K, complex)
    spec[smap] = np.exp(1j * np.pi / 2 * rng.integers(0, 4, A)) * np.sqrt(K / A)
    core = np.tile(np.fft.ifft(spec) * np.sqrt(A), 2) / np.sqrt(K)
    full = np.concatenate((core[-cp:], core))
    taps = get_frequency_domain_filter("rrc", 0.1, M, K, L)
    nt = R.normalize_taps(taps, M)
    bits = rng.integers(0, 2, (nb, A * M, 2))
    sym = ((1 - 2 * bits[..., 0]) + 1j * (1 - 2 * bits[..., 1])) / np.sqrt(2)
    frames = R.transmit(sym, nt, M, K, L, smap, True, cp, 0, 0, np.ones(N + cp), 0, full).astype(np.complex64)
    F = frames.shape[1]
    assert F == cp + 2 * K + cp + N
    starts = np.cumsum(np.array(LOOP_GAPS[:nb]) + np.concatenate(([0], np.full(nb - 1, F)))).astype(np.int64)
    out_len = int(starts[-1] + F + LOOP_TAIL)
    return dict(M=M, K=K, L=L, A=A, N=N, cp=cp, pcp=cp, pre_off=0, F=2 * K + cp + N, frame_len=F, taps=taps, nt=nt, smap=smap, preamble=core,
                full_preamble=full, sym=sym.astype(np.complex64), frames=frames, starts=starts, out_len=out_len, nb=nb,
                lead=cp + K // 2, window_len=cp + K // 2 + 3 * K + cp, min_distance=F // 2)
