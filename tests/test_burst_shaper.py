"""CPU-side checks of the burst shaper (contract in include/gfdm_hip.h, gfdm_hip_burst_shaper): the entry points are exported and bound,
the argument table answers without a device, the numpy restatement (tests/burst_shaper_ref.py, the yardstick of the GPU tests) is what
the reference's three lines and to_sc16 say, Python-side argument errors come before any device, and the preconditions of the GPU
loop-back test hold on the restatement alone."""
import numpy as np
import pytest

import burst_shaper_ref as S
import gfdm_ref as R
from burst_detect_ref import nms_maxima, ref_detect
from burst_receive_cases import MARGIN, restatement, virtual_bursts

STEMS = ("gfdm_hip_burst_shaper_shape", "gfdm_hip_burst_shaper_place")
PLAIN = ("create", "destroy", "frame_len", "pre_padding", "post_padding", "scale", "check", "workspace_bytes")


def test_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.capi.exported_symbols())
    for stem in STEMS:
        for kind in ("host", "device", "sc16_host", "sc16_device"):
            assert "%s_%s" % (stem, kind) in names
            assert hasattr(gfdm_amd.lib(), "%s_%s" % (stem, kind))
    for name in PLAIN:
        assert "gfdm_hip_burst_shaper_" + name in names
    assert gfdm_amd.BurstShaper is gfdm_amd.capi.BurstShaper


# (frame_len, pre, post, peak, n_bursts, out_len) -> what the message names; None = accepted
TABLE = [
    ((721, 0, 0, 0.0, 7, 5000), None),
    ((1, 5, 1, 32767.0, 0, 0), None),
    ((1, 0, 0, 1e-3, 1, 1), None),
    ((0, 0, 0, 0.0, 1, 1), "frame_len"),
    ((-3, 0, 0, 0.0, 1, 1), "frame_len"),
    ((5, -1, 0, 0.0, 1, 1), "Pre-padding"),
    ((5, 0, -1, 0.0, 1, 1), "Post-padding"),
    ((5, 0, 0, -1.0, 1, 1), "peak"),
    ((5, 0, 0, 32767.5, 1, 1), "peak"),
    ((5, 0, 0, float("nan"), 1, 1), "peak"),
    ((5, 0, 0, float("inf"), 1, 1), "peak"),
    ((5, 0, 0, 0.0, -1, 1), "n_bursts"),
    ((5, 0, 0, 0.0, 1, -1), "out_len"),
    ((5, 0, 0, 0.0, 1, 1 << 60), "overflow"),                   # 8 out_len
    ((5, 0, 0, 0.0, 1 << 58, 1), "overflow"),                   # 8 n_bursts frame_len
    ((1 << 30, 0, 0, 0.0, 1 << 31, 1), "overflow"),
    ((5, 0, 0, 0.0, (1 << 60) // 5 - 1, (1 << 60) - 1), None),  # the largest sizes that fit
]


@pytest.mark.parametrize("args,match", TABLE)
def test_argument_table(args, match):
    import gfdm_amd
    L = gfdm_amd.lib()
    rc = L.gfdm_hip_burst_shaper_check(*args)
    if match is None:
        assert rc == gfdm_amd.capi.OK
    else:
        assert rc == gfdm_amd.capi.EINVAL
        assert match in L.gfdm_hip_last_error().decode()


def _frames(rng, n, F):
    return (rng.standard_normal((n, F)) + 1j * rng.standard_normal((n, F))).astype(np.complex64)


@pytest.mark.parametrize("F,pre,post,n", [(1, 0, 0, 1), (3, 1, 0, 7), (257, 5, 1, 2), (721, 0, 5, 3)])
def test_restatement_is_the_reference_block(F, pre, post, n):
    """short_burst_shaper_impl.cc:174-181 per burst: memset(out, 0, pre); volk_32fc_s32fc_multiply_32fc(out + pre, in, scale, F);
    memset(out + pre + F, 0, post) -- written out here burst by burst with numpy's own complex64 product"""
    rng = np.random.default_rng(F)
    x = _frames(rng, n, F)
    for scale in (0.25, -3.0, 0.7 - 0.2j):
        want = np.zeros(n * (pre + F + post), np.complex64)
        for b in range(n):
            o = b * (pre + F + post)
            want[o + pre:o + pre + F] = np.complex64(scale) * x[b]
        got = S.shape_c64(x, F, pre, post, scale)
        if np.imag(scale) == 0:
            assert np.array_equal(got, want)
        else:
            bound = 4 * 2.0 ** -24 * abs(scale) * np.abs(want / np.complex64(scale))
            assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
        # place on the slots' own starts is shape
        starts = pre + (pre + F + post) * np.arange(n)
        assert np.array_equal(S.place_c64(x, F, starts, want.size, scale), got)


def test_restatement_place_rules():
    """the cutting rules of the contract on a hand-made case"""
    F = 4
    x = (np.arange(1, 13) + 0j).astype(np.complex64).reshape(3, F)            # frames 1..4, 5..8, 9..12
    out = S.place_c64(x, F, [-2, 3, 5], 8, 1.0)
    #            i:  0  1  2  3  4  5   6   7        frame 0 from -2: 3 4 | gap | frame 1 at 3 cut by frame 2 at 5 | frame 2 cut by out_len
    assert np.array_equal(out.real, [3, 4, 0, 5, 6, 9, 10, 11])
    assert np.array_equal(S.place_c64(x, F, [-2, 3, 5], 8, 1.0, count=2).real, [3, 4, 0, 5, 6, 7, 8, 0])
    assert np.array_equal(S.place_c64(x, F, [-2, 3, 5], 8, 1.0, count=-4), np.zeros(8))
    assert np.array_equal(S.place_c64(x, F, [-2, 3, 5], 8, 1.0, count=9), out)


@pytest.mark.parametrize("peak", [0.9 * 2048, 32767.0, 1.0, 100.5])
def test_normalised_sc16_is_within_one_lsb_of_to_sc16(peak):
    """|y g| <= 32767 (1 + a few 2^-24), so the fp32 products are off by well under 0.01 and truncation can move by at most one"""
    import gfdm_amd
    rng = np.random.default_rng(int(peak))
    F, n = 257, 5
    x = _frames(rng, n, F) * np.float32(37.5)
    for scale in (1.0, 0.37, 1e-3):
        got = S.shape_sc16(x, F, 0, 0, scale, peak)
        want = gfdm_amd.to_sc16(x.ravel(), peak)                   # scale > 0 drops out of the normalisation
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1
        assert np.abs(got).max() in (int(peak), int(peak) - 1)
    zeros = S.shape_sc16(np.zeros((2, F), np.complex64), F, 1, 1, 1.0, peak)
    assert zeros.shape == (2 * (F + 2), 2) and not zeros.any()


def test_fixed_sc16_rule():
    v = np.array([32767.4, -32767.4, 32767.9, 40000.0, -40000.0, -32768.0, -32769.5, np.nan, -0.9, 0.9, 1.5, -1.5, np.inf, -np.inf], np.float32)
    want = [32767, -32767, 32767, 32767, -32768, -32768, -32768, 0, 0, 0, 1, -1, 32767, -32768]
    assert S.q16(v).tolist() == want
    fin = np.isfinite(v)
    z = np.empty(int(fin.sum()) + 1, np.complex64)
    z.real[:-1], z.imag[:-1] = v[fin], v[fin][::-1]
    z[-1] = complex(np.nan, 5.0)                  # the complex product spreads a NaN to both components (0 * NaN): both give 0
    wf = [w for w, f in zip(want, fin) if f]
    out = S.shape_sc16(z, z.size, 0, 0, 1.0)
    assert out[:, 0].tolist() == wf + [0] and out[:, 1].tolist() == wf[::-1] + [0]


def _handle_free():
    import gfdm_amd
    return object.__new__(gfdm_amd.BurstShaper)              # no handle: whatever these calls raise, they raise before the library is asked


def test_python_argument_errors_come_before_any_device():
    import torch
    sh = _handle_free()
    x = np.zeros((2, 5), np.complex64)
    for call in (lambda f, **kw: sh.shape(f, **kw), lambda f, **kw: sh.place(f, np.zeros(2, np.int64), 20, **kw)):
        for dt in (np.int16, np.int32, np.uint8, bool):
            with pytest.raises(TypeError, match="complex samples"):
                call(np.zeros((2, 5), dt))
        with pytest.raises(TypeError, match="contiguous complex64"):
            call(torch.zeros(2, 5, dtype=torch.complex64))                      # a tensor off the device
        with pytest.raises(TypeError, match="contiguous complex64"):
            call(torch.zeros(2, 5, dtype=torch.float32))
        with pytest.raises(ValueError, match="sc16=True"):
            call(x, peak=100.0)
        for peak in (0, -1.0, 32768, float("nan")):
            with pytest.raises(ValueError, match="peak"):
                call(x, sc16=True, peak=peak)
        with pytest.raises(TypeError, match="int16"):
            call(x, sc16=True, out=np.zeros((10, 2), np.complex64))
        with pytest.raises(TypeError, match="complex64"):
            call(x, out=np.zeros((10, 2), np.int16))
        with pytest.raises(ValueError, match="odd"):
            call(x, sc16=True, out=np.zeros(21, np.int16))
        with pytest.raises(ValueError, match="shape"):
            call(x, sc16=True, out=np.zeros((10, 3), np.int16))
        with pytest.raises(TypeError, match="contiguous"):
            call(x, sc16=True, out=np.zeros((10, 4), np.int16)[:, :2])
        with pytest.raises(TypeError, match="numpy array"):
            call(x, out=torch.zeros(10, dtype=torch.complex64))
        with pytest.raises(ValueError, match="one array per port"):
            call([x, x], out=[np.zeros(10, np.complex64)])
    with pytest.raises(TypeError, match="starts"):
        sh.place(x, torch.zeros(2, dtype=torch.int64), 20)


def test_no_cpu_fallback():
    """without a device the constructor fails loudly; with one it answers its getters"""
    import gfdm_amd
    from conftest import have_gpu
    if have_gpu():
        sh = gfdm_amd.BurstShaper(721, 3, 4, 0.5 - 0.25j)
        assert (sh.frame_len(), sh.pre_padding(), sh.post_padding(), sh.slot_len(), sh.scale()) == (721, 3, 4, 728, 0.5 - 0.25j)
    else:
        with pytest.raises(gfdm_amd.GfdmHipError, match="no HIP device"):
            gfdm_amd.BurstShaper(721)
    for bad, match in (((0,), "frame_len"), ((5, -1), "Pre-padding"), ((5, 0, -1), "Post-padding")):
        with pytest.raises(ValueError, match=match):
            gfdm_amd.BurstShaper(*bad)


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_back_preconditions(fmt):
    """what tests/test_burst_shaper_gpu.py::test_loop_back_on_the_device relies on, on the restatements alone: the float64 detector finds
    exactly the placed bursts at starts + cp_len, every maximum of ic is at least 1e-3 away from the threshold, every decision of every
    round (and of the plain matched-filter receiver) is at least MARGIN from a boundary and equals the transmitted symbol"""
    import gfdm_amd
    c = S.loop_case()
    if fmt == "c64":
        s = S.place_c64(c["frames"], c["frame_len"], c["starts"], c["out_len"], S.LOOP_SCALE)
    else:
        s = gfdm_amd.from_sc16(S.place_sc16(c["frames"], c["frame_len"], c["starts"], c["out_len"], S.LOOP_SCALE, peak=S.LOOP_PEAK))
    d = ref_detect(s, c["preamble"], c["K"], c["pcp"], c["window_len"], S.LOOP_THRESHOLD, c["min_distance"], c["lead"])
    assert np.array_equal(d["frame_start"], c["starts"] + c["pcp"])
    maxima = nms_maxima(d["ic"], c["min_distance"])
    thr_margin = float(np.min(np.abs(d["ic"][maxima] - S.LOOP_THRESHOLD)))
    e = virtual_bursts(s, d["frame_start"], d["sc_rot"], 0, c["F"])
    ic, margin = restatement(c, e, 2)
    mf, _ = restatement(c, e, None)
    mf_margin = float(np.min(R.decision_margin(mf, R.qpsk_points(), "qpsk")))
    print(fmt, "threshold margin %.4f, decision margin IC %.3f MF %.3f" % (thr_margin, margin, mf_margin))
    assert thr_margin >= 1e-3 and margin >= MARGIN and mf_margin >= MARGIN
    for out in (ic, mf):
        assert np.array_equal(out.real > 0, c["sym"].real > 0) and np.array_equal(out.imag > 0, c["sym"].imag > 0)
