"""CPU-side checks of the channel model (contract in include/gfdm_hip.h, gfdm_hip_channel_model): the entry points are exported and
bound, the argument table answers without a device, there is no CPU fallback, the restatement of tests/channel_model_ref.py (the
yardstick of the GPU tests) reproduces the generator's published known answers and the statistics the contract promises,
awgn_noise_voltage is pygfdm's noise sizing, Python-side argument errors come before any device, and the preconditions of the GPU tests
hold on the restatements alone."""
import os

import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import gfdm_ref as R
from burst_detect_ref import nms_maxima, ref_detect
from burst_receive_cases import MARGIN, restatement, virtual_bursts
from conftest import GOLDEN_DIR, have_gpu

PLAIN = ("create", "destroy", "n_taps", "taps", "frequency_offset", "noise_voltage", "seed", "set_frequency_offset", "set_noise_voltage", "set_seed",
         "check")


def test_entry_points_are_bound():
    import gfdm_amd
    names = set(gfdm_amd.capi.exported_symbols())
    for kind in ("host", "device", "sc16_host", "sc16_device"):
        assert "gfdm_hip_channel_model_apply_%s" % kind in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_channel_model_apply_%s" % kind)
    for name in PLAIN:
        assert "gfdm_hip_channel_model_" + name in names
        assert hasattr(gfdm_amd.lib(), "gfdm_hip_channel_model_" + name)
    assert gfdm_amd.ChannelModel is gfdm_amd.capi.ChannelModel and gfdm_amd.awgn_noise_voltage is gfdm_amd.capi.awgn_noise_voltage


NAN, INF = float("nan"), float("inf")
# (n_taps, frequency_offset, noise_voltage, n, history, offset, gain) -> what the message names; None = accepted
TABLE = [
    ((1, 0.0, 0.0, 0, 0, 0, 1.0), None),
    ((64, 0.5, 1e9, 1 << 40, 63, 1 << 61, -3.5), None),
    ((3, -0.5, 0.0, 1, 0, (1 << 62) - 1, 0.0), None),                # offset + n == 2^62
    ((3, 0.0, 0.0, 1 << 59, (1 << 60) - (1 << 59) - 1, 0, 1.0), None),         # 8 (history + n) just fits
    ((0, 0.0, 0.0, 1, 0, 0, 1.0), "n_taps"),
    ((65, 0.0, 0.0, 1, 0, 0, 1.0), "n_taps"),
    ((-1, 0.0, 0.0, 1, 0, 0, 1.0), "n_taps"),
    ((3, NAN, 0.0, 1, 0, 0, 1.0), "frequency_offset"),
    ((3, INF, 0.0, 1, 0, 0, 1.0), "frequency_offset"),
    ((3, 0.5000001, 0.0, 1, 0, 0, 1.0), "frequency_offset"),
    ((3, -0.5000001, 0.0, 1, 0, 0, 1.0), "frequency_offset"),
    ((3, 0.0, NAN, 1, 0, 0, 1.0), "noise_voltage"),
    ((3, 0.0, INF, 1, 0, 0, 1.0), "noise_voltage"),
    ((3, 0.0, -1e-30, 1, 0, 0, 1.0), "noise_voltage"),
    ((3, 0.0, 0.0, 1, 0, 0, NAN), "gain"),
    ((3, 0.0, 0.0, 1, 0, 0, -INF), "gain"),
    ((3, 0.0, 0.0, -1, 0, 0, 1.0), "n must"),
    ((3, 0.0, 0.0, 1, -1, 0, 1.0), "history"),
    ((3, 0.0, 0.0, 1, 0, -1, 1.0), "offset must"),
    ((3, 0.0, 0.0, 2, 0, (1 << 62) - 1, 1.0), "2^62"),
    ((3, 0.0, 0.0, 1, 0, 1 << 62, 1.0), "2^62"),
    ((3, 0.0, 0.0, (1 << 62) + 1, 0, 0, 1.0), "2^62"),
    ((3, 0.0, 0.0, 1 << 60, 0, 0, 1.0), "overflow"),                  # 8 n
    ((3, 0.0, 0.0, 1, 1 << 60, 0, 1.0), "overflow"),                  # 8 (history + n)
    ((3, 0.0, 0.0, 1 << 59, (1 << 60) - (1 << 59), 0, 1.0), "overflow"),
]


@pytest.mark.parametrize("args,match", TABLE)
def test_argument_table(args, match):
    import gfdm_amd
    L = gfdm_amd.lib()
    rc = L.gfdm_hip_channel_model_check(*args)
    if match is None:
        assert rc == gfdm_amd.capi.OK
    else:
        assert rc == gfdm_amd.capi.EINVAL
        assert match in L.gfdm_hip_last_error().decode()


def test_no_cpu_fallback():
    """without a device the constructor fails loudly with ENODEV; with one it answers its getters and setters.  What create can refuse
    without a device it refuses first."""
    import gfdm_amd
    for kw, match in ((dict(taps=[]), "n_taps"), (dict(taps=np.ones(65)), "n_taps"), (dict(taps=[1, NAN]), "taps"), (dict(taps=[1, complex(0, INF)]), "taps"),
                      (dict(frequency_offset=0.6), "frequency_offset"), (dict(noise_voltage=-1.0), "noise_voltage"), (dict(noise_voltage=NAN), "noise_voltage")):
        with pytest.raises(ValueError, match=match):
            gfdm_amd.ChannelModel(**kw)
    with pytest.raises(ValueError, match="epsilon"):
        gfdm_amd.ChannelModel(0.1, 0.0, 1.001)
    if have_gpu():
        ch = gfdm_amd.ChannelModel(0.25, -0.125, 1.0, [1, 0.5j], -2)
        assert (ch.n_taps(), ch.frequency_offset(), ch.noise_voltage(), ch.seed()) == (2, -0.125, 0.25, 2 ** 64 - 2)
        assert np.array_equal(ch.taps(), np.array([1, 0.5j], np.complex64))
        ch.set_frequency_offset(0.5)
        ch.set_noise_voltage(0.0)
        ch.set_seed(7)
        assert (ch.frequency_offset(), ch.noise_voltage(), ch.seed()) == (0.5, 0.0, 7)
        for call, bad in ((ch.set_frequency_offset, 0.51), (ch.set_frequency_offset, NAN), (ch.set_noise_voltage, -1.0), (ch.set_noise_voltage, INF)):
            with pytest.raises(ValueError):
                call(bad)
        assert (ch.frequency_offset(), ch.noise_voltage()) == (0.5, 0.0)          # a refused value changes nothing
    else:
        with pytest.raises(gfdm_amd.GfdmHipError, match="no HIP device") as e:
            gfdm_amd.ChannelModel(0.1, 0.01, 1.0, [1, 0.2])
        assert e.value.status == gfdm_amd.capi.ENODEV


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    """the three known answers of the Random123 distribution for philox4x32-10 (kat_vectors), scalar and inside a vector call"""
    f = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((f, f, f, f), (f, f), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert _hex(C.philox4x32_10(ctr, key)) == want
    ctr, key, want = kat[2]
    out = C.philox4x32_10([np.array([0, c, 5]) for c in ctr], key)
    assert _hex(w[1] for w in out) == want
    # the noise's use of it: counter (lo32(a >> 1), hi32(a >> 1), 0, 0), key (lo32(seed), hi32(seed)); even a words (0, 1), odd a words (2, 3)
    seed, a = 0x299F31D0A4093822, 2 * 0x85A308D3243F6A88 % 2 ** 64
    assert a == 2 * (0x85A308D3243F6A88 % 2 ** 63)
    pair = a >> 1
    ref = C.philox4x32_10((pair & f, pair >> 32, 0, 0), (seed & f, seed >> 32))
    k0, k1 = C.noise_words(a, 2, seed)
    assert (int(k0[0]), int(k1[0]), int(k0[1]), int(k1[1])) == tuple(int(w) for w in ref)


def test_the_kernels_philox_header_gives_the_known_answers(tmp_path):
    """gr-gfdm_amd/csrc/gfdm_philox.h -- the rounds k_channel runs -- is plain integer code: compiled for the host it prints the same three
    known answers, and the words of a pair as the restatement's noise_words has them"""
    import subprocess
    from conftest import ROOT
    src = tmp_path / "kat.cc"
    src.write_text('#include "gfdm_philox.h"\n#include <cstdio>\n'
                   'static void p(gfdm::Philox4 r) { std::printf("%08x %08x %08x %08x\\n", r.v[0], r.v[1], r.v[2], r.v[3]); }\n'
                   'int main() {\n'
                   '    p(gfdm::philox4x32_10(0, 0, 0, 0, 0, 0));\n'
                   '    p(gfdm::philox4x32_10(~0u, ~0u, ~0u, ~0u, ~0u, ~0u));\n'
                   '    p(gfdm::philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u));\n'
                   '    p(gfdm::philox4x32_10(0x80000001u, 0x7fu, 0, 0, 11u, 0x12345678u));\n'
                   '    return 0;\n}\n')
    exe = str(tmp_path / "kat")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "gr-gfdm_amd", "csrc"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:3] == ["6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd", "d16cfe09 94fdcceb 5001e420 24126ea1"]
    a = 2 * ((0x7F << 32) | 0x80000001)                              # the pair whose counter is (0x80000001, 0x7f, 0, 0)
    k0, k1 = C.noise_words(a, 2, (0x12345678 << 32) | 11)
    assert out[3] == _hex((k0[0], k1[0], k0[1], k1[1]))


def test_noise_statistics():
    """2^20 samples of the restatement: mean, the two component variances, the re / im correlation and the lag-1 correlation within 5
    standard errors of what unit-variance independent Gaussian components give; the standard errors follow from N alone (var of a
    unit Gaussian's square is 2, of a product of two independent ones 1)"""
    N = 1 << 20
    w = C.noise(0, N, 7)
    re, im = w.real, w.imag
    se_mean, se_var, se_corr = 1 / np.sqrt(N), np.sqrt(2.0 / N), 1 / np.sqrt(N)
    stats = dict(mean_re=(re.mean(), 0, se_mean), mean_im=(im.mean(), 0, se_mean), var_re=(np.mean(re ** 2), 1, se_var), var_im=(np.mean(im ** 2), 1, se_var),
                 corr_re_im=(np.mean(re * im), 0, se_corr), lag1_re=(np.mean(re[1:] * re[:-1]), 0, se_corr), lag1_im=(np.mean(im[1:] * im[:-1]), 0, se_corr),
                 lag1_cross=(np.mean(re[1:] * im[:-1]), 0, se_corr), power=(np.mean(np.abs(w) ** 2), 2, 2 / np.sqrt(N)))
    for name, (got, want, se) in stats.items():
        print("%-10s %+.5f  expected %g  (%.2f standard errors)" % (name, got, want, (got - want) / se))
        assert abs(got - want) <= 5 * se, name
    assert np.abs(w).max() <= C.W_MAX and 5.88 < C.W_MAX < 5.89
    # a pure function of (seed, a): any cut gives the same samples, another seed other ones
    assert np.array_equal(np.concatenate((C.noise(0, 1001, 7), C.noise(1001, 999, 7))), w[:2000])
    assert np.array_equal(C.noise(2 ** 33 - 3, 7, 7)[3:], C.noise(2 ** 33, 4, 7)) and not np.array_equal(C.noise(0, 8, 8), w[:8])


def test_awgn_noise_voltage_is_pygfdm():
    """sqrt(2 * calculate_awgn_noise_variance(...)) on the fixture of tests/golden/make_golden_channel.py, numpy and torch inputs"""
    import torch
    import gfdm_amd
    z = np.load(os.path.join(GOLDEN_DIR, "channel", "awgn_variance.npz"))
    assert int(z["n_cases"]) >= 5
    for i in range(int(z["n_cases"])):
        x, snr_db, rate, var = z["signal_%d" % i], float(z["snr_db_%d" % i]), float(z["rate_%d" % i]), float(z["variance_%d" % i])
        want = np.sqrt(2 * var)
        assert abs(gfdm_amd.awgn_noise_voltage(x, snr_db, rate) - want) <= 1e-12 * want
        assert abs(gfdm_amd.awgn_noise_voltage(torch.from_numpy(x), snr_db, rate) - want) <= 1e-12 * want
    assert abs(gfdm_amd.awgn_noise_voltage(z["signal_1"], float(z["snr_db_1"])) - np.sqrt(2 * float(z["variance_1"]))) < 1e-12       # rate defaults to 1
    with pytest.raises(ValueError):
        gfdm_amd.awgn_noise_voltage([], 10.0)


def _handle_free():
    import gfdm_amd
    return object.__new__(gfdm_amd.ChannelModel)              # no handle: whatever these calls raise, they raise before the library is asked


def test_python_argument_errors_come_before_any_device():
    import torch
    ch = _handle_free()
    x = np.zeros(10, np.complex64)
    for dt in (np.int16, np.int32, np.uint8, bool):
        with pytest.raises(TypeError, match="x must be complex samples"):
            ch.apply(np.zeros(10, dt))
    with pytest.raises(TypeError, match="x must be a contiguous complex64"):
        ch.apply(torch.zeros(10, dtype=torch.complex64))                        # a tensor off the device
    with pytest.raises(TypeError, match="contiguous complex64"):
        ch.apply(torch.zeros(10, dtype=torch.float32))
    with pytest.raises(ValueError, match="sc16=True"):
        ch.apply(x, gain=2.0)
    with pytest.raises(TypeError, match="int16"):
        ch.apply(x, sc16=True, out=np.zeros(10, np.complex64))
    with pytest.raises(TypeError, match="complex64"):
        ch.apply(x, out=np.zeros((10, 2), np.int16))
    with pytest.raises(ValueError, match="odd"):
        ch.apply(x, sc16=True, out=np.zeros(21, np.int16))
    with pytest.raises(ValueError, match="shape"):
        ch.apply(x, sc16=True, out=np.zeros((10, 3), np.int16))
    with pytest.raises(TypeError, match="contiguous"):
        ch.apply(x, sc16=True, out=np.zeros((10, 4), np.int16)[:, :2])
    with pytest.raises(TypeError, match="numpy array, as x is"):
        ch.apply(x, out=torch.zeros(10, dtype=torch.complex64))
    for history in (-1, 11):
        with pytest.raises(ValueError, match="history"):
            ch.apply(x, history=history)
    with pytest.raises(RuntimeError, match="out holds 10 samples, expected 7"):
        ch.apply(x, history=3, out=np.zeros(10, np.complex64))


def test_case_table_covers_what_the_contract_names():
    """every T, n, kind of history, f, s, offset, both input parities, every output alignment of both formats; (f, s) in all four
    zero / non-zero combinations; the seeded inputs keep the sc16 cases far from saturation"""
    cases = C.all_cases()
    assert len(cases) == 2 * len(C.TS) * len(C.NS)
    assert {c["T"] for c in cases} == set(C.TS) and {c["n"] for c in cases} == set(C.NS)
    assert {c["f"] for c in cases} == set(C.FS) and {c["s"] for c in cases} == set(C.SS) and {c["offset"] for c in cases} == set(C.OFFSETS)
    for T in C.TS:
        per = C.cases(T)
        assert {c["history"] for c in per} == set(C.histories(T)) and {c["n"] for c in per} == set(C.NS)
        assert {c["offset"] for c in per} == set(C.OFFSETS) and {c["f"] for c in per} == set(C.FS)
    assert {(c["f"] != 0, c["s"] != 0) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c["fmt"], c["in_shift"], c["out_shift"]) for c in cases} == {("c64", i, o) for i in (0, 1) for o in (0, 1)} | {("sc16", i, o) for i in (0, 1) for o in range(4)}
    assert {(c["offset"] + c["n"]) % 2 for c in cases} == {0, 1} and {(c["offset"] % 2, c["out_shift"] % 2) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the counter's high word changes inside a call
    assert any(c["offset"] >> 33 != (c["offset"] + c["n"] - 1) >> 33 for c in cases)


def test_sc16_guard_band_stays_small():
    """the guard band of the sc16 comparison -- components within gain * budget of a step of q -- holds at most 1 % of the components of
    every sc16 case of the table and of the loop test, and no case of the table saturates"""
    worst = 0.0
    for c in C.all_cases():
        if c["fmt"] != "sc16":
            continue
        d = C.case_data(c["T"], C.cases(c["T"]).index(c))
        want, guard = C.sc16(d["y"], d["budget"], C.sc16_gain(c["T"]))
        assert np.abs(want.astype(np.int32)).max() < 32767
        if guard.size >= 200:                                        # (a case of 1 .. 3 samples has no percentages)
            worst = max(worst, float(guard.mean()))
        assert guard.sum() <= max(1, C.GUARD_CAP * guard.size), (c, guard.mean())
    _, y, budget = C.loop_stream()
    want, guard = C.sc16(y, budget, C.LOOP_GAIN)
    worst = max(worst, float(guard.mean()))
    print("largest guard band: %.4f of the components" % worst)
    assert guard.mean() <= C.GUARD_CAP
    assert 1024 <= np.abs(want.astype(np.int32)).max() < 2048          # inside 12 bits, and using them


def test_q_and_its_guard():
    v = np.array([32767.4, -32767.4, 32767.9, 40000.0, -40000.0, -32768.0, -32769.5, np.nan, -0.9, 0.9, 1.5, -1.5, np.inf, -np.inf])
    assert C.q16(v).tolist() == [32767, -32767, 32767, 32767, -32768, -32768, -32768, 0, 0, 0, 1, -1, 32767, -32768]
    assert np.array_equal(C.q16(v.astype(np.float32)), B.q16(v.astype(np.float32)))              # the burst shaper's rule
    y = np.array([0.0, 1e-9, 0.9999995, -1.0000001, 5.5, 7.0000001 - 3.9999999j, 32766.9999999, 40000.0])
    _, guard = C.sc16(y, np.full(y.size, 1e-6), 1.0)
    assert guard[:, 0].tolist() == [False, False, True, True, False, True, True, False] and bool(guard[5, 1])


@pytest.mark.parametrize("fmt", ["c64", "sc16"])
def test_loop_preconditions(fmt):
    """what tests/test_channel_model_gpu.py::test_loop_with_a_channel relies on, on the restatements alone: behind three taps, a CFO of
    -0.003 and noise 20 dB below the frames the float64 detector finds exactly the placed bursts, every maximum of ic is at least 1e-3 away
    from the threshold, and every decision of every round (and of the matched-filter receiver) is at least MARGIN from a boundary and
    equals the transmitted symbol.  (Measured while writing: threshold margin 0.19, decision margin 0.258.)"""
    import gfdm_amd
    c = B.loop_case()
    x, y, budget = C.loop_stream()
    frames_power = float(np.mean(np.abs(x[x != 0]) ** 2))
    rx_power = frames_power * float(np.sum(np.abs(np.array(C.LOOP_TAPS)) ** 2))                  # behind the taps
    assert abs(20 * np.log10(C.LOOP_NOISE_VOLTAGE / np.sqrt(rx_power)) + 20) < 0.05             # 20 dB below the frames
    if fmt == "c64":
        s = y.astype(np.complex64)
    else:
        s = gfdm_amd.from_sc16(C.sc16(y, budget, C.LOOP_GAIN)[0])
    d = ref_detect(s, c["preamble"], c["K"], c["pcp"], c["window_len"], B.LOOP_THRESHOLD, c["min_distance"], c["lead"])
    assert np.array_equal(d["frame_start"], c["starts"] + c["pcp"])
    maxima = nms_maxima(d["ic"], c["min_distance"])
    thr_margin = float(np.min(np.abs(d["ic"][maxima] - B.LOOP_THRESHOLD)))
    e = virtual_bursts(s, d["frame_start"], d["sc_rot"], 0, c["F"])
    ic, margin = restatement(c, e, 2)
    mf, _ = restatement(c, e, None)
    mf_margin = float(np.min(R.decision_margin(mf, R.qpsk_points(), "qpsk")))
    print(fmt, "threshold margin %.4f, decision margin IC %.3f MF %.3f" % (thr_margin, margin, mf_margin))
    assert thr_margin >= 1e-3 and margin >= MARGIN and mf_margin >= MARGIN
    for out in (ic, mf):
        assert np.array_equal(out.real > 0, c["sym"].real > 0) and np.array_equal(out.imag > 0, c["sym"].imag > 0)
