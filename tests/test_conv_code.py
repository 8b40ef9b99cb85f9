"""CPU tests of the convolutional code (contract in include/gfdm_hip.h, gfdm_hip_conv_code): the numpy restatement of
tests/conv_code_ref.py held to facts that do not depend on it, and what the library answers without a device -- the argument table, the
constructor's ENODEV, the wrapper's surface.  The last test holds the inputs of the GPU coding-gain test before they reach a GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import conv_code_ref as V
from conftest import have_gpu


def test_impulse_response_of_171_133():
    """a single 1, terminated: the two generators read out MSB first, interleaved (1011011 and 1111001 from the newest bit on)"""
    c = V.encode_bits([[1]])
    assert c.tolist() == [[1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1]]
    assert V.encode(np.array([[0x80]], np.uint8), 1).tolist() == [[0b11011111, 0b00101100]]
    assert V.encode(np.array([[0xFF]], np.uint8), 1).tolist() == [[0b11011111, 0b00101100]]      # the spare bits are ignored
    # a negative generator complements its output, tail included
    assert V.encode_bits([[1]], (109, -79)).tolist() == [[1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 1, 0]]


def test_free_distance_is_10():
    msgs = np.array([[(m >> (11 - i)) & 1 for i in range(12)] for m in range(1, 4096)])
    assert int(V.encode_bits(msgs).sum(axis=1).min()) == 10


@pytest.mark.parametrize("mode", [V.TERMINATED, V.TRUNCATED])
def test_path_metric_is_the_brute_force_maximum(mode):
    """n_info = 8: the decoder's metric equals the best correlation over all 256 messages, and its message attains it"""
    rng = np.random.default_rng(5)
    n = 8
    msgs = np.array([[(m >> (7 - i)) & 1 for i in range(n)] for m in range(256)])
    signs = 1 - 2 * V.encode_bits(msgs, mode=mode).astype(np.int64)                  # (256, 2 T)
    q = rng.integers(-127, 128, (40, signs.shape[1]))
    bits, metric = V.viterbi(q, n, mode=mode)
    corr = q @ signs.T                                                               # (40, 256)
    assert np.array_equal(metric, corr.max(axis=1))
    got = (1 - 2 * V.encode_bits(bits, mode=mode).astype(np.int64))
    assert np.array_equal((got * q).sum(axis=1), metric)


def test_round_trip_and_up_to_four_flips():
    rng = np.random.default_rng(6)
    for mode in (V.TERMINATED, V.TRUNCATED):
        for n_info in (1, 2, 8, 57, 456):
            data = V.random_info(rng, 3, n_info)
            got, _ = V.decode_hard(V.encode(data, n_info, mode=mode), n_info, mode=mode)
            assert np.array_equal(got, V.clean(data, n_info)), (mode, n_info)
    # every pattern of <= 4 sign flips in a terminated row is corrected (free distance 10)
    n_info, n = 40, 300
    u = rng.integers(0, 2, (n, n_info))
    q = 1 - 2 * V.encode_bits(u).astype(np.int64)
    for r in range(n):
        q[r, rng.choice(q.shape[1], size=int(rng.integers(1, 5)), replace=False)] *= -1
    bits, _ = V.viterbi(q, n_info)
    assert np.array_equal(bits, u)


def test_quantiser():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0, 3.4e38], np.float32)
    assert V.quantise(x, 1.0).tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127, 127, -127, 0, 0, 0, 127]
    assert V.quantise(np.array([3.4e38], np.float32), 8.0).tolist() == [127]         # the product overflows to +inf


def test_erasures_decode_to_zero():
    bits, metric = V.viterbi(np.zeros((2, 2 * 30), np.int64), 24)
    assert not bits.any() and not metric.any()


# ---- the library, without a device ----

def _lib():
    import gfdm_amd
    return gfdm_amd.lib()


def test_check_table():
    import gfdm_amd
    L = _lib()
    chk = L.gfdm_hip_conv_code_check
    ok = [(109, 79, 0, 1, 0), (109, -79, 1, 456, 64), (-127, 127, 0, (1 << 20) - 6, 1), (1, 1, 1, 1 << 20, 1), (55, 79, 0, 1, 1 << 40)]
    for a in ok:
        assert chk(*a) == gfdm_amd.capi.OK, a
    bad = [(0, 79, 0, 8, 1), (109, 0, 0, 8, 1), (128, 79, 0, 8, 1), (109, -128, 0, 8, 1), (109, 79, 2, 8, 1), (109, 79, -1, 8, 1), (109, 79, 0, 0, 1),
           (109, 79, 0, -5, 1), (109, 79, 0, (1 << 20) - 5, 1), (109, 79, 1, (1 << 20) + 1, 1), (109, 79, 0, 1 << 62, 1), (109, 79, 0, 8, -1),
           (109, 79, 0, 1 << 19, 1 << 44)]
    for a in bad:
        assert chk(*a) == gfdm_amd.capi.EINVAL, a
        assert L.gfdm_hip_last_error()
    assert L.gfdm_hip_conv_code_steps(None, 8) == gfdm_amd.capi.EINVAL
    assert L.gfdm_hip_conv_code_poly(None, 0) == 0


def test_constructor_table_and_enodev():
    import gfdm_amd
    for polys, mode in (((0, 79), "terminated"), ((109, 200), "terminated"), ((109, 79), 7)):
        with pytest.raises(ValueError):
            gfdm_amd.ConvolutionalCode(polys, mode)
    if have_gpu():                                           # where a device is visible the same call succeeds
        cc = gfdm_amd.ConvolutionalCode((109, -79), "truncated")
        assert cc.polys() == (109, -79) and cc.mode() == "truncated"
        return
    with pytest.raises(gfdm_amd.GfdmHipError) as e:
        gfdm_amd.ConvolutionalCode()
    assert e.value.status == gfdm_amd.capi.ENODEV
    h = ctypes.c_void_p(1)
    assert _lib().gfdm_hip_conv_code_create(ctypes.byref(h), 109, 79, 0, 0) == gfdm_amd.capi.ENODEV and not h.value


def test_size_formulas_of_the_reference():
    for n_info, mode in itertools.product((1, 2, 7, 8, 9, 456, 2042), (V.TERMINATED, V.TRUNCATED)):
        T = n_info + (6 if mode == V.TERMINATED else 0)
        assert V.steps(n_info, mode) == T and V.coded_bits(n_info, mode) == 2 * T
        assert V.coded_bytes(n_info, mode) == -(-2 * T // 8) and V.info_bytes(n_info) == -(-n_info // 8)
    import gfdm_amd
    assert gfdm_amd.ConvolutionalCode.__init__.__defaults__ == ((109, 79), "terminated", 0)


def test_coding_gain_inputs():
    """the inputs of the GPU coding-gain test: the reference decodes every row although about one coded bit in twenty has the wrong sign"""
    payload, llr, c = V.coding_gain_case()
    assert payload.shape == (64, 57) and llr.shape == (64, 924) and llr.dtype == np.float32
    wrong = int(((llr < 0) != (c == 1)).sum())
    got, metric = V.decode(llr, V.GAIN_N_INFO, V.GAIN_GAIN)
    errors = int(np.unpackbits(got ^ payload, axis=1).sum())
    print("coding-gain case: %d of %d coded bits with the wrong sign, %d of %d information bits wrong" % (wrong, c.size, errors, 64 * 456))
    assert errors == 0 and np.array_equal(got, payload)
    assert 2000 < wrong < 3600                               # Q(1 / 0.6) = 4.8 % of 59 136 is 2 830
    sat = float(np.mean(np.abs(V.quantise(llr, V.GAIN_GAIN)) == 127))
    assert 0.0 < sat < 1.0                                    # part of the values saturates, part does not
