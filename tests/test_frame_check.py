"""CPU tests of the frame check (contract in include/gfdm_hip.h, gfdm_hip_frame_check): the numpy restatement of
tests/frame_check_ref.py held to facts that do not depend on it -- zlib's CRC-32 and its residue, the period and balance of the
whitening sequences -- attach and verify of the restatement against each other, and what the library answers without a device: the
argument table and the constructor's refusals and its ENODEV.  The device calls are in tests/test_frame_check_gpu.py."""
import ctypes
import zlib

import numpy as np
import pytest

import frame_check_ref as F
from conftest import have_gpu


# ---- the restatement ----

def test_crc_is_zlibs():
    assert F.crc32(b"") == zlib.crc32(b"") == 0
    assert F.crc32(b"123456789") == 0xCBF43926 == zlib.crc32(b"123456789")
    rng = np.random.default_rng(1)
    for n in (1, 15, 16, 17, 57, 1024, 1025):
        rows = rng.integers(0, 256, (9, n), dtype=np.uint8)
        want = [zlib.crc32(row.tobytes()) for row in rows]
        assert [F.crc32(row.tobytes()) for row in rows] == want, n
        assert F.crc32_rows(rows).tolist() == want and F.crc32_rows(rows[:2]).tolist() == want[:2], n      # side by side, and the scalar loop


def test_crc_of_payload_and_crc_is_the_residue():
    """zlib.crc32(payload + crc, least significant byte first) is one constant for every payload"""
    rng = np.random.default_rng(2)
    residue = zlib.crc32(b"" + zlib.crc32(b"").to_bytes(4, "little"))
    assert residue == 0x2144DF1C
    for n in (1, 3, 16, 57, 200):
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert zlib.crc32(payload + zlib.crc32(payload).to_bytes(4, "little")) == residue
        frame = F.attach(np.frombuffer(payload, np.uint8)[None, :], n, degree=0)[0]
        assert zlib.crc32(frame.tobytes()) == residue and frame[:n].tobytes() == payload


@pytest.mark.parametrize("mask", [0x11, 0x09])
def test_degree_7_sequences_have_period_127_and_64_ones(mask):
    for seed in range(1, 128):
        w = F.lfsr_bits(3 * 127 + 5, mask, seed, 7)
        assert np.array_equal(w[:-127], w[127:]), seed
        assert int(w[:127].sum()) == 64, seed
        for p in range(1, 127):
            if 127 % p == 0:                                 # 127 is prime: the only shorter period would be 1
                assert not np.array_equal(w[:-p], w[p:]), (seed, p)
        for i in range(200):                                 # w_{i+7} = XOR over the set bits j of mask of w_{i+j}
            assert w[i + 7] == np.bitwise_xor.reduce([w[i + j] for j in range(7) if (mask >> j) & 1])


def test_other_sequences():
    assert F.lfsr_bits(40, 1, 1, 1).tolist() == [1] * 40                   # degree 1: the state is its own parity
    assert not F.lfsr_bits(40, 0x11, 0x7F, 0).any()                        # degree 0: no whitening
    mask = 0x80200003                                                      # x^32 + x^31 + x^21 + x + 1 in this convention: taps at 0, 1, 21, 31
    w = F.lfsr_bits(5000, mask, 0xFFFFFFFF, 32)
    assert w[:32].all() and not w[32:].all()                               # the seed comes out first
    for i in range(4000):                                                  # no overflow: bit 31 feeds back, the recurrence holds throughout
        assert w[i + 32] == w[i] ^ w[i + 1] ^ w[i + 21] ^ w[i + 31]
    seq = F.whitening(3, 0x11, 0x7F, 7)
    assert seq[0] == 0xFE and np.array_equal(np.unpackbits(seq), F.lfsr_bits(24, 0x11, 0x7F, 7))      # seven ones, MSB first


def test_verify_of_attach_is_the_payload():
    rng = np.random.default_rng(3)
    for n, lfsr in ((1, (0x11, 0x7F, 7)), (57, (0x11, 0x7F, 7)), (57, (1, 1, 0)), (124, (0x80200003, 0xDEADBEEF, 32)), (16, (0x09, 0x01, 7))):
        x = rng.integers(0, 256, (9, n + 2), dtype=np.uint8)
        frames = F.attach(x, n, *lfsr, out_row_bytes=n + 7)
        assert frames.shape == (9, n + 7) and not frames[:, n + 4:].any()
        payload, ok, good_row, n_good = F.verify(frames, n, *lfsr, out_row_bytes=n + 1)
        assert np.array_equal(payload[:, :n], x[:, :n]) and not payload[:, n:].any()
        assert ok.tolist() == [1] * 9 and good_row.tolist() == list(range(9)) and n_good == 9
        plain = frames[:, :n + 4] ^ F.whitening(n + 4, *lfsr)
        assert all(zlib.crc32(row[:n].tobytes()) == int.from_bytes(row[n:].tobytes(), "little") for row in plain)


def test_every_single_bit_flip_of_a_61_byte_frame_is_caught():
    rng = np.random.default_rng(4)
    n = 57
    frame = F.attach(rng.integers(0, 256, (1, n), dtype=np.uint8), n)[0]
    assert frame.size == 61
    flipped = np.tile(frame, (8 * 61 + 1, 1))
    for i in range(8 * 61):
        flipped[i, i >> 3] ^= 0x80 >> (i & 7)
    _, ok, good_row, n_good = F.verify(flipped, n)
    assert not ok[:-1].any() and ok[-1] == 1
    assert good_row.tolist() == [8 * 61] + [-1] * (8 * 61) and n_good == 1


def test_an_all_zero_payload_is_sent_as_the_sequence():
    n = 57
    frame = F.attach(np.zeros((1, n), np.uint8), n)[0]
    bits = np.unpackbits(frame)
    assert np.array_equal(bits[:127], F.lfsr_bits(127, 0x11, 0x7F, 7)) and np.array_equal(bits[:8 * n], F.lfsr_bits(8 * n, 0x11, 0x7F, 7))
    assert int(bits[:127].sum()) == 64
    plain = F.attach(np.zeros((1, n), np.uint8), n, degree=0)[0]
    assert not plain[:n].any() and int.from_bytes(plain[n:].tobytes(), "little") == zlib.crc32(bytes(n))


# ---- the library, without a device ----

MAXP = 2 ** 17 - 4
GOOD = [(1, 0x11, 0x7F, 7), (57, 0x11, 0x7F, 7), (MAXP, 0x09, 0x01, 7), (57, 1, 1, 1), (57, 0, 0, 0), (57, 12345, 0, 0), (57, 0x80200003, 0xFFFFFFFF, 32),
        (57, 0xFFFFFFFF, 1, 32), (57, 0x3, 0x2, 2)]
BAD = [((0, 0x11, 0x7F, 7), "n_payload 0"), ((-3, 0x11, 0x7F, 7), "n_payload negative"), ((MAXP + 1, 0x11, 0x7F, 7), "n_payload above 2^17 - 4"),
       ((57, 0x11, 0x7F, -1), "degree negative"), ((57, 0x11, 0x7F, 33), "degree 33"), ((57, 0, 0x7F, 7), "mask 0"), ((57, 0x11, 0, 7), "seed 0"),
       ((57, 0x80, 0x7F, 7), "mask 2^d"), ((57, 0x11, 0x80, 7), "seed 2^d"), ((57, 2, 1, 1), "mask 2^d, d = 1"), ((57, 1 << 32, 1, 32), "mask 2^32"),
       ((57, 1, 1 << 32, 32), "seed 2^32"), ((57, (1 << 63) + 1, 1, 32), "mask beyond 2^63")]


def _lib():
    import gfdm_amd
    return gfdm_amd.lib()


def test_check_table():
    import gfdm_amd
    L = _lib()
    OK, EINVAL = gfdm_amd.capi.OK, gfdm_amd.capi.EINVAL
    for a in GOOD:
        assert L.gfdm_hip_frame_check_check(*a, 5) == OK, a
        gfdm_amd.FrameCheck.check(*a, n_rows=5)
    for a, what in BAD:
        assert L.gfdm_hip_frame_check_check(*a, 1) == EINVAL, what
        assert L.gfdm_hip_last_error(), what
        with pytest.raises(ValueError):
            gfdm_amd.FrameCheck.check(*a)
    assert L.gfdm_hip_frame_check_check(57, 0x11, 0x7F, 7, -1) == EINVAL                               # n_rows < 0
    assert L.gfdm_hip_frame_check_check(57, 0x11, 0x7F, 7, 0) == OK
    assert L.gfdm_hip_frame_check_check(MAXP, 0x11, 0x7F, 7, 1 << 47) == EINVAL                        # 2^17 * 2^47 bytes
    assert L.gfdm_hip_frame_check_check(MAXP, 0x11, 0x7F, 7, 1 << 45) == OK
    assert L.gfdm_hip_frame_check_check(1, 0x11, 0x7F, 7, 1 << 60) == EINVAL                           # 8 bytes of good_row a row
    assert L.gfdm_hip_frame_check_check(1, 0x11, 0x7F, 7, 1 << 59) == OK
    for bad in (dict(mask=-1), dict(seed=-1), dict(mask=1 << 64, degree=32)):
        with pytest.raises(ValueError):
            gfdm_amd.FrameCheck.check(57, **bad)
    for getter in ("payload_bytes", "frame_bytes", "frame_bits"):
        assert getattr(L, "gfdm_hip_frame_check_" + getter)(None) == EINVAL
    assert L.gfdm_hip_frame_check_whitening(None, None) == EINVAL
    # the calls refuse a NULL handle before anything else
    assert L.gfdm_hip_frame_check_attach_host(None, None, None, None, 57, 61, 1) == EINVAL
    assert L.gfdm_hip_frame_check_verify_device(None, None, None, None, None, None, None, 61, 57, 1, None) == EINVAL


def test_create_refuses_its_arguments_before_it_looks_for_a_device():
    """Every refusal of the constructor is EINVAL where no device exists as well: the checks, the sequence and the constants are made
    before the handle's context is opened (gfdm::create_handle).  A valid constructor then answers ENODEV here, and works where a GPU
    is visible."""
    import gfdm_amd
    L = _lib()
    for a, what in BAD:
        h = ctypes.c_void_p(1)
        assert L.gfdm_hip_frame_check_create(ctypes.byref(h), *a, 0) == gfdm_amd.capi.EINVAL and not h.value, what
        with pytest.raises(ValueError):
            gfdm_amd.FrameCheck(*a)
    assert L.gfdm_hip_frame_check_create(None, 57, 0x11, 0x7F, 7, 0) == gfdm_amd.capi.EINVAL            # a NULL handle pointer
    assert gfdm_amd.FrameCheck.__init__.__defaults__ == (0x11, 0x7F, 7, 0)
    if have_gpu():
        fc = gfdm_amd.FrameCheck(57)
        assert (fc.payload_bytes, fc.frame_bytes, fc.frame_bits) == (57, 61, 488)
        assert np.array_equal(fc.whitening, F.whitening(61, 0x11, 0x7F, 7))
        return
    for a in GOOD[:2] + GOOD[4:5]:
        with pytest.raises(gfdm_amd.GfdmHipError) as e:
            gfdm_amd.FrameCheck(*a)
        assert e.value.status == gfdm_amd.capi.ENODEV
