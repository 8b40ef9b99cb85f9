"""numpy restatement of the convolutional code of include/gfdm_hip.h (gfdm_hip_conv_code): encoder, quantiser and Viterbi decoder exactly as
the header's formulas state them, in integers, vectorised over rows and states with a Python loop over the trellis steps.  It is the
yardstick of tests/test_conv_code_gpu.py and is itself held to facts that do not depend on it by tests/test_conv_code.py."""
import functools

import numpy as np

TERMINATED, TRUNCATED = "terminated", "truncated"
POLYS = (109, 79)                       # 171 / 133 octal
NEG = -(1 << 30)
LDS_STEPS = 2048                        # GFDM_HIP_CC_LDS_STEPS of the header


def steps(n_info, mode=TERMINATED):
    return n_info + 6 if mode == TERMINATED else n_info


def coded_bits(n_info, mode=TERMINATED):
    return 2 * steps(n_info, mode)


def coded_bytes(n_info, mode=TERMINATED):
    return (coded_bits(n_info, mode) + 7) // 8


def info_bytes(n_info):
    return (n_info + 7) // 8


def parity(x):
    x = np.asarray(x)
    p = np.zeros_like(x)
    for d in range(7):
        p ^= (x >> d) & 1
    return p


def output_bit(R, g):
    """c_i(R) = parity(R & |g|) XOR (g < 0)"""
    return parity(np.asarray(R) & abs(g)) ^ (1 if g < 0 else 0)


def unpack(rows, n_bits):
    """packed bytes (n_rows, >= ceil(n_bits / 8)) -> bits (n_rows, n_bits), MSB first"""
    rows = np.atleast_2d(np.asarray(rows, np.uint8))
    return np.unpackbits(rows, axis=1)[:, :n_bits]


def pack(bits, width=None):
    """bits (n_rows, n) -> packed bytes (n_rows, width or ceil(n / 8)), MSB first, zero padded"""
    bits = np.atleast_2d(np.asarray(bits, np.uint8))
    out = np.packbits(bits, axis=1)
    if width is not None and width > out.shape[1]:
        out = np.concatenate((out, np.zeros((out.shape[0], width - out.shape[1]), np.uint8)), axis=1)
    return out


def encode_bits(u, polys=POLYS, mode=TERMINATED):
    """information bits (n_rows, n_info) -> coded bits (n_rows, 2 T)"""
    u = np.atleast_2d(np.asarray(u, np.int64))
    if mode == TERMINATED:
        u = np.concatenate((u, np.zeros((u.shape[0], 6), np.int64)), axis=1)
    T = u.shape[1]
    padded = np.concatenate((np.zeros((u.shape[0], 6), np.int64), u), axis=1)
    R = np.zeros((u.shape[0], T), np.int64)
    for d in range(7):
        R |= padded[:, 6 - d:6 - d + T] << d                 # u_{t-d} << d
    c = np.empty((u.shape[0], 2 * T), np.uint8)
    c[:, 0::2] = output_bit(R, polys[0])
    c[:, 1::2] = output_bit(R, polys[1])
    return c


def encode(data, n_info, polys=POLYS, mode=TERMINATED, out_row_bytes=None):
    """information bytes (n_rows, info_bytes) -> coded bytes (n_rows, out_row_bytes or coded_bytes); the spare bits of the input are ignored"""
    return pack(encode_bits(unpack(data, n_info), polys, mode), out_row_bytes)


def quantise(llr, gain):
    """q = clamp(rintf(llr * gain), -127, 127) with the product in float32; NaN gives 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(llr, np.float32) * np.float32(gain))          # float32 * float32 -> float32; rint is half to even
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, -127, 127).astype(np.int64)


def hard_values(coded, n_info, mode=TERMINATED):
    """packed coded rows -> q = +1 for a 0 bit, -1 for a 1 bit"""
    return 1 - 2 * unpack(coded, coded_bits(n_info, mode)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _signs(polys):
    s = np.arange(64)
    return np.array([[1 - 2 * output_bit(s | (b << 6), g) for g in polys] for b in range(2)], np.int64)      # [b][i][state]


def viterbi(q, n_info, polys=POLYS, mode=TERMINATED):
    """q: int soft values (n_rows, >= 2 T) -> (bits (n_rows, n_info) uint8, path_metric (n_rows,) int32)"""
    q = np.atleast_2d(np.asarray(q, np.int64))
    n, T = q.shape[0], steps(n_info, mode)
    sg = _signs(tuple(polys))
    s = np.arange(64)
    pm = np.full((n, 64), NEG, np.int64)
    pm[:, 0] = 0
    dec = np.zeros((T, n, 64), bool)
    for t in range(T):
        q0, q1 = q[:, 2 * t, None], q[:, 2 * t + 1, None]
        m0 = pm[:, s >> 1] + sg[0, 0] * q0 + sg[0, 1] * q1
        m1 = pm[:, (s >> 1) + 32] + sg[1, 0] * q0 + sg[1, 1] * q1
        dec[t] = m1 > m0                                     # strict: a tie keeps b = 0
        pm = np.where(dec[t], m1, m0)
    assert np.abs(pm).max() < 2 ** 31
    state = np.zeros(n, np.int64) if mode == TERMINATED else np.argmax(pm, axis=1)          # argmax: the first maximum
    metric = pm[np.arange(n), state].astype(np.int32)
    u = np.zeros((n, T), np.uint8)
    rows = np.arange(n)
    for t in range(T - 1, -1, -1):
        u[:, t] = state & 1
        state = (state >> 1) | (dec[t, rows, state].astype(np.int64) << 5)
    return u[:, :n_info], metric


def decode(llr, n_info, gain, polys=POLYS, mode=TERMINATED):
    """LLRs (n_rows, >= 2 T) -> (information bytes (n_rows, info_bytes), path_metric)"""
    llr = np.atleast_2d(llr)[:, :coded_bits(n_info, mode)]
    bits, metric = viterbi(quantise(llr, gain), n_info, polys, mode)
    return pack(bits), metric


def decode_hard(coded, n_info, polys=POLYS, mode=TERMINATED):
    bits, metric = viterbi(hard_values(coded, n_info, mode), n_info, polys, mode)
    return pack(bits), metric


def random_info(rng, n_rows, n_info):
    """random information rows; the spare low bits of the last byte are random too (encode must ignore them)"""
    return rng.integers(0, 256, (n_rows, info_bytes(n_info)), dtype=np.uint8)


def clean(data, n_info):
    """information rows with the spare bits of the last byte zeroed: what decode gives back"""
    return pack(unpack(data, n_info))


# ---- the coding-gain case: 64 rows of n_info = 456 (57 bytes: one K = 64, M = 9, 52-subcarrier QPSK frame at rate 1/2 with 12 pad bits),
# BPSK +-1 plus Gaussian noise of sigma 0.6, LLR 2 y / sigma^2, gain 8 ----
GAIN_ROWS, GAIN_N_INFO, GAIN_SIGMA, GAIN_GAIN, GAIN_SEED = 64, 456, 0.6, 8.0, 2024


@functools.lru_cache(maxsize=None)
def coding_gain_case():
    """(payload bytes (64, 57), llr float32 (64, 924), coded bits (64, 924))"""
    rng = np.random.default_rng(GAIN_SEED)
    payload = rng.integers(0, 256, (GAIN_ROWS, info_bytes(GAIN_N_INFO)), dtype=np.uint8)
    c = encode_bits(unpack(payload, GAIN_N_INFO))
    y = (1.0 - 2.0 * c) + GAIN_SIGMA * rng.standard_normal(c.shape)
    llr = (2.0 * y / GAIN_SIGMA ** 2).astype(np.float32)
    for a in (payload, llr, c):
        a.setflags(write=False)
    return payload, llr, c
