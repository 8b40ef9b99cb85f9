"""numpy restatement of the rate matcher of include/gfdm_hip.h (gfdm_hip_rate_matcher): the puncturing pattern, the permutation and the
gather convention exactly as the header states them, in integer index arithmetic.  It is the yardstick of tests/test_rate_match_gpu.py
and is itself held to facts that do not depend on it by tests/test_rate_match.py.  It imports nothing from the product."""
import functools

import numpy as np

import conv_code_ref as V

LDS_BITS = 8192                         # GFDM_HIP_RM_LDS_BITS of the header
RATES = {"1/2": [1, 1], "2/3": [1, 1, 1, 0], "3/4": [1, 1, 1, 0, 0, 1], "5/6": [1, 1, 1, 0, 0, 1, 1, 0, 0, 1]}


def kept(n_coded, keep=None):
    """k_0 < ... < k_{n_tx-1}: the positions i of the coded row with keep[i mod P] != 0"""
    keep = np.ones(1, np.uint8) if keep is None else np.asarray(keep).ravel()
    i = np.arange(n_coded)
    return i[keep[i % keep.size] != 0]


def source_index(n_coded, keep=None, perm=None):
    """src[j] = k_{perm[j]}: transmitted bit j is coded bit src[j]"""
    k = kept(n_coded, keep)
    return k if perm is None else k[np.asarray(perm, np.int64)]


def inverse_index(n_coded, src):
    """inv[i]: the transmitted bit behind coded bit i, -1 where it is punctured"""
    inv = np.full(n_coded, -1, np.int64)
    inv[src] = np.arange(len(src))
    return inv


def block(n, columns):
    """0 .. rows * columns - 1 written row-wise into rows = ceil(n / columns) rows, read column-wise, the indices >= n dropped"""
    rows = -(-n // columns)
    a = np.arange(rows * columns).reshape(rows, columns).T.ravel()
    return a[a < n]


def match(coded, n_coded, keep=None, perm=None, out_row_bytes=None):
    """packed coded bytes (n_rows, >= ceil(n_coded / 8)) -> packed transmitted bytes (n_rows, out_row_bytes or ceil(n_tx / 8)), zero padded"""
    src = source_index(n_coded, keep, perm)
    return V.pack(V.unpack(coded, n_coded)[:, src], out_row_bytes)


def _spread(values, n_coded, src, out_stride):
    values = np.atleast_2d(values)
    out = np.zeros((values.shape[0], n_coded if out_stride is None else out_stride), np.float32)
    out.view(np.uint32)[:, src] = values[:, :len(src)].view(np.uint32)          # a bit copy: no float ever passes through arithmetic
    return out


def unmatch(llr, n_coded, keep=None, perm=None, out_stride=None):
    """float32 (n_rows, >= n_tx) -> float32 (n_rows, out_stride or n_coded): out[src[j]] = in[j] bit for bit, +0.0 elsewhere"""
    return _spread(np.ascontiguousarray(llr, np.float32), n_coded, source_index(n_coded, keep, perm), out_stride)


def unmatch_hard(tx, n_coded, keep=None, perm=None, out_stride=None):
    """packed transmitted bytes (n_rows, >= ceil(n_tx / 8)) -> float32 rows as unmatch's: +1.0 for a 0 bit, -1.0 for a 1 bit, +0.0 elsewhere"""
    src = source_index(n_coded, keep, perm)
    return _spread((1.0 - 2.0 * V.unpack(tx, len(src))).astype(np.float32), n_coded, src, out_stride)


# ---- the decoding cases: rows of n_info = 456 (one K = 64, M = 9, 52-subcarrier QPSK frame at rate 1/2), block interleaver of 18 columns ----
CASE_N_INFO, CASE_COLUMNS, CASE_GAIN = 456, 18, 8.0
# coding gain under puncturing: rate -> (sigma, n_tx, transmitted values with the wrong sign); BPSK +-1 plus Gaussian noise, LLR 2 y / sigma^2
GAIN_CASES = {"2/3": (0.5, 693, 969), "3/4": (0.45, 616, 502), "5/6": (0.4, 555, 206)}
BURST_ROWS, BURST_LEN = 16, 48


@functools.lru_cache(maxsize=None)
def coding_gain_case(rate):
    """(payload bytes (64, 57), coded bits (64, 924), transmitted bits (64, n_tx), llr float32 (64, n_tx), perm, the noise in llr)"""
    sigma = GAIN_CASES[rate][0]
    rng = np.random.default_rng(2025)
    payload = rng.integers(0, 256, (64, V.info_bytes(CASE_N_INFO)), dtype=np.uint8)
    c = V.encode_bits(V.unpack(payload, CASE_N_INFO))
    k = kept(c.shape[1], RATES[rate])
    perm = block(len(k), CASE_COLUMNS)
    tx = c[:, k][:, perm]
    noise = sigma * rng.standard_normal(tx.shape)
    llr = gain_llr(tx, noise, sigma)
    for a in (payload, c, tx, llr, perm, noise):
        a.setflags(write=False)
    return payload, c, tx, llr, perm, noise


def gain_llr(tx, noise, sigma):
    """LLR 2 y / sigma^2 of y = (1 - 2 tx) + noise, float32"""
    return (2.0 * ((1.0 - 2.0 * tx) + noise) / sigma ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def burst_case(rate):
    """(payload bytes (16, 57), coded bits (16, 924), keep): the rows of the burst-erasure case"""
    rng = np.random.default_rng(7)
    payload = rng.integers(0, 256, (BURST_ROWS, V.info_bytes(CASE_N_INFO)), dtype=np.uint8)
    c = V.encode_bits(V.unpack(payload, CASE_N_INFO))
    for a in (payload, c):
        a.setflags(write=False)
    return payload, c, RATES[rate]


def burst_llrs(tx, starts):
    """noise-free LLRs 4 (1 - 2 tx) of the transmitted bits (n_rows, n_tx), once per start with BURST_LEN consecutive values from the
    start on erased: float32 (len(starts) * n_rows, n_tx), the rows of one start together"""
    llr = np.tile((4.0 * (1.0 - 2.0 * tx)).astype(np.float32), (len(starts), 1)).reshape(len(starts), tx.shape[0], tx.shape[1])
    for a, s in enumerate(starts):
        llr[a, :, s:s + BURST_LEN] = 0.0
    return llr.reshape(-1, tx.shape[1])
