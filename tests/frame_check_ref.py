"""numpy restatement of the frame check's contract (include/gfdm_hip.h, gfdm_hip_frame_check): the bitwise CRC-32, the Fibonacci LFSR of
the whitening sequence, attach and verify.  It follows the header's formulas line by line and imports nothing from the product;
tests/test_frame_check.py holds it to zlib and to facts about the sequences that do not depend on it."""
import functools

import numpy as np

POLY = 0xEDB88320
MAX_PAYLOAD = 2 ** 17 - 4


def crc32(data):
    """r = 0xFFFFFFFF; for every byte b: r ^= b, then eight times r = (r >> 1) ^ (POLY if r & 1 else 0); the CRC is r ^ 0xFFFFFFFF"""
    r = 0xFFFFFFFF
    for b in bytes(data):
        r ^= b
        for _ in range(8):
            r = (r >> 1) ^ (POLY if r & 1 else 0)
    return r ^ 0xFFFFFFFF


def crc32_rows(rows):
    """crc32 of every row of a uint8 array (n_rows, n): the same formula, the rows side by side"""
    rows = np.ascontiguousarray(rows, np.uint8)
    if rows.shape[0] < 8:                                    # a few long rows: the scalar loop is the faster one
        return np.array([crc32(row.tobytes()) for row in rows], np.uint32)
    r = np.full(rows.shape[0], 0xFFFFFFFF, np.uint32)
    for j in range(rows.shape[1]):
        r ^= rows[:, j]
        for _ in range(8):
            r = (r >> np.uint32(1)) ^ np.where(r & np.uint32(1), np.uint32(POLY), np.uint32(0))
    return r ^ np.uint32(0xFFFFFFFF)


def lfsr_bits(n, mask, seed, degree):
    """w_0 .. w_{n-1}: s_0 = seed, w_i = s_i & 1, s_{i+1} = (s_i >> 1) | (parity(s_i & mask) << (degree - 1)); all zeros for degree 0"""
    w = np.zeros(n, np.uint8)
    if degree == 0:
        return w
    s = int(seed)
    for i in range(n):
        w[i] = s & 1
        s = (s >> 1) | ((bin(s & mask).count("1") & 1) << (degree - 1))
    return w


@functools.lru_cache(maxsize=None)
def whitening(frame_bytes, mask, seed, degree):
    """the packed sequence of a frame row: bit i of the sequence on bit i of the row, MSB first (computed once, read-only)"""
    seq = np.packbits(lfsr_bits(8 * frame_bytes, mask, seed, degree))
    seq.setflags(write=False)
    return seq


def attach(payload, n_payload, mask=0x11, seed=0x7F, degree=7, out_row_bytes=None):
    """payload (n_rows, >= n_payload) uint8 -> frames (n_rows, out_row_bytes): the payload, its CRC least significant byte first,
    the whitening over both, zeros behind"""
    payload = np.ascontiguousarray(payload, np.uint8)[:, :n_payload]
    width = n_payload + 4 if out_row_bytes is None else out_row_bytes
    out = np.zeros((payload.shape[0], width), np.uint8)
    out[:, :n_payload] = payload
    crc = crc32_rows(payload)
    for j in range(4):
        out[:, n_payload + j] = (crc >> np.uint32(8 * j)) & np.uint32(0xFF)
    out[:, :n_payload + 4] ^= whitening(n_payload + 4, mask, seed, degree)
    return out


def verify(frames, n_payload, mask=0x11, seed=0x7F, degree=7, out_row_bytes=None):
    """frames (n_rows, >= n_payload + 4) uint8 -> (payload (n_rows, out_row_bytes), ok uint8 (n_rows,), good_row int64 (n_rows,), n_good)"""
    plain = np.ascontiguousarray(frames, np.uint8)[:, :n_payload + 4] ^ whitening(n_payload + 4, mask, seed, degree)
    width = n_payload if out_row_bytes is None else out_row_bytes
    payload = np.zeros((plain.shape[0], width), np.uint8)
    payload[:, :n_payload] = plain[:, :n_payload]
    stored = np.zeros(plain.shape[0], np.uint32)
    for j in range(4):
        stored |= plain[:, n_payload + j].astype(np.uint32) << np.uint32(8 * j)
    ok = (crc32_rows(plain[:, :n_payload]) == stored).astype(np.uint8)
    good = np.flatnonzero(ok).astype(np.int64)
    good_row = np.full(plain.shape[0], -1, np.int64)
    good_row[:len(good)] = good
    return payload, ok, good_row, len(good)


def limit(payload, ok, count):
    """what a call with `count` leaves of verify's results: rows from clamp(count, 0, n_rows) on are zeros and not good"""
    n = len(ok)
    live = n if count is None else min(max(int(count), 0), n)
    payload, ok = payload.copy(), ok.copy()
    payload[live:], ok[live:] = 0, 0
    good = np.flatnonzero(ok).astype(np.int64)
    good_row = np.full(n, -1, np.int64)
    good_row[:len(good)] = good
    return payload, ok, good_row, len(good)
