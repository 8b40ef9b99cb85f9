"""numpy restatement of the link meter's contract (include/gfdm_hip.h, gfdm_hip_link_meter): the matching rule in plain Python loops,
bit errors and the two powers of every row in float64 on the float32 inputs, and the totals a call adds.  The yardstick of
tests/test_link_meter.py and tests/test_link_meter_gpu.py: nothing here calls the library.  Decisions, bit packing and the seeded cases
are tests/symbol_mapper_ref.py's, unchanged."""
import numpy as np

import symbol_mapper_ref as S

TILE = 2048                      # symbols per tile of the measure kernel: n_sym = 4097 is a row longer than two of them
BUDGET = 2.0 ** -19              # |got - ref| <= BUDGET * ref for err_power and ref_power
FIELDS = ("rows", "symbols", "bits", "bit_errors", "symbol_errors", "row_errors", "detections", "matched", "missed", "false_alarms")


def zero_totals():
    return {f: 0 for f in FIELDS}


def add_totals(*parts):
    out = zero_totals()
    for p in parts:
        for f, v in p.items():
            out[f] += int(v)
    return out


def match(frame_start, sent_pos, tol, offset=0, count=None):
    """(ref_row (n_rows,), sent_row (n_sent,), totals): the contract's rule, one loop per sentence of it"""
    fs = [int(v) for v in np.asarray(frame_start).ravel()]
    e = [int(v) + int(offset) for v in np.asarray(sent_pos).ravel()]
    n_rows, n_sent = len(fs), len(e)
    n_live = S.live(count, n_rows)
    detections = [d for d in range(n_live) if fs[d] >= 0]
    proposes = {}                                                # d -> (j, distance)
    for d in detections:
        best = None
        for j in range(n_sent):
            dist = abs(fs[d] - e[j])
            if best is None or dist < best[1]:                   # strict: the lower j on a tie
                best = (j, dist)
        if best is not None and best[1] <= tol:
            proposes[d] = best
    ref_row, sent_row = [-1] * n_rows, [-1] * n_sent
    for j in range(n_sent):
        bids = sorted((dist, d) for d, (jj, dist) in proposes.items() if jj == j)
        if bids:
            sent_row[j] = bids[0][1]
            ref_row[bids[0][1]] = j
    winners = sum(1 for d in sent_row if d >= 0)
    totals = zero_totals()
    totals.update(detections=len(detections), matched=winners, missed=n_sent - winners, false_alarms=len(detections) - winners)
    return np.array(ref_row, np.int64), np.array(sent_row, np.int64), totals


def measured_rows(n_rows, n_ref, ref_row=None, count=None, aided=True):
    """(ref (n_rows,) int64, measured (n_rows,) bool)"""
    ref = np.arange(n_rows, dtype=np.int64) if ref_row is None else np.asarray(ref_row, np.int64)
    ok = (np.arange(n_rows) < S.live(count, n_rows)) & (ref >= 0)
    if aided:
        ok &= ref < n_ref
    return ref, ok


def measure(symbols, points, rule, payload=None, ref_row=None, count=None):
    """dict: bit_errors (int64, -1 unmeasured; None when decision-directed), err_power, ref_power (float64), symbol_errors (per row), measured,
    idx (the decisions, 0 in unmeasured rows), totals.  Unmeasured rows are not looked at."""
    x = np.asarray(symbols, np.complex64)
    p = np.asarray(points, np.complex64)
    k = S.bits_per_symbol(p)
    n_rows, n_sym = x.shape
    aided = payload is not None
    n_ref = len(payload) if aided else 0
    ref, ok = measured_rows(n_rows, n_ref, ref_row, count, aided)
    idx = np.zeros((n_rows, n_sym), np.int64)
    idx[ok] = S.indices(x[ok], p, rule)
    sent = idx.copy()
    if aided:
        sent[ok] = S.unpack(np.asarray(payload, np.uint8)[ref[ok]], n_sym, k)
    pp = p[sent].astype(np.complex128)
    xx = np.where(ok[:, None], x, 0).astype(np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        err = ((xx.real - pp.real) ** 2 + (xx.imag - pp.imag) ** 2).sum(axis=1)
    refp = (pp.real ** 2 + pp.imag ** 2).sum(axis=1)
    err[~ok], refp[~ok] = 0, 0
    flips = idx ^ sent
    bits = np.zeros((n_rows, n_sym), np.int64)
    for j in range(k):
        bits += (flips >> j) & 1
    be = bits.sum(axis=1)
    se = (flips != 0).sum(axis=1)
    be[~ok], se[~ok] = -1, 0
    totals = zero_totals()
    n = int(ok.sum())
    totals.update(rows=n, symbols=n * n_sym)
    if aided:
        totals.update(bits=n * n_sym * k, bit_errors=int(be[ok].sum()), symbol_errors=int(se[ok].sum()), row_errors=int((be[ok] > 0).sum()))
    return dict(bit_errors=be if aided else None, err_power=err, ref_power=refp, symbol_errors=se, measured=ok, idx=idx, totals=totals)


def popcount_rows(a, b, n_sym, k):
    """per row: the number of differing live bits of two packed arrays (n_rows, row_bytes)"""
    mask = S.spare_mask(n_sym, k)
    return np.unpackbits((np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)) & mask, axis=1).sum(axis=1).astype(np.int64)


# (frame_start, sent_pos, tol, offset, count) -> (ref_row, sent_row, (detections, matched, missed, false_alarms)): written by hand
KNOWN_MATCHES = [
    # two detections inside tol of one sent burst: the nearer wins
    (([103, 101], [100], 5, 0, None), ([-1, 0], [1], (2, 1, 0, 1))),
    # ... and the lower d on an equal distance
    (([102, 98, 102], [100], 5, 0, None), ([0, -1, -1], [0], (3, 1, 0, 2))),
    # a detection equally far from two sent bursts: the lower j
    (([105], [100, 110], 5, 0, None), ([0], [0, -1], (1, 1, 1, 0))),
    # ... even where the higher j would otherwise stay without a detection, and one beyond tol is a false alarm
    (([105, 117], [100, 110], 5, 0, None), ([0, -1], [0, -1], (2, 1, 1, 1))),
    # frame_start = -1 inside n_live counts nowhere
    (([-1, 100, -1], [100], 0, 0, None), ([-1, 0, -1], [1], (1, 1, 0, 0))),
    # n_sent = 0: every detection is a false alarm
    (([5, 9, -1], [], 3, 0, None), ([-1, -1, -1], [], (2, 0, 0, 2))),
    # n_rows = 0: every sent burst is missed
    (([], [5, 9], 3, 0, None), ([], [-1, -1], (0, 0, 2, 0))),
    # count below, at and beyond n_rows, and negative
    (([10, 20, 30], [10, 20, 30], 0, 0, 2), ([0, 1, -1], [0, 1, -1], (2, 2, 1, 0))),
    (([10, 20, 30], [10, 20, 30], 0, 0, 3), ([0, 1, 2], [0, 1, 2], (3, 3, 0, 0))),
    (([10, 20, 30], [10, 20, 30], 0, 0, 8), ([0, 1, 2], [0, 1, 2], (3, 3, 0, 0))),
    (([10, 20, 30], [10, 20, 30], 0, 0, 0), ([-1, -1, -1], [-1, -1, -1], (0, 0, 3, 0))),
    (([10, 20, 30], [10, 20, 30], 0, 0, -4), ([-1, -1, -1], [-1, -1, -1], (0, 0, 3, 0))),
    # non-ascending detections, an offset, tol = 0 exact and one off
    (([47, 17, 32, 27], [10, 20, 30, 40], 0, 7, None), ([3, 0, -1, 1], [1, 3, -1, 0], (4, 3, 1, 1))),
    # the nearest sent burst is taken, not the first within tol
    (([109], [100, 110], 20, 0, None), ([1], [-1, 0], (1, 1, 1, 0))),
]


def noisy_names():
    """the constellations of the GPU file's decode comparison: k = 1, 2, 2, 3, 4, 6, 8"""
    return ("gr_bpsk", "gr_qpsk", "pygfdm_qpsk", "psk8", "qam16", "qam64", "grid256")


def match_case(seed=5, n_sent=300, n_det=320, tol=3):
    """(frame_start (n_det,), sent_pos (n_sent,) ascending, tol, offset): detections made from a subset of the sent positions +- jitter up to
    tol + 2 (some fall outside tol, some collide on one burst: a second detection of the same burst) plus random false alarms, shuffled,
    with a few -1 among them"""
    rng = np.random.default_rng(seed)
    offset = 17
    sent_pos = np.sort(rng.choice(np.arange(0, 400000, 7), n_sent, replace=False)).astype(np.int64)
    hit = rng.choice(n_sent, 240, replace=False)
    twice = rng.choice(hit, 30, replace=False)
    fs = np.concatenate((sent_pos[hit] + offset + rng.integers(-tol - 2, tol + 3, hit.size),
                         sent_pos[twice] + offset + rng.integers(-tol, tol + 1, twice.size),
                         rng.integers(0, 400000, n_det - hit.size - twice.size - 6), np.full(6, -1)))
    assert fs.size == n_det
    return rng.permutation(fs).astype(np.int64), sent_pos, tol, offset
