"""CPU tests of the rate matcher (contract in include/gfdm_hip.h, gfdm_hip_rate_matcher): the numpy restatement of
tests/rate_match_ref.py and the package's two host helpers held to facts that do not depend on them, what the library answers without a
device -- the argument table, tx_bits_of, the constructor's refusals and its ENODEV -- and the two decoding cases whose device versions
are in tests/test_rate_match_gpu.py, here with tests/conv_code_ref.py alone."""
import ctypes

import numpy as np
import pytest

import conv_code_ref as V
import rate_match_ref as M
from conftest import have_gpu


def test_unmatch_of_match_restores_the_kept_positions():
    rng = np.random.default_rng(1)
    for n_coded, keep, perm_of in ((37, None, None), (924, M.RATES["3/4"], lambda n: M.block(n, 18)), (65, [1, 0, 1, 1, 0, 1, 1], lambda n: np.arange(n)[::-1]),
                                   (50, [0, 1], lambda n: rng.permutation(n))):
        k = M.kept(n_coded, keep)
        perm = None if perm_of is None else perm_of(len(k))
        c = rng.integers(0, 2, (5, n_coded)).astype(np.uint8)
        tx = M.match(V.pack(c), n_coded, keep, perm)
        assert tx.shape == (5, -(-len(k) // 8))
        back = M.unmatch_hard(tx, n_coded, keep, perm)
        want = np.zeros((5, n_coded), np.float32)
        want[:, k] = 1.0 - 2.0 * c[:, k]
        assert np.array_equal(back, want) and not np.signbit(back[:, np.setdiff1d(np.arange(n_coded), k)]).any()
        llr = rng.standard_normal((5, len(k))).astype(np.float32)
        soft = M.unmatch(llr, n_coded, keep, perm, n_coded + 3)
        src = M.source_index(n_coded, keep, perm)
        assert soft.shape == (5, n_coded + 3) and np.array_equal(soft[:, src], llr) and np.count_nonzero(soft) == np.count_nonzero(llr)
        inv = M.inverse_index(n_coded, src)
        assert np.array_equal(np.flatnonzero(inv >= 0), k) and np.array_equal(src[inv[k]], k)


def test_source_index_is_increasing_for_the_identity():
    for n_coded, keep in ((1, None), (40, [1, 1, 1, 0]), (41, [0, 1]), (9, [1] + [0] * 11), (100, [1, 0, 1, 1, 0, 1, 1])):
        src = M.source_index(n_coded, keep)
        assert len(src) >= 1 and np.all(np.diff(src) > 0) and np.array_equal(src, M.kept(n_coded, keep))
    assert M.kept(9, [0, 1]).tolist() == [1, 3, 5, 7] and M.kept(5, [1, 0, 0, 0, 0, 0, 1]).tolist() == [0]


def test_block_interleaver():
    import gfdm_amd
    assert M.block(8, 3).tolist() == [0, 3, 6, 1, 4, 7, 2, 5]
    assert gfdm_amd.block_interleaver(8, 3).tolist() == [0, 3, 6, 1, 4, 7, 2, 5]
    for n in range(1, 41):
        for c in range(1, 10):
            p = gfdm_amd.block_interleaver(n, c)
            assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(n)), (n, c)
            assert np.array_equal(p, M.block(n, c))
    assert gfdm_amd.block_interleaver(7, 1).tolist() == list(range(7)) and gfdm_amd.block_interleaver(7, 7).tolist() == list(range(7))
    for bad in ((0, 3), (5, 0)):
        with pytest.raises(ValueError):
            gfdm_amd.block_interleaver(*bad)


def test_puncture_patterns():
    import gfdm_amd
    for rate, kept_share in (("1/2", (1, 1)), ("2/3", (3, 4)), ("3/4", (2, 3)), ("5/6", (3, 5))):
        p = gfdm_amd.puncture_pattern(rate)
        assert p.dtype == np.uint8 and p.tolist() == M.RATES[rate]
        assert int(p.sum()) * kept_share[1] == p.size * kept_share[0]
        num, den = (int(x) for x in rate.split("/"))
        assert num * int(p.sum()) == den * (p.size // 2)                  # p.size / 2 information bits give p.sum() transmitted bits
    with pytest.raises(ValueError):
        gfdm_amd.puncture_pattern("7/8")


# ---- the library, without a device ----

def _lib():
    import gfdm_amd
    return gfdm_amd.lib()


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


BAD_CREATE = [  # (n_coded, keep, period or None for len(keep), perm, n_perm or None for len(perm)), what
    ((0, [1], None, None, 0), "n_coded 0"),
    ((-4, [1], None, None, 0), "n_coded negative"),
    (((1 << 21) + 1, [1], None, None, 0), "n_coded above 2^21"),
    ((16, [1], 0, None, 0), "period 0"),
    ((16, [1] * 4097, None, None, 0), "period above 4096"),
    ((16, [0, 0, 0], None, None, 0), "a pattern that keeps nothing"),
    ((3, [0, 0, 0, 1], None, None, 0), "a pattern that keeps nothing within n_coded"),
    ((16, [1, 1, 1, 0], None, [0, 1, 2], None), "n_perm below n_tx"),
    ((8, [1, 1, 1, 0], None, [0, 1, 2, 3, 4, 5, 6], None), "n_perm above n_tx"),
    ((8, [1, 1, 1, 0], None, [0, 1, 2, 3, 4, 4], None), "a repeated entry"),
    ((8, [1, 1, 1, 0], None, [0, 1, 2, 3, 4, 6], None), "an entry of n_tx"),
    ((8, [1, 1, 1, 0], None, [0, 1, 2, 3, 4, -1], None), "a negative entry"),
]


def _args(n_coded, keep, period, perm, n_perm):
    keep = _u8(keep)
    perm = None if perm is None else _i32(perm)
    return (n_coded, keep.ctypes.data, keep.size if period is None else period, None if perm is None else perm.ctypes.data,
            (0 if perm is None else perm.size) if n_perm is None else n_perm), (keep, perm)


def test_check_table_and_tx_bits_of():
    import gfdm_amd
    L = _lib()
    EINVAL = gfdm_amd.capi.EINVAL
    ok = [((1, [1], None, None, 0), 1), ((924, M.RATES["3/4"], None, M.block(616, 18), None), 616), ((1 << 21, [1, 0], None, None, 0), 1 << 20),
          ((5, [0] * 4095 + [1], None, None, 0), 0), ((9, [0, 1], None, [3, 2, 1, 0], None), 4), ((7, [1, 0, 0, 0, 0, 0, 0, 0, 1], None, [0], None), 1)]
    for a, n_tx in ok:
        args, hold = _args(*a)                               # (hold: the arrays behind the pointers)
        if n_tx == 0:                                        # the only kept position lies behind the row
            assert L.gfdm_hip_rate_matcher_tx_bits_of(*args[:3]) == EINVAL
            continue
        assert L.gfdm_hip_rate_matcher_check(*args, 5) == gfdm_amd.capi.OK, a
        assert L.gfdm_hip_rate_matcher_tx_bits_of(*args[:3]) == n_tx == len(M.kept(a[0], a[1]))
        assert gfdm_amd.RateMatcher.tx_bits_of(a[0], a[1]) == n_tx
    for a, what in BAD_CREATE:
        args, hold = _args(*a)
        assert L.gfdm_hip_rate_matcher_check(*args, 1) == EINVAL, what
        assert L.gfdm_hip_last_error(), what
        if a[3] is None:                                     # what is wrong lies in the pattern: tx_bits_of refuses it too
            assert L.gfdm_hip_rate_matcher_tx_bits_of(*args[:3]) == EINVAL, what
    args, hold = _args(16, [1], None, None, 0)
    assert L.gfdm_hip_rate_matcher_check(args[0], None, 1, None, 0, 1) == EINVAL                       # a NULL pattern
    assert L.gfdm_hip_rate_matcher_check(*args, -1) == EINVAL                                          # n_rows < 0
    assert L.gfdm_hip_rate_matcher_check(1 << 21, *args[1:], 1 << 42) == EINVAL                        # 4 * 2^21 * 2^42 bytes
    assert L.gfdm_hip_rate_matcher_check(*args, 1 << 40) == gfdm_amd.capi.OK
    with pytest.raises(ValueError):
        gfdm_amd.RateMatcher.tx_bits_of(16, [0, 0])
    for getter in ("coded_bits", "tx_bits", "tx_bytes"):
        assert getattr(L, "gfdm_hip_rate_matcher_" + getter)(None) == EINVAL
    assert L.gfdm_hip_rate_matcher_source_index(None, None) == EINVAL


def test_create_refuses_its_arguments_before_it_looks_for_a_device():
    """Every refusal of the constructor that needs no device is EINVAL where no device exists as well: the checks and the composition
    of the tables run before the handle's context is opened (gfdm::create_handle, whose refused constructors tests/sanitize counts
    runtime calls for: none).  A valid constructor then answers ENODEV here, and works where a GPU is visible."""
    import gfdm_amd
    L = _lib()
    for a, what in BAD_CREATE:
        args, hold = _args(*a)
        h = ctypes.c_void_p(1)
        assert L.gfdm_hip_rate_matcher_create(ctypes.byref(h), *args, 0) == gfdm_amd.capi.EINVAL and not h.value, what
    args, hold = _args(16, [1], None, None, 0)
    assert L.gfdm_hip_rate_matcher_create(None, *args, 0) == gfdm_amd.capi.EINVAL                      # a NULL handle pointer
    for kw in (dict(n_coded=0), dict(n_coded=16, keep=[0]), dict(n_coded=16, keep=[1, 0], perm=[0, 1, 2]), dict(n_coded=4, perm=[0, 1, 2, 2]),
               dict(n_coded=4, perm=[0, 1, 2, 2 ** 31])):
        with pytest.raises(ValueError):
            gfdm_amd.RateMatcher(**kw)
    with pytest.raises(TypeError):
        gfdm_amd.RateMatcher(4, perm=[0.0, 1.0, 2.0, 3.0])
    if have_gpu():
        rm = gfdm_amd.RateMatcher(924, gfdm_amd.puncture_pattern("3/4"), gfdm_amd.block_interleaver(616, 18))
        assert (rm.coded_bits(), rm.tx_bits(), rm.tx_bytes()) == (924, 616, 77)
        assert np.array_equal(rm.source_index(), M.source_index(924, M.RATES["3/4"], M.block(616, 18)))
        return
    with pytest.raises(gfdm_amd.GfdmHipError) as e:
        gfdm_amd.RateMatcher(924, gfdm_amd.puncture_pattern("3/4"))
    assert e.value.status == gfdm_amd.capi.ENODEV
    assert gfdm_amd.RateMatcher.__init__.__defaults__ == (None, None, 0)


# ---- the two decoding cases ----

@pytest.mark.parametrize("rate", sorted(M.GAIN_CASES))
def test_coding_gain_under_puncturing(rate):
    """64 rows of 456 information bits, punctured, interleaved, BPSK in Gaussian noise: every row decodes to its payload"""
    sigma, n_tx, raw = M.GAIN_CASES[rate]
    payload, c, tx, llr, perm, _ = M.coding_gain_case(rate)
    assert tx.shape == (64, n_tx) and llr.dtype == np.float32
    wrong = int(((llr < 0) != (tx == 1)).sum())
    got, _ = V.decode(M.unmatch(llr, c.shape[1], M.RATES[rate], perm), M.CASE_N_INFO, M.CASE_GAIN)
    rows = int((got != payload).any(axis=1).sum())
    print("rate %s, sigma %g: %d of %d transmitted values with the wrong sign, %d of 64 rows wrong" % (rate, sigma, wrong, tx.size, rows))
    assert wrong == raw                                      # the inputs are the ones the issue's figures were taken with
    assert rows == 0 and np.array_equal(got, payload)


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_burst_erasure_needs_the_interleaver(rate):
    """48 consecutive transmitted values erased, noise-free, at every 7th start: with the 18-column block interleaver every row decodes
    right at every start; without it rows decode wrong (seen: every row at every start)"""
    payload, c, keep = M.burst_case(rate)
    k = M.kept(c.shape[1], keep)
    n_tx = len(k)
    starts = list(range(0, n_tx - M.BURST_LEN, 7))
    want = np.tile(payload, (len(starts), 1))
    wrong = {}
    for name, perm in (("block", M.block(n_tx, M.CASE_COLUMNS)), ("identity", None)):
        tx = c[:, M.source_index(c.shape[1], keep, perm)]
        got, _ = V.decode(M.unmatch(M.burst_llrs(tx, starts), c.shape[1], keep, perm), M.CASE_N_INFO, M.CASE_GAIN)
        wrong[name] = int((got != want).any(axis=1).sum())
    print("rate %s, %d starts: %d of %d rows wrong with the block interleaver, %d without" % (rate, len(starts), wrong["block"], len(want), wrong["identity"]))
    assert wrong["block"] == 0
    assert wrong["identity"] > 0
