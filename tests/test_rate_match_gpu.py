"""GPU tests of the rate matcher (contract in include/gfdm_hip.h, gfdm_hip_rate_matcher).  The yardstick is the numpy restatement of
tests/rate_match_ref.py, which tests/test_rate_match.py holds to facts that do not depend on it.  Everything is integer index arithmetic
and bit copies, so every comparison is exact: array_equal on uint8, and on a uint32 view of the floats; there is no tolerance anywhere.
Every output written through out= lies between canaries."""
import os
import re

import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import conv_code_ref as V
import gfdm_ref as R
import rate_match_ref as M
from conftest import ROOT, have_gpu

pytestmark = pytest.mark.gpu
CANARY = {np.uint8: 0xA5, np.int32: 0x5A5A5A5A, np.float32: 7.0}
GUARD = 32                                   # canary elements on either side


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


def _bits(a):
    """float32 -> its bit patterns"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _matcher(n_coded, keep=None, perm=None):
    import gfdm_amd
    return gfdm_amd.RateMatcher(n_coded, keep, perm)


class Window:
    """`shape` elements of `dtype` inside a larger device buffer, `shift` elements past a 16-byte boundary, canaries on either side"""

    def __init__(self, shape, dtype, shift=0, content=None):
        import torch
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.n = int(np.prod(self.shape))
        per = 16 // np.dtype(dtype).itemsize
        self.lo = GUARD // per * per + per + shift
        self.buf = torch.full((self.lo + self.n + GUARD,), CANARY[dtype], dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")
        self.view = self.buf[self.lo:self.lo + self.n].view(self.shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * np.dtype(dtype).itemsize) % 16
        self.fill = _h(self.buf[:1])[0]
        if content is not None:
            self.view.copy_(_t(np.ascontiguousarray(content, dtype)).view(self.shape))

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == self.fill) and np.all(b[self.lo + self.n:] == self.fill), "canaries overwritten"
        return b[self.lo:self.lo + self.n].reshape(self.shape)


SPECIALS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                     0x00400000, 0x3F800000, 0xBF800000], np.uint32)      # NaNs with distinct payloads (quiet, signalling), +-inf, -0.0, +0.0, denormals, +-1


def wild_floats(rng, shape):
    """float32 of random BIT patterns -- NaNs of every payload, denormals, both zeros among them -- with the SPECIALS sprinkled over them"""
    bits = rng.integers(0, 2 ** 32, shape, dtype=np.uint32)
    where = rng.random(shape) < 0.25
    bits[where] = rng.choice(SPECIALS, size=int(where.sum()))
    return bits.view(np.float32)


def check_calls(n_coded, keep, perm, n_rows, rng, extra=0, shifts=(0, 0, 0, 0), count=None, tag=""):
    """match, unmatch and unmatch_hard of one handle on the device against the restatement.  extra: every width and stride above its
    minimum by this much.  shifts: of (byte input, byte output, float input, float output) past a 16-byte boundary.  The spare bits and
    bytes of the coded rows are random, the floats behind n_tx are NaN; with a count the dead rows' inputs are 0xFF / NaN."""
    rm = _matcher(n_coded, keep, perm)
    src = M.source_index(n_coded, keep, perm)
    n_tx = len(src)
    assert (rm.coded_bits(), rm.tx_bits(), rm.tx_bytes()) == (n_coded, n_tx, -(-n_tx // 8)), tag
    assert np.array_equal(rm.source_index(), src), tag + ": src"
    live = n_rows if count is None else min(max(int(count), 0), n_rows)
    in_bytes, tx_bytes, in_stride, out_stride = -(-n_coded // 8) + extra, -(-n_tx // 8) + extra, n_tx + extra, n_coded + extra
    sb, so, sf, sg = shifts
    # match
    coded = rng.integers(0, 256, (n_rows, in_bytes), dtype=np.uint8)
    want = M.match(coded, n_coded, keep, perm, tx_bytes)
    want[live:] = 0
    coded[live:] = 0xFF
    out = Window((n_rows, tx_bytes), np.uint8, so)
    rm.match(Window(coded.shape, np.uint8, sb, coded).view, out_row_bytes=tx_bytes, count=count, out=out.view)
    assert np.array_equal(out.result(), want), tag + ": match"
    # unmatch
    llr = wild_floats(rng, (n_rows, in_stride))
    llr[:, n_tx:] = np.nan
    want = M.unmatch(llr, n_coded, keep, perm, out_stride)
    want[live:] = 0
    llr[live:] = np.nan
    out = Window((n_rows, out_stride), np.float32, sg)
    rm.unmatch(Window(llr.shape, np.float32, sf, llr).view, out_stride=out_stride, count=count, out=out.view)
    got = out.result()
    assert np.array_equal(_bits(got), _bits(want)), tag + ": unmatch"
    punctured = np.setdiff1d(np.arange(out_stride), src)
    assert not _bits(got)[:, punctured].any(), tag + ": punctured positions and padding must be +0.0"
    # unmatch_hard
    tx = rng.integers(0, 256, (n_rows, tx_bytes), dtype=np.uint8)
    want = M.unmatch_hard(tx, n_coded, keep, perm, out_stride)
    want[live:] = 0
    tx[live:] = 0xFF
    out = Window((n_rows, out_stride), np.float32, sg)
    rm.unmatch_hard(Window(tx.shape, np.uint8, sb, tx).view, out_stride=out_stride, count=count, out=out.view)
    assert np.array_equal(_bits(out.result()), _bits(want)), tag + ": unmatch_hard"
    return rm


def patterns(n_coded):
    """all ones, the four rates, the first bit dropped, a period that does not divide 8, a period above n_coded, one kept bit"""
    long_period = min(n_coded + 3, 4096)                     # above n_coded wherever the 4096 of the contract allow it
    above = (np.arange(long_period) % 3 != 1).astype(np.uint8)
    one = np.zeros(long_period, np.uint8)
    one[min(n_coded, long_period) // 2] = 1                  # exactly one bit of a row of up to 4093; one per 4096 of a longer one
    return [("ones", None), ("1/2", M.RATES["1/2"]), ("2/3", M.RATES["2/3"]), ("3/4", M.RATES["3/4"]), ("5/6", M.RATES["5/6"]), ("[0,1]", [0, 1]),
            ("period 7", [1, 0, 1, 1, 0, 1, 1]), ("period %d" % long_period, above), ("one bit", one)]


def permutations(n_tx):
    return [("identity", None), ("reversal", np.arange(n_tx)[::-1]), ("block 18", M.block(n_tx, 18)), ("block n_tx", M.block(n_tx, n_tx)),
            ("random", np.random.default_rng(11).permutation(n_tx))]


SHAPES = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 924, 1388, M.LDS_BITS, M.LDS_BITS + 1, M.LDS_BITS + 2]


@pytest.mark.parametrize("n_coded", SHAPES)
def test_every_shape(n_coded):
    """every pattern with every permutation: rows shorter than a byte, either side of a byte, of a 4-byte word and of a 16-byte vector,
    the two frame sizes, and either side of GFDM_HIP_RM_LDS_BITS, where the table moves from LDS to the cache"""
    import gfdm_amd
    header = open(os.path.join(ROOT, "include", "gfdm_hip.h")).read()
    assert int(re.search(r"#define GFDM_HIP_RM_LDS_BITS (\d+)", header).group(1)) == M.LDS_BITS      # the shapes straddle the header's threshold
    rng = np.random.default_rng(3000 + n_coded)
    i = 0
    for pname, keep in patterns(n_coded):
        n_tx = len(M.kept(n_coded, keep))
        if n_tx == 0:                                        # [0, 1] on a row of one bit
            with pytest.raises(ValueError):
                gfdm_amd.RateMatcher(n_coded, keep)
            continue
        assert gfdm_amd.RateMatcher.tx_bits_of(n_coded, keep) == n_tx
        for qname, perm in permutations(n_tx):
            i += 1
            check_calls(n_coded, keep, perm, 3, rng, shifts=(i % 16, (5 * i) % 16, i % 4, (3 * i) % 4), tag="n_coded %d, %s, %s" % (n_coded, pname, qname))
    assert i >= 40


def test_one_long_row():
    """2^17 + 6 coded bits: the table read through the cache, 513 tiles of floats"""
    n_coded = 2 ** 17 + 6
    rng = np.random.default_rng(78)
    n_tx = len(M.kept(n_coded, M.RATES["3/4"]))
    check_calls(n_coded, M.RATES["3/4"], M.block(n_tx, 18), 1, rng, shifts=(3, 9, 1, 2), tag="long row, block 18")
    check_calls(n_coded, M.RATES["3/4"], rng.permutation(n_tx), 1, rng, extra=1, tag="long row, random")


@pytest.mark.parametrize("n_rows, n_coded", [(1, 6), (3, 6), (4, 6), (5, 6), (7, 6), (5000, 6), (32768 + 7, 4)])
def test_rows_per_call(n_rows, n_coded):
    """less than one tile, many rows in one word / vector, and more tiles than the bounded grid has workgroups"""
    rng = np.random.default_rng(n_rows)
    check_calls(n_coded, [1, 1, 1, 0], np.arange(len(M.kept(n_coded, [1, 1, 1, 0])))[::-1], n_rows, rng, shifts=(1, 2, 3, 1), tag="%d rows" % n_rows)
    check_calls(n_coded, None, None, n_rows, rng, extra=1, tag="%d rows, all kept" % n_rows)


@pytest.mark.parametrize("extra", [0, 1, 12])
def test_widths_and_alignment(extra):
    """widths and strides above the minimum (odd ones move every other row off its alignment), and every buffer at every alignment of
    one element: bytes at all 16 positions of a 16-byte line, floats at all four"""
    n_coded, keep = 65, M.RATES["3/4"]
    perm = M.block(len(M.kept(n_coded, keep)), 18)
    rng = np.random.default_rng(200 + extra)
    for s in range(16):
        check_calls(n_coded, keep, perm, 6, rng, extra, shifts=(s, 15 - s, s % 4, (s // 4) % 4), tag="widths +%d, shift %d" % (extra, s))


def test_values_are_copied_bit_for_bit():
    """every special once in every row at a known place: the float that comes out is the float that went in, punctured positions and the
    padding are +0.0 whatever surrounds them"""
    n_coded, keep = 129, [1, 0, 1, 1, 0, 1, 1]
    src = M.source_index(n_coded, keep, M.block(len(M.kept(n_coded, keep)), 18))
    rm = _matcher(n_coded, keep, M.block(len(src), 18))
    llr = np.full((4, len(src) + 2), np.nan, np.float32)
    llr.view(np.uint32)[:, :len(SPECIALS)] = SPECIALS
    llr.view(np.uint32)[:, len(SPECIALS):len(src)] = 0xFFFFFFFF
    out = Window((4, n_coded + 5), np.float32, 1)
    rm.unmatch(_t(llr), out_stride=n_coded + 5, out=out.view)
    got = _bits(out.result())
    assert np.array_equal(got[:, src[:len(SPECIALS)]], np.tile(SPECIALS, (4, 1)))
    assert np.all(got[:, src[len(SPECIALS):]] == 0xFFFFFFFF)
    assert not got[:, np.setdiff1d(np.arange(n_coded + 5), src)].any()


@pytest.mark.parametrize("count", [0, 3, 9, 10, 15, -2])
def test_count(count):
    """rows from clamp(count, 0, n_rows) on are zeros, and their input -- 0xFF bytes and NaN -- is not read into the output; a device
    count tensor such as detect's is accepted"""
    import torch
    for cnt in (count, torch.tensor([count], dtype=torch.int64, device="cuda:0")):
        check_calls(122, M.RATES["2/3"], M.block(92, 18), 10, np.random.default_rng(31), extra=1, shifts=(5, 3, 1, 2), count=cnt, tag="count %d" % count)


def test_argument_errors_on_the_device():
    import ctypes
    import gfdm_amd
    rm = _matcher(20, M.RATES["3/4"])                        # n_tx 14: 3 coded bytes, 2 transmitted bytes
    assert (rm.tx_bits(), rm.tx_bytes()) == (14, 2)
    coded, llr, tx = _t(np.zeros((2, 3), np.uint8)), _t(np.zeros((2, 14), np.float32)), _t(np.zeros((2, 2), np.uint8))
    for call in (lambda: rm.match(_t(np.zeros((2, 2), np.uint8))), lambda: rm.match(coded, out_row_bytes=1),
                 lambda: rm.unmatch(_t(np.zeros((2, 13), np.float32))), lambda: rm.unmatch(llr, out_stride=19),
                 lambda: rm.unmatch_hard(_t(np.zeros((2, 1), np.uint8))), lambda: rm.unmatch_hard(tx, out_stride=19)):
        with pytest.raises(ValueError):
            call()
    # the same at the C-ABI, and what the wrapper cannot be made to pass: NULL buffers, a NULL handle, n_rows < 0, sizes beyond int64
    L = gfdm_amd.lib()
    EINVAL = gfdm_amd.capi.EINVAL
    out_b, out_f = _t(np.zeros((2, 2), np.uint8)), _t(np.zeros((2, 20), np.float32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h = rm._h
    big = 1 << 62
    for name, out, x, ok, bad in (("match", out_b, coded, (3, 2), ((2, 2), (3, 1), (big, 2), (3, big))),
                                  ("unmatch", out_f, llr, (14, 20), ((13, 20), (14, 19), (big, 20), (14, big))),
                                  ("unmatch_hard", out_f, tx, (2, 20), ((1, 20), (2, 19), (big, 20), (2, big)))):
        fn = getattr(L, "gfdm_hip_rate_matcher_%s_device" % name)
        for widths in bad:
            assert fn(h, p(out), p(x), None, *widths, 2, None) == EINVAL, (name, widths)
            assert L.gfdm_hip_last_error()
        assert fn(h, None, p(x), None, *ok, 2, None) == EINVAL and fn(h, p(out), None, None, *ok, 2, None) == EINVAL
        assert fn(None, p(out), p(x), None, *ok, 2, None) == EINVAL and fn(h, p(out), p(x), None, *ok, -1, None) == EINVAL
        assert fn(h, p(out), p(x), None, *ok, 0, None) == gfdm_amd.capi.OK and fn(h, None, None, None, *ok, 0, None) == gfdm_amd.capi.OK
    with pytest.raises(TypeError):
        rm.match(_t(np.zeros((2, 3), np.float32)))          # floats where packed bytes are expected
    with pytest.raises(TypeError):
        rm.unmatch(llr, out=np.zeros((2, 20), np.float32))  # a host result for a device input
    empty = rm.unmatch(_t(np.zeros((0, 14), np.float32)))
    assert tuple(empty.shape) == (0, 20)
    one = rm.unmatch_hard(tx[0])                             # a 1-D input is one row
    assert tuple(one.shape) == (20,) and np.array_equal(_h(one), M.unmatch_hard(np.zeros((1, 2), np.uint8), 20, M.RATES["3/4"])[0])


def test_host_flavour_equals_device_flavour_and_calls_repeat():
    rng = np.random.default_rng(41)
    for n_coded, keep, columns in ((924, M.RATES["3/4"], 18), (M.LDS_BITS + 5, M.RATES["5/6"], 18), (9, None, 2)):
        n_tx = len(M.kept(n_coded, keep))
        perm = M.block(n_tx, columns)
        rm = _matcher(n_coded, keep, perm)
        n_rows = 7
        coded = rng.integers(0, 256, (n_rows, -(-n_coded // 8) + 2), dtype=np.uint8)
        llr = wild_floats(rng, (n_rows, n_tx + 1))
        tx = rng.integers(0, 256, (n_rows, -(-n_tx // 8)), dtype=np.uint8)
        for count in (None, 4):
            live = n_rows if count is None else count
            for call, x, want in ((rm.match, coded, M.match(coded, n_coded, keep, perm)), (rm.unmatch, llr, M.unmatch(llr, n_coded, keep, perm)),
                                  (rm.unmatch_hard, tx, M.unmatch_hard(tx, n_coded, keep, perm))):
                want = want.copy()
                want[live:] = 0
                host = call(x, count=count)
                first, second = _h(call(_t(x), count=count)), _h(call(_t(x), count=count))
                assert isinstance(host, np.ndarray) and host.dtype == want.dtype
                view = (lambda a: a) if want.dtype == np.uint8 else _bits
                assert np.array_equal(view(host), view(want)) and np.array_equal(view(first), view(want)) and np.array_equal(view(second), view(want))
        assert np.array_equal(rm.match(coded[0]), M.match(coded[:1], n_coded, keep, perm)[0])          # one row, on the host
        into = np.full((n_rows, n_coded + 3), 7.0, np.float32)
        assert rm.unmatch(llr, out_stride=n_coded + 3, out=into) is into and np.array_equal(_bits(into), _bits(M.unmatch(llr, n_coded, keep, perm, n_coded + 3)))


def test_unmatch_hard_and_decode_is_decode_hard():
    """keep all ones, no permutation: decode(unmatch_hard(x), gain 1) is decode_hard(x), bytes and path_metric, on the noisy hard
    decisions of the coding-gain case of tests/conv_code_ref.py"""
    import gfdm_amd
    payload, llr, _ = V.coding_gain_case()
    x = V.pack((llr < 0).astype(np.uint8))
    n_rows, n_coded = x.shape[0], V.coded_bits(V.GAIN_N_INFO)
    cc = gfdm_amd.ConvolutionalCode()
    rm = _matcher(n_coded)
    pm_a, pm_b = Window(n_rows, np.int32), Window(n_rows, np.int32, 1)
    soft = rm.unmatch_hard(_t(x))
    assert np.array_equal(_h(soft), V.hard_values(x, V.GAIN_N_INFO).astype(np.float32))
    a = _h(cc.decode(soft, V.GAIN_N_INFO, 1.0, path_metric=pm_a.view))
    b = _h(cc.decode_hard(_t(x), V.GAIN_N_INFO, path_metric=pm_b.view))
    want, metric = V.decode_hard(x, V.GAIN_N_INFO)
    assert np.array_equal(a, b) and np.array_equal(pm_a.result(), pm_b.result())
    assert np.array_equal(a, want) and np.array_equal(pm_a.result(), metric)


@pytest.mark.parametrize("rate", sorted(M.GAIN_CASES))
def test_coding_gain_under_puncturing(rate):
    """the rows tests/test_rate_match.py decodes on the CPU: encode -> match on the device, the case's noise added on the host, unmatch ->
    decode on the device.  Every row decodes to its payload."""
    import gfdm_amd
    sigma, n_tx, _ = M.GAIN_CASES[rate]
    payload, c, tx, llr, perm, noise = M.coding_gain_case(rate)
    cc = gfdm_amd.ConvolutionalCode()
    rm = _matcher(c.shape[1], M.RATES[rate], perm)
    assert rm.tx_bits() == n_tx == gfdm_amd.RateMatcher.tx_bits_of(c.shape[1], gfdm_amd.puncture_pattern(rate))
    assert np.array_equal(perm, gfdm_amd.block_interleaver(n_tx, M.CASE_COLUMNS))
    sent = _h(rm.match(cc.encode(_t(payload), M.CASE_N_INFO)))
    assert np.array_equal(sent, V.pack(tx))
    received = M.gain_llr(V.unpack(sent, n_tx), noise, sigma)
    assert np.array_equal(_bits(received), _bits(llr))
    pm = Window(64, np.int32)
    depunctured = rm.unmatch(_t(received))
    assert np.array_equal(_bits(_h(depunctured)), _bits(M.unmatch(llr, c.shape[1], M.RATES[rate], perm)))
    got = _h(cc.decode(depunctured, M.CASE_N_INFO, M.CASE_GAIN, path_metric=pm.view))
    want, metric = V.decode(_h(depunctured), M.CASE_N_INFO, M.CASE_GAIN)
    assert np.array_equal(got, want) and np.array_equal(pm.result(), metric)
    assert np.array_equal(got, payload), "%d of 64 rows wrong" % int((got != payload).any(axis=1).sum())


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_burst_erasure_needs_the_interleaver(rate):
    """48 consecutive transmitted values erased at every 97th start: with the 18-column block interleaver every row decodes right at
    every start, without it rows decode wrong"""
    import gfdm_amd
    payload, c, keep = M.burst_case(rate)
    n_coded = c.shape[1]
    n_tx = len(M.kept(n_coded, keep))
    starts = list(range(0, n_tx - M.BURST_LEN, 97))
    want = np.tile(payload, (len(starts), 1))
    cc = gfdm_amd.ConvolutionalCode()
    wrong = {}
    for name, perm in (("block", M.block(n_tx, M.CASE_COLUMNS)), ("identity", None)):
        rm = _matcher(n_coded, keep, perm)
        sent = V.unpack(_h(rm.match(cc.encode(_t(payload), M.CASE_N_INFO))), n_tx)
        assert np.array_equal(sent, c[:, M.source_index(n_coded, keep, perm)])
        llr = M.burst_llrs(sent, starts)
        depunctured = rm.unmatch(_t(llr))
        assert np.array_equal(_bits(_h(depunctured)), _bits(M.unmatch(llr, n_coded, keep, perm)))
        got = _h(cc.decode(depunctured, M.CASE_N_INFO, M.CASE_GAIN))
        assert np.array_equal(got, V.decode(_h(depunctured), M.CASE_N_INFO, M.CASE_GAIN)[0])
        wrong[name] = int((got != want).any(axis=1).sum())
    print("rate %s, %d starts: %d of %d rows wrong with the block interleaver, %d without" % (rate, len(starts), wrong["block"], len(want), wrong["identity"]))
    assert wrong["block"] == 0
    assert wrong["identity"] > 0


def test_graph_of_soft_unmatch_and_decode_replays_with_a_changed_count():
    """SymbolMapper.soft -> unmatch -> decode captured once (three kernels, no allocation inside: every buffer is given); the replays
    follow the count and the symbols on the device"""
    import torch
    import gfdm_amd
    n_info, n_rows = 122, 9
    n_coded = V.coded_bits(n_info)
    keep = M.RATES["3/4"]
    n_tx = len(M.kept(n_coded, keep))                        # 171: odd, so the last symbol carries one spare bit
    perm = M.block(n_tx, 18)
    n_sym = -(-n_tx // 2)
    pts = R.qpsk_points().astype(np.complex64)
    m = gfdm_amd.SymbolMapper(pts)
    cc = gfdm_amd.ConvolutionalCode()
    rm = _matcher(n_coded, keep, perm)
    rng = np.random.default_rng(51)

    def symbols(seed):
        r = np.random.default_rng(seed)
        data = V.random_info(r, n_rows, n_info)
        t = V.unpack(M.match(V.encode(data, n_info), n_coded, keep, perm, m.row_bytes(n_sym)), 2 * n_sym)
        s = pts[2 * t[:, 0::2] + t[:, 1::2]]
        return (s + 0.3 * (r.standard_normal(s.shape) + 1j * r.standard_normal(s.shape))).astype(np.complex64)

    sym = _t(symbols(1))
    scale = _t(rng.uniform(2.0, 6.0, n_rows).astype(np.float32))
    count = torch.tensor([n_rows], dtype=torch.int64, device="cuda:0")
    llr = torch.zeros((n_rows, 2 * n_sym), dtype=torch.float32, device="cuda:0")
    mid = Window((n_rows, n_coded + 1), np.float32, 1)
    out, pm = Window((n_rows, V.info_bytes(n_info)), np.uint8, 3), Window(n_rows, np.int32, 1)

    def run():
        m.soft(sym, scale, count=count, out=llr)
        rm.unmatch(llr, out_stride=n_coded + 1, count=count, out=mid.view)
        cc.decode(mid.view, n_info, 4.0, count=count, out=out.view, path_metric=pm.view)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for seed, cnt in ((2, 9), (3, 4), (4, 0), (5, 7)):
        sym.copy_(_t(symbols(seed)))
        count.fill_(cnt)
        graph.replay()
        torch.cuda.synchronize()
        got_llr = _h(llr)
        assert not got_llr[cnt:].any()
        want_mid = M.unmatch(got_llr, n_coded, keep, perm, n_coded + 1)       # the restatement on the LLRs the device made
        want_mid[cnt:] = 0
        assert np.array_equal(_bits(mid.result()), _bits(want_mid)), "replay with count %d: unmatch" % cnt
        want, metric = V.decode(want_mid, n_info, 4.0)
        want[cnt:], metric[cnt:] = 0, 0
        assert np.array_equal(out.result(), want) and np.array_equal(pm.result(), metric), "replay with count %d" % cnt


NOISE_FACTOR = 4.0                           # as in tests/test_conv_code_gpu.py: the end-to-end loop's noise, over LOOP_NOISE_VOLTAGE


def test_end_to_end_on_the_device():
    """The chain of tests/test_conv_code_gpu.py's end-to-end test at rate 3/4 with an 18-column block interleaver: information bytes ->
    encode -> match -> map -> transmit -> place -> ChannelModel.apply (noise on) -> detect -> demodulate_bursts -> LinkMeter.measure ->
    soft -> unmatch -> decode, and SymbolMapper.decode -> unmatch_hard -> decode(gain 1), on the same loop fixtures and noise.  688
    information bits a burst instead of 456: 1388 coded bits, 926 transmitted, in the 936 of a frame.  Asserted: the device's floats and
    bytes are the restatement's on the downloaded LLRs / bytes, spare rows zero, and decoding leaves no more information-bit errors than
    the hard decisions had transmitted-bit errors.  The error counts themselves are printed, not asserted.  Seen on an MI355X: 107 of
    6482 transmitted bits wrong in the hard decisions, 58 of 4816 information bits wrong after unmatch + decode, 154 after unmatch_hard +
    decode (profiles/r17/rate_matcher_kernel_durations.txt)."""
    import gfdm_amd
    c = B.loop_case()
    M_, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym, n_info = A * M_, 688
    pts = R.qpsk_points().astype(np.complex64)
    m = gfdm_amd.SymbolMapper(pts)
    cc = gfdm_amd.ConvolutionalCode()
    n_coded = cc.coded_bits(n_info)
    keep = gfdm_amd.puncture_pattern("3/4")
    n_tx = gfdm_amd.RateMatcher.tx_bits_of(n_coded, keep)
    assert (n_coded, n_tx) == (1388, 926) and n_tx <= 2 * n_sym
    perm = gfdm_amd.block_interleaver(n_tx, 18)
    rm = gfdm_amd.RateMatcher(n_coded, keep, perm)
    rng = np.random.default_rng(60)
    info = V.clean(V.random_info(rng, nb, n_info), n_info)
    coded = cc.encode(_t(info), n_info)
    sent = rm.match(coded, out_row_bytes=m.row_bytes(n_sym))                             # as wide as map's rows: no kernel in between
    assert np.array_equal(_h(sent), M.match(V.encode(info, n_info), n_coded, keep, perm, m.row_bytes(n_sym)))
    sym = m.map(sent, n_sym)
    tx = gfdm_amd.Transmitter(M_, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(frames, _t(c["starts"]), c["out_len"])[0]
    ch = gfdm_amd.ChannelModel(NOISE_FACTOR * C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    ds = ch.apply(placed)
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb, "the loop's bursts were not all found at this noise: the rows below would not line up with the payload"
    est = gfdm_amd.ChannelEstimator(M_, K, A, True, 1, c["preamble"])
    rx = gfdm_amd.AdvancedReceiver(M_, K, L, c["taps"], c["smap"], 2, pts)
    rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
    rx.set_channel_estimator(est)
    demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
    meter = gfdm_amd.LinkMeter(pts)
    noise = meter.measure(demod, count=r["count"])                                       # decision-directed: err_power / n_sym estimates the noise
    scale = (n_sym / noise["err_power"].clamp_min(1e-12)).float()
    llr = m.soft(demod, scale, count=r["count"])
    depunctured = rm.unmatch(llr, count=r["count"])
    want_mid = M.unmatch(_h(llr), n_coded, keep, perm)
    want_mid[nb:] = 0
    assert np.array_equal(_bits(_h(depunctured)), _bits(want_mid))
    pm = Window(nb + 3, np.int32)
    got = _h(cc.decode(depunctured, n_info, 4.0, count=r["count"], path_metric=pm.view))
    want, metric = V.decode(want_mid, n_info, 4.0)
    want[nb:], metric[nb:] = 0, 0
    assert np.array_equal(got, want) and np.array_equal(pm.result(), metric)
    hard = m.decode(demod, count=r["count"])
    hard_mid = rm.unmatch_hard(hard, count=r["count"])
    want_mid = M.unmatch_hard(_h(hard), n_coded, keep, perm)
    want_mid[nb:] = 0
    assert np.array_equal(_bits(_h(hard_mid)), _bits(want_mid))
    got_hard = _h(cc.decode(hard_mid, n_info, 1.0, count=r["count"]))
    want_hard = V.decode(want_mid, n_info, 1.0)[0]
    want_hard[nb:] = 0
    assert np.array_equal(got_hard, want_hard)
    uncoded = int((V.unpack(_h(hard)[:nb], n_tx) != V.unpack(_h(sent), n_tx)).sum())
    after_soft = int(np.unpackbits(got[:nb] ^ info).sum())
    after_hard = int(np.unpackbits(got_hard[:nb] ^ info).sum())
    print("end to end at rate 3/4, noise x%g: %d of %d transmitted bits wrong in the hard decisions; information-bit errors of %d: %d after unmatch + decode, "
          "%d after unmatch_hard + decode" % (NOISE_FACTOR, uncoded, nb * n_tx, nb * n_info, after_soft, after_hard))
    assert after_soft <= uncoded
