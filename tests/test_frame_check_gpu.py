"""GPU tests of the frame check (contract in include/gfdm_hip.h, gfdm_hip_frame_check).  The yardstick is the numpy restatement of
tests/frame_check_ref.py, which tests/test_frame_check.py holds to zlib and to facts that do not depend on it.  Everything is integer
arithmetic, so every comparison is exact: array_equal, no tolerance anywhere.  Every output written through out= lies between
canaries."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import conv_code_ref as V
import frame_check_ref as F
import gfdm_ref as R
from conftest import have_gpu

pytestmark = pytest.mark.gpu
CANARY = {np.uint8: 0xA5, np.int64: 0x5A5A5A5A5A5A5A5A}
GUARD = 32                                   # canary elements on either side
DEFAULT, OFF, WIDE = (0x11, 0x7F, 7), (0, 0, 0), (0x80200003, 0xDEADBEEF, 32)
LFSRS = (DEFAULT, OFF, WIDE)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def _h(t):
    return t.cpu().numpy()


def _check(n_payload, lfsr=DEFAULT):
    import gfdm_amd
    return gfdm_amd.FrameCheck(n_payload, *lfsr)


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
        if content is not None:
            self.view.copy_(_t(np.ascontiguousarray(content, dtype)).view(self.shape))

    def result(self):
        b = _h(self.buf)
        assert np.all(b[:self.lo] == b.dtype.type(CANARY[b.dtype.type])) and np.all(b[self.lo + self.n:] == b.dtype.type(CANARY[b.dtype.type])), "canaries overwritten"
        return b[self.lo:self.lo + self.n].reshape(self.shape)


def corrupted(frames, n_payload, rows, rng):
    """one bit flipped in each of `rows`, in turn in the payload, in the CRC and in the frame's last byte"""
    frames = frames.copy()
    for k, r in enumerate(rows):
        at = (int(rng.integers(0, n_payload)), n_payload + int(rng.integers(0, 4)), n_payload + 3)[k % 3]
        frames[r, at] ^= 1 << int(rng.integers(0, 8))
    return frames


def chosen(n_rows):
    """the first row, the last, every 7th"""
    return sorted(set([0, n_rows - 1] + list(range(0, n_rows, 7))))


def check_calls(n_payload, lfsr, n_rows, rng, extra=0, shifts=(0, 0), count=None, bad="chosen", tag=""):
    """attach and verify of one handle on the device against the restatement.  extra: every width above its minimum by this much.
    shifts: of (input, output) past a 16-byte boundary.  The bytes behind the payload and behind the frame are random; with a count the
    dead rows' input is 0xFF.  bad: the rows verify sees with one bit flipped -- "chosen", "none" or "all"."""
    fc = _check(n_payload, lfsr)
    nf = n_payload + 4
    assert (fc.payload_bytes, fc.frame_bytes, fc.frame_bits) == (n_payload, nf, 8 * nf), tag
    assert np.array_equal(fc.whitening, F.whitening(nf, *lfsr)), tag + ": whitening"
    live = n_rows if count is None else min(max(int(count), 0), n_rows)
    si, so = shifts
    # attach
    x = rng.integers(0, 256, (n_rows, n_payload + extra), dtype=np.uint8)
    frames = F.attach(x, n_payload, *lfsr, out_row_bytes=nf + extra)
    want = frames.copy()
    want[live:] = 0
    x[live:] = 0xFF
    out = Window((n_rows, nf + extra), np.uint8, so)
    fc.attach(Window(x.shape, np.uint8, si, x).view, count=count, out=out.view, out_row_bytes=nf + extra)
    assert np.array_equal(out.result(), want), tag + ": attach"
    # verify
    rows = {"chosen": chosen(n_rows), "none": [], "all": list(range(n_rows))}[bad]
    frames[:, nf:] = rng.integers(0, 256, (n_rows, extra), dtype=np.uint8)
    frames = corrupted(frames, n_payload, rows, rng)
    payload, ok, good_row, n_good = F.limit(*F.verify(frames, n_payload, *lfsr, out_row_bytes=n_payload + extra)[:2], count)
    untouched = np.ones(n_rows, np.uint8)
    untouched[rows] = 0
    untouched[live:] = 0
    assert np.array_equal(ok, untouched), tag + ": the restatement itself"
    frames[live:] = 0xFF
    o_p, o_k = Window((n_rows, n_payload + extra), np.uint8, so), Window(n_rows, np.uint8, (so + 5) % 16)
    o_g, o_n = Window(n_rows, np.int64, so % 2), Window(1, np.int64, (so + 1) % 2)
    fc.verify(Window(frames.shape, np.uint8, si, frames).view, count=count, good_rows=True, out_row_bytes=n_payload + extra,
              out={"payload": o_p.view, "ok": o_k.view, "good_row": o_g.view, "n_good": o_n.view})
    assert np.array_equal(o_k.result(), untouched), tag + ": ok"
    assert np.array_equal(o_p.result(), payload), tag + ": payload"
    assert np.array_equal(o_g.result(), good_row) and int(o_n.result()[0]) == n_good == int(untouched.sum()), tag + ": good_row"
    return fc


SIZES = [1, 2, 11, 12, 13, 27, 28, 29, 57, 60, 61, 124, 1019, 1020, 1021, 1024, 2044, 2045]


@pytest.mark.parametrize("n_payload", SIZES)
def test_every_payload_size(n_payload):
    """frame_bytes on every side of 16, 32, 64, 1024 (64 lanes a row, then the first second step) and 2048, with every whitening"""
    rng = np.random.default_rng(1000 + n_payload)
    for i, lfsr in enumerate(LFSRS):
        check_calls(n_payload, lfsr, 5, rng, shifts=((3 * i + n_payload) % 16, (5 * i + 1) % 16), tag="n_payload %d, lfsr %d" % (n_payload, i))


def test_one_long_row():
    """2^17 - 4 payload bytes: 128 steps of 64 chunks"""
    rng = np.random.default_rng(77)
    check_calls(2 ** 17 - 4, DEFAULT, 1, rng, shifts=(3, 9), bad="none", tag="long row")
    check_calls(2 ** 17 - 4, DEFAULT, 1, rng, extra=1, bad="all", tag="long row, corrupted")


GROUPS = [3, 20, 57, 100, 200, 400, 900]     # n_payload for 1, 2, 4, 8, 16, 32 and 64 lanes a row


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 7, 63, 64, 65])
def test_rows_per_call(n_rows):
    """either side of the 64 / G rows of a wavefront and of the 256 / G of a workgroup's pass, for every group size G"""
    rng = np.random.default_rng(n_rows)
    for i, n_payload in enumerate(GROUPS):
        check_calls(n_payload, LFSRS[i % 3], n_rows, rng, extra=i % 2, shifts=(i, 2 * i + 1), tag="%d rows of %d" % (n_rows, n_payload))


@pytest.mark.parametrize("n_rows", [5000, 32768 + 7, 65536 + 5])
def test_many_rows(n_rows):
    """many passes of a workgroup, a ragged last row of the scan's tile, and more flags than one tile (65 536)"""
    rng = np.random.default_rng(n_rows)
    check_calls(3, DEFAULT, n_rows, rng, shifts=(1, 2), tag="%d rows" % n_rows)
    check_calls(3, WIDE, n_rows, rng, extra=1, shifts=(7, 0), bad="none", tag="%d rows, all good" % n_rows)


def test_more_row_groups_than_workgroups():
    """64 lanes a row leave four rows to a workgroup's pass: 4 * 2048 + 5 rows are more passes than the bounded grid has workgroups, so
    workgroups walk on to a second pass"""
    check_calls(1021, DEFAULT, 4 * 2048 + 5, np.random.default_rng(8197), shifts=(3, 5), tag="8197 rows of 1021")


def test_more_rows_than_the_scan_has_workgroups():
    """2^20 + 4096 + 5 rows of one payload byte: the scan behind verify has 256 workgroups of 4096 rows at most, so here a workgroup
    owns 8192 rows and walks two tiles (the last one 4096 + 5 rows); every seventh row and the last carry a flipped bit"""
    n_rows = 2 ** 20 + 4096 + 5
    rng = np.random.default_rng(20)
    fc = _check(1)
    x = rng.integers(0, 256, (n_rows, 1), dtype=np.uint8)
    frames = F.attach(x, 1)
    assert np.array_equal(_h(fc.attach(_t(x))), frames)
    frames[::7, 2] ^= 0x40
    frames[-1, 4] ^= 0x01
    payload, ok, good_row, n_good = F.verify(frames, 1)
    assert n_good == n_rows - len(range(0, n_rows, 7)) - 1
    o_g, o_n = Window(n_rows, np.int64, 1), Window(1, np.int64)
    got = fc.verify(_t(frames), good_rows=True, out={"good_row": o_g.view, "n_good": o_n.view})
    assert np.array_equal(_h(got[0]), payload) and np.array_equal(_h(got[1]), ok)
    assert np.array_equal(o_g.result(), good_row) and int(o_n.result()[0]) == n_good


@pytest.mark.parametrize("extra", [0, 1, 12])
def test_widths_and_alignment(extra):
    """widths above the minimum (odd ones move every other row off its alignment), input and output at every byte alignment"""
    rng = np.random.default_rng(200 + extra)
    for s in range(16):
        check_calls(57, DEFAULT, 6, rng, extra, shifts=(s, 15 - s), tag="57 bytes, widths +%d, shift %d" % (extra, s))
        check_calls(1021, WIDE, 3, rng, extra, shifts=(15 - s, s), tag="1021 bytes, widths +%d, shift %d" % (extra, s))


@pytest.mark.parametrize("bad", ["none", "all"])
def test_all_rows_good_and_no_row_good(bad):
    rng = np.random.default_rng(300)
    for n_payload, n_rows in ((57, 70), (12, 300), (1024, 9)):
        check_calls(n_payload, DEFAULT, n_rows, rng, shifts=(1, 3), bad=bad, tag="%d rows of %d, bad: %s" % (n_rows, n_payload, bad))


def test_optional_outputs():
    """payload = NULL: check only; good_row = NULL: one kernel; neither touches what it was not given"""
    rng = np.random.default_rng(400)
    n, n_rows = 57, 20
    fc = _check(n)
    frames = corrupted(F.attach(rng.integers(0, 256, (n_rows, n), dtype=np.uint8), n), n, chosen(n_rows), rng)
    payload, ok, good_row, n_good = F.verify(frames, n)
    o_k, o_g, o_n = Window(n_rows, np.uint8, 3), Window(n_rows, np.int64, 1), Window(1, np.int64)
    res = fc.verify(_t(frames), good_rows=True, payload=False, out={"ok": o_k.view, "good_row": o_g.view, "n_good": o_n.view})
    assert res[0] is None and np.array_equal(o_k.result(), ok) and np.array_equal(o_g.result(), good_row) and int(o_n.result()[0]) == n_good
    res = fc.verify(_t(frames), payload=False)
    assert len(res) == 2 and res[0] is None and np.array_equal(_h(res[1]), ok)
    o_p, o_k = Window((n_rows, n), np.uint8, 7), Window(n_rows, np.uint8, 1)
    res = fc.verify(_t(frames), out={"payload": o_p.view, "ok": o_k.view})
    assert len(res) == 2 and np.array_equal(o_p.result(), payload) and np.array_equal(o_k.result(), ok)
    with pytest.raises(ValueError):
        fc.verify(_t(frames), out={"good_row": o_g.view})
    with pytest.raises(ValueError):
        fc.verify(_t(frames), payload=False, out={"payload": o_p.view})


@pytest.mark.parametrize("count", [0, 3, 9, 10, 15, -2])
def test_count(count):
    """rows from clamp(count, 0, n_rows) on are zeros, not good, and their input -- 0xFF bytes -- is not read into the output; a device
    count tensor such as detect's is accepted"""
    import torch
    for cnt in (count, torch.tensor([count], dtype=torch.int64, device="cuda:0")):
        for n_payload in (57, 1021):
            check_calls(n_payload, DEFAULT, 10, np.random.default_rng(31), extra=1, shifts=(5, 3), count=cnt, tag="count %d" % count)


def test_argument_errors_on_the_device():
    import ctypes
    import gfdm_amd
    fc = _check(57)
    x, frames = _t(np.zeros((2, 57), np.uint8)), _t(np.zeros((2, 61), np.uint8))
    for call in (lambda: fc.attach(_t(np.zeros((2, 56), np.uint8))), lambda: fc.attach(x, out_row_bytes=60),
                 lambda: fc.verify(_t(np.zeros((2, 60), np.uint8))), lambda: fc.verify(frames, out_row_bytes=56)):
        with pytest.raises(ValueError):
            call()
    # the same at the C-ABI, and what the wrapper cannot be made to pass: NULL buffers, a NULL handle, n_rows < 0, sizes beyond int64
    L = gfdm_amd.lib()
    OK, EINVAL = gfdm_amd.capi.OK, gfdm_amd.capi.EINVAL
    o_f, o_p, o_k = _t(np.zeros((2, 61), np.uint8)), _t(np.zeros((2, 57), np.uint8)), _t(np.zeros(2, np.uint8))
    o_g, o_n = _t(np.zeros(2, np.int64)), _t(np.zeros(1, np.int64))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    h, big = fc._h, 1 << 62
    attach, verify = L.gfdm_hip_frame_check_attach_device, L.gfdm_hip_frame_check_verify_device
    for widths in ((56, 61), (57, 60), (big, 61), (57, big)):
        assert attach(h, p(o_f), p(x), None, *widths, 2, None) == EINVAL, widths
        assert L.gfdm_hip_last_error()
    assert attach(h, None, p(x), None, 57, 61, 2, None) == EINVAL and attach(h, p(o_f), None, None, 57, 61, 2, None) == EINVAL
    assert attach(None, p(o_f), p(x), None, 57, 61, 2, None) == EINVAL and attach(h, p(o_f), p(x), None, 57, 61, -1, None) == EINVAL
    assert attach(h, p(o_f), p(x), None, 57, 61, 0, None) == OK and attach(h, None, None, None, 57, 61, 0, None) == OK
    assert attach(h, p(o_f), p(x), ctypes.c_void_p(o_n.data_ptr() + 4), 57, 61, 2, None) == EINVAL              # a count off its 8 bytes
    for widths in ((60, 57), (61, 56), (big, 57), (61, big)):
        assert verify(h, p(o_p), p(o_k), p(o_g), p(o_n), p(frames), None, *widths, 2, None) == EINVAL, widths
    assert verify(h, None, p(o_k), None, None, p(frames), None, 61, -5, 2, None) == OK                           # no payload: its width is not looked at
    assert verify(h, p(o_p), None, p(o_g), p(o_n), p(frames), None, 61, 57, 2, None) == EINVAL                   # ok is not optional
    assert verify(h, p(o_p), p(o_k), p(o_g), p(o_n), None, None, 61, 57, 2, None) == EINVAL
    assert verify(h, p(o_p), p(o_k), p(o_g), None, p(frames), None, 61, 57, 2, None) == EINVAL                   # exactly one of good_row / n_good
    assert verify(h, p(o_p), p(o_k), None, p(o_n), p(frames), None, 61, 57, 2, None) == EINVAL
    assert verify(h, p(o_p), p(o_k), ctypes.c_void_p(o_g.data_ptr() + 4), p(o_n), p(frames), None, 61, 57, 1, None) == EINVAL
    assert verify(None, p(o_p), p(o_k), p(o_g), p(o_n), p(frames), None, 61, 57, 2, None) == EINVAL
    assert verify(h, p(o_p), p(o_k), p(o_g), p(o_n), p(frames), None, 61, 57, -1, None) == EINVAL
    assert verify(h, None, None, None, None, None, None, 61, 57, 0, None) == OK
    with pytest.raises(TypeError):
        fc.attach(_t(np.zeros((2, 57), np.float32)))        # floats where packed bytes are expected
    with pytest.raises(TypeError):
        fc.attach(x, out=np.zeros((2, 61), np.uint8))       # a host result for a device input
    empty = fc.verify(_t(np.zeros((0, 61), np.uint8)), good_rows=True)
    assert tuple(empty[0].shape) == (0, 57) and tuple(empty[1].shape) == (0,) and int(_h(empty[3])[0]) == 0
    one = fc.attach(x[0])                                    # a 1-D input is one row
    assert tuple(one.shape) == (61,) and np.array_equal(_h(one), F.attach(np.zeros((1, 57), np.uint8), 57)[0])
    back = fc.verify(one)
    assert tuple(back[0].shape) == (57,) and not _h(back[0]).any() and _h(back[1]).tolist() == [1]


def test_host_flavour_equals_device_flavour_and_calls_repeat():
    rng = np.random.default_rng(41)
    for n, lfsr in ((57, DEFAULT), (1021, WIDE), (3, OFF)):
        fc = _check(n, lfsr)
        n_rows = 7
        x = rng.integers(0, 256, (n_rows, n + 2), dtype=np.uint8)
        frames = corrupted(F.attach(x, n, *lfsr, out_row_bytes=n + 5), n, [1, 5], rng)
        for count in (None, 4):
            live = n_rows if count is None else count
            want = F.attach(x, n, *lfsr)
            want[live:] = 0
            host = fc.attach(x, count=count)
            first, second = _h(fc.attach(_t(x), count=count)), _h(fc.attach(_t(x), count=count))
            assert isinstance(host, np.ndarray) and np.array_equal(host, want) and np.array_equal(first, want) and np.array_equal(second, want)
            want = F.limit(*F.verify(frames, n, *lfsr)[:2], count)
            host = fc.verify(frames, count=count, good_rows=True)
            assert all(isinstance(a, np.ndarray) for a in host)
            for got in (host, fc.verify(_t(frames), count=count, good_rows=True), fc.verify(_t(frames), count=count, good_rows=True)):
                assert all(np.array_equal((g if isinstance(g, np.ndarray) else _h(g)).ravel(), np.asarray(w).ravel()) for g, w in zip(got, want))
            assert np.array_equal(fc.verify(frames, count=count, payload=False)[1], want[1])
        assert np.array_equal(fc.attach(x[0]), F.attach(x[:1], n, *lfsr)[0])                            # one row, on the host
        into = np.full((n_rows, n + 9), 7, np.uint8)
        assert fc.attach(x, out=into, out_row_bytes=n + 9) is into and np.array_equal(into, F.attach(x, n, *lfsr, out_row_bytes=n + 9))


def test_graph_of_decode_and_verify_replays_with_a_changed_count():
    """ConvolutionalCode.decode -> verify with good_row captured once (three kernels, no allocation inside: every buffer is given); the
    replays follow the count and the LLRs on the device, and equal the eager calls and the restatement"""
    import torch
    import gfdm_amd
    n, n_rows = 11, 9
    fc = _check(n)
    n_info = fc.frame_bits
    cc = gfdm_amd.ConvolutionalCode()
    n_coded = V.coded_bits(n_info)

    def llrs(seed, lost):
        r = np.random.default_rng(seed)
        frames = F.attach(r.integers(0, 256, (n_rows, n), dtype=np.uint8), n)
        v = (4.0 * V.hard_values(V.encode(frames, n_info), n_info) + r.standard_normal((n_rows, n_coded))).astype(np.float32)
        v[lost] = r.standard_normal((len(lost), n_coded)).astype(np.float32)               # rows of noise alone: they decode to something else
        return v

    llr = _t(llrs(1, []))
    count = torch.tensor([n_rows], dtype=torch.int64, device="cuda:0")
    dec = Window((n_rows, fc.frame_bytes), np.uint8, 3)
    o_p, o_k = Window((n_rows, n + 1), np.uint8, 5), Window(n_rows, np.uint8, 1)
    o_g, o_n = Window(n_rows, np.int64, 1), Window(1, np.int64)
    out = {"payload": o_p.view, "ok": o_k.view, "good_row": o_g.view, "n_good": o_n.view}

    def run():
        cc.decode(llr, n_info, 4.0, count=count, out=dec.view)
        fc.verify(dec.view, count=count, good_rows=True, out_row_bytes=n + 1, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for seed, cnt, lost in ((2, 9, [0, 4]), (3, 4, [3]), (4, 0, []), (5, 7, [6, 8]), (6, 12, [])):
        v = llrs(seed, lost)
        llr.copy_(_t(v))
        count.fill_(cnt)
        graph.replay()
        torch.cuda.synchronize()
        got = (o_p.result(), o_k.result(), o_g.result(), o_n.result())
        live = min(cnt, n_rows)
        decoded = V.decode(v, n_info, 4.0)[0]
        decoded[live:] = 0
        assert np.array_equal(dec.result(), decoded), "replay with count %d: decode" % cnt
        want = F.limit(*F.verify(decoded, n, out_row_bytes=n + 1)[:2], cnt)
        assert [r for r in range(live) if not want[1][r]] == [r for r in lost if r < live], "the rows of noise, and they alone, fail the check"
        eager = fc.verify(cc.decode(llr, n_info, 4.0, count=cnt), count=cnt, good_rows=True, out_row_bytes=n + 1)
        for g, e, w in zip(got, eager, want):
            assert np.array_equal(g.ravel(), np.asarray(w).ravel()) and np.array_equal(g.ravel(), _h(e).ravel()), "replay with count %d" % cnt


NOISE_FACTOR = 4.0                           # as in tests/test_rate_match_gpu.py: the end-to-end loop's noise, over LOOP_NOISE_VOLTAGE


def test_end_to_end_on_the_device():
    """The chain of tests/test_rate_match_gpu.py's end-to-end test (rate 3/4, 18-column block interleaver, the same loop fixtures and
    noise) with attach in front of encode and verify behind decode: 82 payload bytes a burst make the 688 information bits of that
    test.  Asserted: for every burst ok[r] == (payload[r] == sent payload), at least one row is good, good_row / n_good list the good
    rows, and the spare rows behind the count are dropped.  Whether the noise leaves a bad row is not known beforehand, so a second
    part flips one bit of chosen decoded rows on the device before verify: those rows and only those are dropped.  A third part runs
    verify over every row without the count: the spare rows, erasures that decode to zeros as a false alarm on silence would, fail
    the check too.  The counts are printed, not asserted."""
    import torch
    import gfdm_amd
    c = B.loop_case()
    M_, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym, n = A * M_, 82
    fc = _check(n)
    n_info = fc.frame_bits
    pts = R.qpsk_points().astype(np.complex64)
    m = gfdm_amd.SymbolMapper(pts)
    cc = gfdm_amd.ConvolutionalCode()
    n_coded = cc.coded_bits(n_info)
    keep = gfdm_amd.puncture_pattern("3/4")
    n_tx = gfdm_amd.RateMatcher.tx_bits_of(n_coded, keep)
    assert (n_info, n_coded, n_tx) == (688, 1388, 926) and n_tx <= 2 * n_sym
    rm = gfdm_amd.RateMatcher(n_coded, keep, gfdm_amd.block_interleaver(n_tx, 18))
    rng = np.random.default_rng(60)
    payload = rng.integers(0, 256, (nb, n), dtype=np.uint8)
    payload[0] = 0                                                                       # idle fill: whitened, it is sent as the sequence
    frames = fc.attach(_t(payload))
    assert np.array_equal(_h(frames), F.attach(payload, n))
    sent = rm.match(cc.encode(frames, n_info), out_row_bytes=m.row_bytes(n_sym))
    sym = m.map(sent, n_sym)
    tx = gfdm_amd.Transmitter(M_, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(tx.transmit(sym), _t(c["starts"]), c["out_len"])[0]
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
    noise = gfdm_amd.LinkMeter(pts).measure(demod, count=r["count"])
    scale = (n_sym / noise["err_power"].clamp_min(1e-12)).float()
    decoded = cc.decode(rm.unmatch(m.soft(demod, scale, count=r["count"]), count=r["count"]), n_info, 4.0, count=r["count"])
    n_rows = nb + 3
    assert tuple(decoded.shape) == (n_rows, fc.frame_bytes)
    got, ok, good_row, n_good = (_h(a) for a in fc.verify(decoded, count=r["count"], good_rows=True))
    want = F.limit(*F.verify(_h(decoded), n)[:2], nb)
    for g, w in zip((got, ok, good_row, n_good), want):
        assert np.array_equal(g.ravel(), np.asarray(w).ravel())
    right = (got[:nb] == payload).all(axis=1)
    assert np.array_equal(ok[:nb] != 0, right), "the check's verdict is not the comparison with the payload that was sent"
    assert not ok[nb:].any() and right.any()
    good = int(n_good[0])
    assert good == int(right.sum()) and np.array_equal(good_row[:good], np.flatnonzero(right)) and np.all(good_row[good:] == -1)
    # one bit flipped in chosen rows of the decoder's output, on the device
    rows = chosen(nb)
    flipped = decoded.clone()
    at = torch.tensor([(17 * k) % fc.frame_bytes for k in range(len(rows))], device="cuda:0")
    flipped[torch.tensor(rows, device="cuda:0"), at] ^= 0x10
    ok2 = _h(fc.verify(flipped, count=r["count"], payload=False)[1])
    hit = np.zeros(n_rows, bool)
    hit[rows] = True
    assert np.array_equal(ok2 != 0, (ok != 0) & ~hit), "the rows with a flipped bit, and only those, are dropped"
    # every row, the spare ones included
    ok3 = _h(fc.verify(decoded, payload=False)[1])
    assert np.array_equal(ok3[:nb], ok[:nb]) and not ok3[nb:].any()
    print("end to end at rate 3/4, noise x%g, %d bursts of %d payload bytes: %d rows good, %d bad (each one differs from its payload); of the %d good "
          "rows %d had a bit flipped behind the decoder and were dropped; %d spare rows of erasures dropped"
          % (NOISE_FACTOR, nb, n, good, nb - good, good, int(((ok != 0) & hit).sum()), 3))
