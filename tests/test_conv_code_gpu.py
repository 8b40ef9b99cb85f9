"""GPU tests of the convolutional code (contract in include/gfdm_hip.h, gfdm_hip_conv_code).  The yardstick is the numpy restatement of
tests/conv_code_ref.py, which tests/test_conv_code.py holds to facts that do not depend on it.  Everything is integer arithmetic, so every
comparison is bit for bit, path_metric included; there is no tolerance anywhere.  Every output written through out= lies between canaries.

Seen on an MI355X in the end-to-end test (noise 4 x the loop's, 7 bursts of 924 coded bits): the figures are in
profiles/r16/conv_code_kernel_durations.txt."""
import numpy as np
import pytest

import burst_shaper_ref as B
import channel_model_ref as C
import conv_code_ref as V
import gfdm_ref as R
from conftest import have_gpu

pytestmark = pytest.mark.gpu
MODES = [V.TERMINATED, V.TRUNCATED]
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


def _code(polys=V.POLYS, mode=V.TERMINATED):
    import gfdm_amd
    return gfdm_amd.ConvolutionalCode(polys, mode)


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


def noisy_llr(rng, data, n_info, polys, mode, amp=4.0, sigma=2.5, stride=None):
    """LLRs of the encoded rows plus noise, float32 (n_rows, stride); with gain 16 a good part of them saturates at +-127"""
    c = V.encode_bits(V.unpack(data, n_info), polys, mode)
    llr = (amp * (1.0 - 2.0 * c) + sigma * rng.standard_normal(c.shape)).astype(np.float32)
    if stride is not None and stride > llr.shape[1]:
        llr = np.concatenate((llr, np.full((llr.shape[0], stride - llr.shape[1]), np.nan, np.float32)), axis=1)
    return llr


def check_decode(cc, llr, n_info, gain, polys, mode, tag, **kw):
    """cc.decode on the device against the restatement, bytes and path_metric"""
    n_rows = llr.shape[0]
    pm = Window(n_rows, np.int32, kw.pop("pm_shift", 0))
    out = Window((n_rows, V.info_bytes(n_info)), np.uint8, kw.pop("out_shift", 0))
    x = kw.pop("x", None)
    cc.decode(_t(llr) if x is None else x, n_info, gain, out=out.view, path_metric=pm.view, **kw)
    want, metric = V.decode(llr, n_info, gain, polys, mode)
    got, got_pm = out.result(), pm.result()
    assert np.array_equal(got_pm, metric), "%s: path_metric differs in %d of %d rows" % (tag, int((got_pm != metric).sum()), n_rows)
    assert np.array_equal(got, want), "%s: %d rows differ" % (tag, int((got != want).any(axis=1).sum()))
    return got, got_pm


def flip(rng, coded, n_bits, most=4):
    """the packed rows with 1 .. most bits flipped in each, inside the first n_bits"""
    bits = np.unpackbits(coded, axis=1)
    for r in range(bits.shape[0]):
        bits[r, rng.choice(n_bits, size=min(n_bits, int(rng.integers(1, most + 1))), replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def lds_edge(mode):
    """the last n_info whose survivor decisions stay in LDS"""
    return V.LDS_STEPS - (6 if mode == V.TERMINATED else 0)


SHAPES = [1, 2, 5, 6, 7, 8, 57, 58, 59, 122, 456, "edge", "edge+1", "edge+2"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_info", SHAPES)
def test_every_shape(n_info, mode):
    """encode, decode and decode_hard against the restatement: rows shorter than the register (unreachable states keep the -2^30 start),
    either side of the 64-step chunk, and either side of GFDM_HIP_CC_LDS_STEPS, where the decisions move from LDS to the workspace"""
    if isinstance(n_info, str):
        n_info = lds_edge(mode) + int(n_info[5:] or 0)
    cc = _code(V.POLYS, mode)
    T = n_info + (6 if mode == V.TERMINATED else 0)
    assert (cc.steps(n_info), cc.coded_bits(n_info), cc.coded_bytes(n_info), cc.info_bytes(n_info)) == (T, 2 * T, -(-2 * T // 8), -(-n_info // 8))
    assert (cc.workspace_bytes(n_info, 5) == 0) == (T <= V.LDS_STEPS)
    assert cc.workspace_bytes(n_info, 5) in (0, 5 * 8 * (-(-T // 64) * 64)) and cc.workspace_bytes(n_info, 10 ** 6) == cc.workspace_bytes(n_info, 2048)
    rng = np.random.default_rng(1000 + n_info)
    n_rows = 5
    data = V.random_info(rng, n_rows, n_info)
    # encode: at the row's own width and three bytes wider (zero padded)
    for extra in (0, 3):
        width = V.coded_bytes(n_info, mode) + extra
        out = Window((n_rows, width), np.uint8, extra)
        cc.encode(_t(data), n_info, out_row_bytes=width, out=out.view)
        assert np.array_equal(out.result(), V.encode(data, n_info, V.POLYS, mode, width)), "encode, %d bytes wider" % extra
    coded = V.encode(data, n_info, V.POLYS, mode)
    # soft decode of noisy rows
    check_decode(cc, noisy_llr(rng, data, n_info, V.POLYS, mode), n_info, 16.0, V.POLYS, mode, "soft")
    # hard decode: of the clean rows, and of rows with up to four flipped bits (a terminated row then still decodes to the payload)
    pm = Window(n_rows, np.int32)
    got = _h(cc.decode_hard(_t(coded), n_info, path_metric=pm.view))
    assert np.array_equal(got, V.clean(data, n_info)) and np.all(pm.result() == 2 * T)
    bad = flip(rng, coded, 2 * T)
    got = _h(cc.decode_hard(_t(bad), n_info, path_metric=pm.view))
    want, metric = V.decode_hard(bad, n_info, V.POLYS, mode)
    assert np.array_equal(got, want) and np.array_equal(pm.result(), metric)
    if mode == V.TERMINATED:
        assert np.array_equal(got, V.clean(data, n_info))
    # decode_hard is decode on +-1 with gain 1
    check_decode(cc, V.hard_values(bad, n_info, mode).astype(np.float32), n_info, 1.0, V.POLYS, mode, "soft on +-1")


@pytest.mark.parametrize("mode", MODES)
def test_one_long_row_in_the_workspace(mode):
    """2^16 + 3 information bits: 1025 chunks of decisions in the caller's workspace"""
    import torch
    n_info = 2 ** 16 + 3
    cc = _code(V.POLYS, mode)
    rng = np.random.default_rng(77)
    data = V.random_info(rng, 1, n_info)
    llr = noisy_llr(rng, data, n_info, V.POLYS, mode)
    need = cc.workspace_bytes(n_info, 1)
    assert need == 8 * (-(-cc.steps(n_info) // 64) * 64)
    ws = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    got, _ = check_decode(cc, llr, n_info, 16.0, V.POLYS, mode, "long row", workspace=ws[:need])
    assert np.all(_h(ws[need:]) == 0xEE), "written behind the workspace"
    assert np.unpackbits(got ^ V.clean(data, n_info)).sum() < n_info // 100       # (the noise is mild: the row comes back nearly whole)
    with pytest.raises(TypeError):
        cc.decode(_t(llr), n_info, 16.0, workspace=ws[:need - 1])


@pytest.mark.parametrize("n_rows, n_info", [(1, 3), (3, 3), (4, 3), (5, 3), (7, 3), (5000, 3), (32768 + 7, 2)])
def test_rows_per_call(n_rows, n_info):
    """fewer rows than a workgroup's four waves, a partly filled last workgroup, and more rows than the bounded grid has waves"""
    rng = np.random.default_rng(n_rows)
    for mode in MODES:
        cc = _code(V.POLYS, mode)
        data = V.random_info(rng, n_rows, n_info)
        got = _h(cc.encode(_t(data), n_info))
        assert np.array_equal(got, V.encode(data, n_info, V.POLYS, mode))
        out = Window(got.shape, np.uint8, 5)                 # the many rows are more than a tile's 4096 coded bytes: a tile seam in an unaligned output
        cc.encode(_t(data), n_info, out=out.view)
        assert np.array_equal(out.result(), V.encode(data, n_info, V.POLYS, mode)), "encode at byte 5"
        check_decode(cc, noisy_llr(rng, data, n_info, V.POLYS, mode), n_info, 16.0, V.POLYS, mode, "%d rows" % n_rows)
        pm = Window(n_rows, np.int32, 1)
        bad = flip(rng, got, V.coded_bits(n_info, mode), 2)
        want, metric = V.decode_hard(bad, n_info, V.POLYS, mode)
        assert np.array_equal(_h(cc.decode_hard(_t(bad), n_info, path_metric=pm.view)), want) and np.array_equal(pm.result(), metric)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("polys", [(109, 79), (109, -79), (91, 121), (55, 79)])
def test_polys(polys, mode):
    """the default pair, a complemented output, the pair in the other bit order, and a generator without bit 6 (55 = 0110111), for which the
    two branch metrics of a state are no longer each other's negative"""
    cc = _code(polys, mode)
    assert cc.polys() == polys and cc.mode() == mode
    rng = np.random.default_rng(abs(polys[0] * 131 + polys[1]))
    for n_info in (7, 59, 122):
        data = V.random_info(rng, 6, n_info)
        assert np.array_equal(_h(cc.encode(_t(data), n_info)), V.encode(data, n_info, polys, mode))
        check_decode(cc, noisy_llr(rng, data, n_info, polys, mode), n_info, 16.0, polys, mode, "polys %s" % (polys,))
        bad = flip(rng, V.encode(data, n_info, polys, mode), V.coded_bits(n_info, mode))
        assert np.array_equal(_h(cc.decode_hard(_t(bad), n_info)), V.decode_hard(bad, n_info, polys, mode)[0])


@pytest.mark.parametrize("mode", MODES)
def test_llr_values(mode):
    """saturation, exact halves after the gain (half to even), NaN, +-inf, and a row of erasures"""
    cc = _code(V.POLYS, mode)
    n_info, n_rows = 122, 8
    rng = np.random.default_rng(9)
    cb = V.coded_bits(n_info, mode)
    data = V.random_info(rng, n_rows, n_info)
    sign = 1.0 - 2.0 * V.encode_bits(V.unpack(data, n_info), V.POLYS, mode)
    # rows 0, 1: odd multiples of 0.25 times gain 2 are exact halves
    halves = ((2 * rng.integers(-300, 300, (n_rows, cb)) + 1) * 0.25).astype(np.float32)
    check_decode(cc, halves, n_info, 2.0, V.POLYS, mode, "halves")
    assert np.any(np.abs(halves * 2) > 127) and np.any(np.abs(halves * 2) < 127)
    # magnitudes 0.5, 1.5, 2.5 with the code's signs: rint gives 0, 2, 2
    small = (sign * rng.choice([0.5, 1.5, 2.5], size=sign.shape)).astype(np.float32)
    check_decode(cc, small, n_info, 1.0, V.POLYS, mode, "small halves")
    # non-finite values sprinkled over noisy rows; one row all NaN, one all +inf, one all -inf
    llr = noisy_llr(rng, data, n_info, V.POLYS, mode)
    where = rng.random(llr.shape)
    llr[where < 0.05] = np.nan
    llr[(where >= 0.05) & (where < 0.10)] = np.inf
    llr[(where >= 0.10) & (where < 0.15)] = -np.inf
    llr[5], llr[6], llr[7] = np.nan, np.inf, -np.inf
    check_decode(cc, llr, n_info, 16.0, V.POLYS, mode, "non-finite")
    # erasures: zero bits and metric 0 by the tie rule (NaN rows and zero rows alike)
    zero = np.zeros((3, cb), np.float32)
    zero[1] = np.nan
    zero[2] = -0.0
    got, pm = check_decode(cc, zero, n_info, 16.0, V.POLYS, mode, "erasures")
    assert not got.any() and not pm.any()


@pytest.mark.parametrize("extra", [0, 1, 12])
def test_llr_stride_and_alignment(extra):
    """rows wider than the coded bits with NaN behind them, and every buffer at every alignment of one element: the LLRs at the four float
    positions of a 16-byte line (odd strides move the pairs of every other row off their 8-byte alignment), path_metric likewise, bytes at
    all 16"""
    n_info, n_rows = 59, 6
    rng = np.random.default_rng(20 + extra)
    for mode in MODES:
        cc = _code(V.POLYS, mode)
        cb = V.coded_bits(n_info, mode)
        data = V.random_info(rng, n_rows, n_info)
        llr = noisy_llr(rng, data, n_info, V.POLYS, mode, stride=cb + extra)
        for shift in range(4):
            x = Window((n_rows, cb + extra), np.float32, shift, llr)
            check_decode(cc, llr, n_info, 16.0, V.POLYS, mode, "stride +%d, shift %d" % (extra, shift), x=x.view, pm_shift=shift, out_shift=shift + 4 * extra % 16)
        if extra:
            continue
        coded = V.encode(data, n_info, V.POLYS, mode)
        for shift in range(16):
            out = Window((n_rows, coded.shape[1] + 3), np.uint8, shift)
            src = Window(data.shape, np.uint8, 15 - shift, data)
            cc.encode(src.view, n_info, out_row_bytes=coded.shape[1] + 3, out=out.view)
            assert np.array_equal(out.result(), V.encode(data, n_info, V.POLYS, mode, coded.shape[1] + 3)), "encode at byte %d" % shift
            src = Window(coded.shape, np.uint8, shift, coded)
            out = Window(data.shape, np.uint8, 15 - shift)
            cc.decode_hard(src.view, n_info, out=out.view)
            assert np.array_equal(out.result(), V.clean(data, n_info)), "decode_hard at byte %d" % shift


@pytest.mark.parametrize("count", [0, 3, 9, 10, 15, -2])
def test_count(count):
    """rows from clamp(count, 0, n_rows) on are zeros with metric 0, and their input -- NaN, and bytes that would decode to ones -- is not read"""
    import torch
    n_info, n_rows = 58, 10
    live = min(max(count, 0), n_rows)
    rng = np.random.default_rng(30)
    cc = _code()
    data = V.random_info(rng, n_rows, n_info)
    llr = noisy_llr(rng, data, n_info, V.POLYS, V.TERMINATED)
    want, metric = V.decode(llr, n_info, 16.0)
    want[live:], metric[live:] = 0, 0
    poisoned = llr.copy()
    poisoned[live:] = np.nan
    for cnt in (count, torch.tensor([count], dtype=torch.int64, device="cuda:0")):
        pm, out = Window(n_rows, np.int32), Window(want.shape, np.uint8)
        cc.decode(_t(poisoned), n_info, 16.0, count=cnt, out=out.view, path_metric=pm.view)
        assert np.array_equal(out.result(), want) and np.array_equal(pm.result(), metric)
    coded = V.encode(data, n_info)
    want_c = coded.copy()
    want_c[live:] = 0
    out = Window(coded.shape, np.uint8, 5)
    cc.encode(_t(data), n_info, count=count, out=out.view)
    assert np.array_equal(out.result(), want_c)
    want_h = V.clean(data, n_info)
    want_h[live:] = 0
    pm, out = Window(n_rows, np.int32), Window(want_h.shape, np.uint8)
    cc.decode_hard(_t(coded), n_info, count=count, out=out.view, path_metric=pm.view)
    assert np.array_equal(out.result(), want_h) and np.array_equal(pm.result(), np.where(np.arange(n_rows) < live, 2 * (n_info + 6), 0))


def test_argument_errors_on_the_device():
    import gfdm_amd
    cc = _code()
    llr = _t(np.zeros((2, 2 * 14), np.float32))
    for call in (lambda: cc.decode(llr, 9, 1.0), lambda: cc.decode(llr, 8, 0.0), lambda: cc.decode(llr, 8, float("nan")),
                 lambda: cc.decode(llr, 8, float("inf")), lambda: cc.decode(llr, 0, 1.0), lambda: cc.decode_hard(_t(np.zeros((2, 3), np.uint8)), 8),
                 lambda: cc.encode(_t(np.zeros((2, 1), np.uint8)), 8, out_row_bytes=3), lambda: cc.steps(2 ** 20)):
        with pytest.raises(ValueError):
            call()
    assert gfdm_amd.lib().gfdm_hip_last_error()
    with pytest.raises(RuntimeError):
        cc.encode(_t(np.zeros((2, 2), np.uint8)), 8)             # rows of the wrong width
    empty = cc.decode(_t(np.zeros((0, 28), np.float32)), 8, 1.0)
    assert tuple(empty.shape) == (0, 1)
    one = cc.decode(llr[0], 8, 1.0)                              # a 1-D input is one row
    assert tuple(one.shape) == (1,) and int(one[0]) == 0


def test_host_flavour_equals_device_flavour_and_calls_repeat():
    rng = np.random.default_rng(40)
    for mode, n_info in ((V.TERMINATED, 122), (V.TRUNCATED, 2100)):
        cc = _code(V.POLYS, mode)
        n_rows = 7
        data = V.random_info(rng, n_rows, n_info)
        llr = noisy_llr(rng, data, n_info, V.POLYS, mode)
        want, metric = V.decode(llr, n_info, 16.0, V.POLYS, mode)
        pm_h = np.full(n_rows, -1, np.int32)
        got_h = cc.decode(llr, n_info, 16.0, count=6, path_metric=pm_h)
        assert isinstance(got_h, np.ndarray) and np.array_equal(got_h[:6], want[:6]) and not got_h[6:].any()
        assert np.array_equal(pm_h[:6], metric[:6]) and pm_h[6] == 0
        first = check_decode(cc, llr, n_info, 16.0, V.POLYS, mode, "first call")
        second = check_decode(cc, llr, n_info, 16.0, V.POLYS, mode, "second call")
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        coded_h = cc.encode(data, n_info, out_row_bytes=V.coded_bytes(n_info, mode) + 2)
        assert np.array_equal(coded_h, V.encode(data, n_info, V.POLYS, mode, V.coded_bytes(n_info, mode) + 2))
        assert np.array_equal(coded_h, _h(cc.encode(_t(data), n_info, out_row_bytes=coded_h.shape[1])))
        assert np.array_equal(cc.decode_hard(coded_h, n_info), V.clean(data, n_info))
        assert np.array_equal(cc.decode(llr[0], n_info, 16.0), want[0])
        # the host flavours with the optional operands the calls above leave out: encode with a count, decode_hard with a count and a path_metric
        enc_h = cc.encode(data, n_info, count=4)
        assert isinstance(enc_h, np.ndarray) and np.array_equal(enc_h, _h(cc.encode(_t(data), n_info, count=4))) and enc_h[:4].any() and not enc_h[4:].any()
        pm_h, pm_d = np.full(n_rows, -1, np.int32), _t(np.full(n_rows, -1, np.int32))
        hard_h = cc.decode_hard(coded_h, n_info, count=4, path_metric=pm_h)
        assert np.array_equal(hard_h, _h(cc.decode_hard(_t(coded_h), n_info, count=4, path_metric=pm_d))) and np.array_equal(pm_h, _h(pm_d))
        assert np.array_equal(hard_h[:4], V.clean(data, n_info)[:4]) and not hard_h[4:].any()


def test_graph_of_soft_and_decode_replays_with_a_changed_count():
    """SymbolMapper.soft -> decode captured once (two kernels, no allocation inside: every buffer is given); the replays follow the count and the
    symbols on the device"""
    import torch
    import gfdm_amd
    n_info, n_rows = 122, 9
    cb = V.coded_bits(n_info)
    pts = R.qpsk_points().astype(np.complex64)
    m = gfdm_amd.SymbolMapper(pts)
    cc = _code()
    rng = np.random.default_rng(50)

    def symbols(seed):
        r = np.random.default_rng(seed)
        data = V.random_info(r, n_rows, n_info)
        c = V.encode_bits(V.unpack(data, n_info))
        s = pts[2 * c[:, 0::2] + c[:, 1::2]]
        return (s + 0.35 * (r.standard_normal(s.shape) + 1j * r.standard_normal(s.shape))).astype(np.complex64)

    sym = _t(symbols(1))
    scale = _t(rng.uniform(2.0, 6.0, n_rows).astype(np.float32))
    count = torch.tensor([n_rows], dtype=torch.int64, device="cuda:0")
    llr = torch.zeros((n_rows, cb), dtype=torch.float32, device="cuda:0")
    out, pm = Window((n_rows, V.info_bytes(n_info)), np.uint8, 3), Window(n_rows, np.int32, 1)

    def run():
        m.soft(sym, scale, count=count, out=llr)
        cc.decode(llr, n_info, 4.0, count=count, out=out.view, path_metric=pm.view)

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
        want, metric = V.decode(got_llr, n_info, 4.0)          # the restatement on the LLRs the device made
        want[cnt:], metric[cnt:] = 0, 0
        assert np.array_equal(out.result(), want) and np.array_equal(pm.result(), metric), "replay with count %d" % cnt


def test_coding_gain_inputs():
    """the rows tests/test_conv_code.py::test_coding_gain_inputs holds on the CPU: every row decodes to its payload"""
    payload, llr, _ = V.coding_gain_case()
    got, _ = check_decode(_code(), llr, V.GAIN_N_INFO, V.GAIN_GAIN, V.POLYS, V.TERMINATED, "coding gain")
    assert np.array_equal(got, payload)


NOISE_FACTOR = 4.0                           # the end-to-end loop's noise, over tests/channel_model_ref.py's LOOP_NOISE_VOLTAGE (20 dB below the frames)


def test_end_to_end_on_the_device():
    """information bytes -> encode -> map -> transmit -> place -> ChannelModel.apply (noise on) -> detect -> demodulate_bursts ->
    LinkMeter.measure (decision-directed: the scale) -> soft -> decode, and SymbolMapper.decode -> decode_hard, on the loop fixtures of
    tests/test_channel_model_gpu.py with four times their noise voltage.  Asserted: the device's decoded bytes are the restatement's on the
    downloaded LLRs / bytes, and decoding leaves no more information-bit errors than the hard decisions had coded-bit errors.  The error
    counts themselves are printed, not asserted.  Seen on an MI355X: 100 of 6468 coded bits wrong in the hard decisions, 0 of 3192
    information bits wrong after decode and after decode_hard."""
    import gfdm_amd
    c = B.loop_case()
    M, K, L, A, N, cp, nb = c["M"], c["K"], c["L"], c["A"], c["N"], c["cp"], c["nb"]
    n_sym, n_info = A * M, 456
    pts = R.qpsk_points().astype(np.complex64)
    m = gfdm_amd.SymbolMapper(pts)
    cc = _code()
    assert cc.coded_bytes(n_info) <= m.row_bytes(n_sym) and cc.coded_bits(n_info) <= 2 * n_sym
    rng = np.random.default_rng(60)
    info = V.clean(V.random_info(rng, nb, n_info), n_info)
    coded = cc.encode(_t(info), n_info, out_row_bytes=m.row_bytes(n_sym))             # as wide as map's rows: no kernel in between
    assert np.array_equal(_h(coded), V.encode(info, n_info, out_row_bytes=m.row_bytes(n_sym)))
    sym = m.map(coded, n_sym)
    tx = gfdm_amd.Transmitter(M, K, A, cp, 0, 0, c["smap"], True, L, c["taps"], np.ones(N + cp), [0], [c["full_preamble"]])
    frames = tx.transmit(sym)
    sh = gfdm_amd.BurstShaper(c["frame_len"], scale=B.LOOP_SCALE)
    placed = sh.place(frames, _t(c["starts"]), c["out_len"])[0]
    ch = gfdm_amd.ChannelModel(NOISE_FACTOR * C.LOOP_NOISE_VOLTAGE, C.LOOP_F, 1.0, C.LOOP_TAPS, C.LOOP_SEED)
    ds = ch.apply(placed)
    sync = gfdm_amd.BurstSync(K, c["pcp"], c["preamble"], c["window_len"])
    r = sync.detect(ds, B.LOOP_THRESHOLD, c["min_distance"], c["lead"], max_bursts=nb + 3)
    assert int(r["count"][0]) == nb, "the loop's bursts were not all found at this noise: the rows below would not line up with the payload"
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    rx = gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, pts)
    rx.configure_frames(c["F"], 2 * K + cp, c["smap"], True)
    rx.set_channel_estimator(est)
    demod = rx.demodulate_bursts(ds, r["frame_start"], r["sc_rot"], r["count"])
    meter = gfdm_amd.LinkMeter(pts)
    noise = meter.measure(demod, count=r["count"])                                       # decision-directed: err_power / n_sym estimates the noise
    scale = (n_sym / noise["err_power"].clamp_min(1e-12)).float()
    llr = m.soft(demod, scale, count=r["count"])
    pm = Window(nb + 3, np.int32)
    got = _h(cc.decode(llr, n_info, 4.0, count=r["count"], path_metric=pm.view))
    want, metric = V.decode(_h(llr), n_info, 4.0)
    want[nb:], metric[nb:] = 0, 0
    assert np.array_equal(got, want) and np.array_equal(pm.result(), metric)
    hard = m.decode(demod, count=r["count"])
    got_hard = _h(cc.decode_hard(hard, n_info, count=r["count"]))
    want_hard = V.decode_hard(_h(hard), n_info)[0]
    want_hard[nb:] = 0
    assert np.array_equal(got_hard, want_hard)
    cbits = cc.coded_bits(n_info)
    uncoded = int((V.unpack(_h(hard)[:nb], cbits) != V.unpack(_h(coded), cbits)).sum())
    after_soft = int(np.unpackbits(got[:nb] ^ info).sum())
    after_hard = int(np.unpackbits(got_hard[:nb] ^ info).sum())
    print("end to end, noise x%g: %d of %d coded bits wrong in the hard decisions; information-bit errors of %d: %d after decode, %d after decode_hard"
          % (NOISE_FACTOR, uncoded, nb * cbits, nb * n_info, after_soft, after_hard))
    assert after_soft <= uncoded
