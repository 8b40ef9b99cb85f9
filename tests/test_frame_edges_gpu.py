"""GPU tests of the frame geometry edges and the write extents of the fused transmitter store stage (csrc/gfdm_tx.h: body, prefix copy and
suffix copy of every sample, each with its own window tap, on every port) and of the receivers' frame load and demapper store, on every
kernel route of poison_cases.ROUTES.  The table is tests/frame_edge_cases.py; tests/test_frame_edges.py pins its expectations on the CPU.

Every output lies in a Window: a view `shift` elements past a 16-byte boundary of a larger device buffer, pre-filled with a sentinel, with
canaries on both sides -- one frame in front, bpw frames behind (a kernel that loses the `valid` test of its part-filled last workgroup
writes up to bpw - 1 frames behind the end).  The canaries must survive bit for bit and no sentinel may be left inside: every position
of the output was written, nothing outside it was.  Receiver inputs lie in Windows whose canaries are NaN, and the launch must give the
bits it gives with zeros there: nothing outside the frames was read."""
import numpy as np
import pytest

import frame_edge_cases as E
import gfdm_ref as R
import poison_cases as P
from conftest import check_err, have_gpu, rel_err
from test_poison_gpu import _creating

pytestmark = pytest.mark.gpu
TOL = E.TOL
SENTINEL = complex(-12345.0, 54321.0)
CANARY = complex(7777.0, -3333.0)
NAN = complex(P.NAN, P.NAN)


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.complex64), device="cuda:0")


class Window:
    """n complex64 elements inside a larger device buffer, `shift` elements past a 16-byte boundary, holding `content` or the sentinel,
    with `front` canary elements before and `behind` after it"""

    def __init__(self, n, front, behind, shift, content=None, canary=CANARY):
        import torch
        assert n > 0 and front > 0 and behind > 0 and shift in (0, 1)
        self.lo, self.n = front + (front & 1) + shift, n
        self.buf = torch.full((self.lo + n + behind,), canary, dtype=torch.complex64, device="cuda:0")
        self.view = self.buf[self.lo:self.lo + n]
        assert self.view.is_contiguous() and self.view.numel() == n and self.view.data_ptr() % 16 == 8 * shift
        self.refill(content)
        self.canary = P.bits(self.buf[:1].cpu().numpy()).copy()

    def refill(self, content=None):
        if content is None:
            self.view.fill_(SENTINEL)
        else:
            self.view.copy_(_t(content).reshape(-1))

    def zero_canaries(self):
        self.buf[:self.lo] = 0
        self.buf[self.lo + self.n:] = 0
        self.canary = np.zeros(2, np.uint32)

    def result(self, tag=""):
        """the content, after the canaries were found intact"""
        import torch
        torch.cuda.synchronize()
        b = P.bits(self.buf.cpu().numpy()).reshape(-1, 2)
        for name, part in (("in front of", b[:self.lo]), ("behind", b[self.lo + self.n:])):
            bad = np.argwhere((part != self.canary).any(axis=1))[:4, 0].tolist()
            assert not bad, "%s: written %s the output, canary elements %s" % (tag, name, bad)
        return b[self.lo:self.lo + self.n].copy().view(np.complex64).reshape(-1)


def _unwritten(a):
    """positions of `a` that still hold the sentinel"""
    s = P.bits(np.array([SENTINEL], np.complex64))
    b = P.bits(a).reshape(-1, 2)
    return np.argwhere((b == s).all(axis=1))[:6, 0].tolist()


def _shape(route):
    return P.ROUTES[route]["shape"]


def _transmitter(route, c):
    import gfdm_amd
    with _creating(route):
        tx = gfdm_amd.Transmitter(c["M"], c["K"], c["A"], c["cp"], c["cs"], c["ramp"], c["smap"], c["per_ts"], c["L"], c["taps"],
                                  np.asarray(c["window"]), c["shifts"], c["preambles"])
    assert tx.kernel_name() == P.ROUTES[route]["kernel"]
    assert tx.output_vector_size() == c["F"] and tx.block_size() == c["N"] and tx.input_vector_size() == c["A"] * c["M"]
    return tx


def _check_frames(tag, c, port, got, nb):
    """one port's frames against the complex64 preamble (bit-equal) and the float64 oracle: prefix, body and suffix each within
    TOL sqrt(|S|) rms(body of that frame), the whole frame within TOL"""
    ref = np.asarray(c["frames"][port])[:nb]
    assert got.shape == ref.shape
    assert not _unwritten(got), "%s: frame positions never written: %s" % (tag, _unwritten(got))
    pre = np.broadcast_to(np.asarray(c["preambles"][port]).astype(np.complex64), (nb, c["plen"]))
    assert np.array_equal(P.bits(got[:, :c["plen"]]), P.bits(pre)), "%s: the preamble is not the one given" % tag
    seg = E.segments(c, port)
    rms = np.sqrt(np.mean(np.abs(ref[:, seg["body"]]) ** 2, axis=1))
    assert np.all(rms > 0)
    for name, sl in seg.items():
        n = sl.stop - sl.start
        if n:
            err = float(np.max(np.linalg.norm(got[:, sl] - ref[:, sl], axis=1) / (np.sqrt(n) * rms)))
            check_err("edge_seg_%s_%s" % (tag, name), err, TOL)
    check_err("edge_tx_" + tag, rel_err(got, ref), TOL)


def _symbols(c, nb, shift):
    """the symbols of the first nb blocks, NaN in front of and behind them: a mapper that reads past ninput_size shows in the frames"""
    return Window(nb * c["nin"], c["nin"], c["nin"], shift, content=np.asarray(c["sym"])[:nb], canary=NAN)


def _transmit(route, tx, c, cid, nb, flip=0, n_ports=None):
    """transmit(outs=) of the first nb blocks of the case into one Window per port; the Windows, after every check"""
    F, w = c["F"], E.bpw(route)
    ports = len(c["shifts"]) if n_ports is None else n_ports
    sym = _symbols(c, nb, flip % 2)
    wins = [Window(nb * F, F, w * F, (port + flip) % 2) for port in range(ports)]
    outs = tx.transmit(sym.view, ninput_size=c["nin"], n_ports=n_ports, outs=[x.view for x in wins])
    sym.result("symbols")
    assert len(outs) == ports and all(o.data_ptr() == x.view.data_ptr() for o, x in zip(outs, wins))
    for port, x in enumerate(wins):
        tag = "%s_%s_B%d_p%d" % (route, cid, nb, port) if nb != E.blocks(route) else "%s_%s_p%d" % (route, cid, port)
        _check_frames(tag, c, port, x.result(tag).reshape(nb, F), nb)
    return wins


@pytest.mark.parametrize("route", E.TX_ROUTES)
@pytest.mark.parametrize("geom", E.GEOMETRIES)
def test_transmitter_frame_edges(route, geom):
    import torch
    M, K, L = _shape(route)
    B, w = E.blocks(route), E.bpw(route)
    handles = {}
    for i, case in enumerate(c for c in E.tx_cases() if c[0] == geom):
        c = E.tx_case(M, K, L, B, case)
        key = (case[1], case[2])
        if key not in handles:
            handles[key] = _transmitter(route, c)
        _transmit(route, handles[key], c, E.case_id(case), B, flip=i)
    if geom != "ports8":
        return
    # part-filled and exactly filled single workgroups
    case = ("ports8", "all", True, "full")
    c, tx = E.tx_case(M, K, L, B, case), handles[("all", True)]
    for nb in sorted({1, w}):
        _transmit(route, tx, c, E.case_id(case), nb, flip=nb)
    # fewer ports than the handle has (the single-port stores), the bare modulated blocks, and add_frame on them
    case = ("ports8", "ends", False, "short")
    cid = E.case_id(case)
    c, tx = E.tx_case(M, K, L, B, case), handles[("ends", False)]
    N, F = c["N"], c["F"]
    full = _transmit(route, tx, c, cid + "_again", B)
    one = _transmit(route, tx, c, cid + "_1port", B, flip=1, n_ports=1)
    assert torch.equal(one[0].view, full[0].view)
    sym = _symbols(c, B, 1).view
    mod = Window(B * N, N, w * N, 1)
    assert tx.modulate(sym, ninput_size=c["nin"], out=mod.view).data_ptr() == mod.view.data_ptr()
    blocks = mod.result("modulate %s" % route).reshape(B, N)
    assert not _unwritten(blocks)
    check_err("edge_tx_modulate_%s_%s" % (route, cid), rel_err(blocks, np.asarray(c["block"])), TOL)
    for port, s in enumerate(c["shifts"]):
        fr = Window(B * F, F, w * F, port % 2)
        tx.add_frame(mod.view, s, out=fr.view)
        tag = "%s_%s_addframe_p%d" % (route, cid, port)
        got = fr.result(tag).reshape(B, F)
        _check_frames(tag, c, port, got, B)
        assert rel_err(got, full[port].view.cpu().numpy().reshape(B, F)) < 1e-6      # two kernels, same arithmetic
    with pytest.raises(ValueError, match="no preamble"):
        tx.add_frame(mod.view, len(c["shifts"]) + 1, out=Window(B * F, F, w * F, 0).view)
    with pytest.raises(RuntimeError, match="expected"):
        tx.transmit(sym, ninput_size=c["nin"], n_ports=1, outs=[mod.view])


# ---------------------------------------------------------------- receivers

def _receivers(route, taps, smap):
    """{"zf": Demodulator, "ic": AdvancedReceiver} of a route (the IC receiver alone on the *_ic_mx routes), kernel_name() asserted"""
    import gfdm_amd
    M, K, L = _shape(route)
    rx = {}
    with _creating(route):
        if P.ROUTES[route]["modes"] == P.ALL:
            rx["zf"] = gfdm_amd.Demodulator(M, K, L, taps)
        rx["ic"] = gfdm_amd.AdvancedReceiver(M, K, L, taps, np.sort(smap), P.IC_ITER, R.qpsk_points())
    assert all(h.kernel_name() == P.ROUTES[route]["kernel"] for h in rx.values())
    assert rx["ic"].decision_rule() == "qpsk" and rx["ic"].get_phase_compensation() == 0
    return rx


def _run_twice(tag, call, inputs, out, nb, nout, want, keep):
    """`call` once with NaN canaries around every input and once with zeros there: finite, all written, canaries intact, the oracle's
    result within TOL, and the same bits both times"""
    call()
    a = out.result(tag).reshape(nb, nout)
    assert not _unwritten(a), "%s: output positions never written: %s" % (tag, _unwritten(a))
    assert np.isfinite(a).all(), "%s: something outside the frames was read" % tag
    assert keep.sum() * 2 >= nb
    check_err("edge_rx_" + tag, rel_err(a[keep], np.asarray(want)[keep]), TOL)
    for x in inputs:
        x.zero_canaries()
    out.refill()
    call()
    b = out.result(tag).reshape(nb, nout)
    assert np.array_equal(P.bits(a), P.bits(b)), "%s: the result depends on what lies around the frames" % tag


@pytest.mark.parametrize("route", E.RX_ROUTES)
@pytest.mark.parametrize("mname", E.MAPS)
def test_receiver_frame_edges(route, mname):
    M, K, L = _shape(route)
    B, w = E.blocks(route), E.bpw(route)
    d = E.rx_data(M, K, L, B, mname)
    N = d["N"]
    rx = _receivers(route, d["taps"], d["smap"])
    feq = _t(d["feq"])
    xe = np.asarray(d["xe"]).astype(np.complex64)
    rng = np.random.default_rng(K + M)
    for i, case in enumerate(E.rx_cases(mname)):
        cp, frame_len = E.layout(case[0], N)
        frames = (rng.standard_normal((B, frame_len)) + 1j * rng.standard_normal((B, frame_len))).astype(np.complex64)
        frames[:, cp:cp + N] = xe
        nout_arg = E.nout_of(case[3], d["A"], M)[0] if case[1] else None
        for mode, h in rx.items():
            want = E.rx_expected(d, np.asarray(d["ref_" + mode]), case)
            nout = want.shape[1]
            keep = np.asarray(d["keep_ic"]) if mode == "ic" else np.ones(B, bool)
            h.configure_frames(frame_len, cp, d["smap"] if case[1] else None, case[2])
            fin = Window(B * frame_len, frame_len, w * frame_len, i % 2, content=frames, canary=NAN)
            out = Window(B * nout, nout, w * nout, (i + 1) % 2)
            call = lambda: h.demodulate_frames(fin.view, feq, noutput_size=nout_arg, out=out.view.view(B, nout))
            _run_twice("%s_%s_%s_%s" % (route, mname, E.rx_case_id(case), mode), call, [fin], out, B, nout, want, keep)


@pytest.mark.parametrize("route", E.RX_ROUTES)
def test_estimated_frame_edges(route):
    """demodulate_estimated with the preamble in front of every frame, behind it (the last one ends on the buffer's last element), and
    packed in a buffer of its own"""
    import gfdm_amd
    M, K, L = _shape(route)
    B, w = E.blocks(route), E.bpw(route)
    e = E.est_data(M, K, L, B)
    N, A = e["N"], e["A"]
    rx = _receivers(route, e["taps"], e["smap"])
    with _creating(route):
        est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, np.asarray(e["pre"]))
    assert est.kernel_name() in (P.ROUTES[route]["kernel"], "generic_lds")
    rng = np.random.default_rng(K + M)
    nout = A * M
    for i, name in enumerate(E.EST_LAYOUTS):
        frames, cp, frame_len, pre_at, stride = E.est_frames(e, name, rng)
        for mode, h in rx.items():
            keep = np.asarray(e["keep_ic"]) if mode == "ic" else np.ones(B, bool)
            h.set_channel_estimator(est)
            h.configure_frames(frame_len, cp, e["smap"], True)
            fin = Window(B * frame_len, frame_len, w * frame_len, i % 2, content=frames, canary=NAN)
            inputs = [fin]
            if pre_at is None:
                inputs.append(Window(B * 2 * K, 2 * K, w * 2 * K, (i + 1) % 2, content=e["rx_pre"], canary=NAN))
                pre = inputs[1].view
            else:
                pre = fin.view[pre_at:]
                assert pre.numel() >= (B - 1) * stride + 2 * K and (name != "pre_back" or pre.numel() == (B - 1) * stride + 2 * K)
            out = Window(B * nout, nout, w * nout, (i + 1) % 2)
            call = lambda: h.demodulate_estimated(fin.view, pre, preamble_stride=stride, out=out.view.view(B, nout))
            _run_twice("%s_est_%s_%s" % (route, name, mode), call, inputs, out, B, nout, e["want_" + mode], keep)
            h.set_channel_estimator(None)
