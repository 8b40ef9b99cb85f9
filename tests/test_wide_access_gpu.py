"""GPU tests of the 16-byte sample accesses of the 64-subcarrier row-lane kernels (gfdm_rowlane_impl.h, "16-byte sample accesses").

A call whose device pointers all lie on 16-byte boundaries moves two samples per lane and access; any other call, and every call after
set_wide_access(False), runs the 8-byte form.  Only the data movement differs, so both forms must return the same BITS:

  shapes      K = 64, L = 2 with M = 9 (odd: one 8-byte access for the last 64 elements), M = 8 (no tail) and M = 3 (one row pair + tail);
              M = 9 is compiled into the library, the other two are instantiated at run time (the embedded copy of the same headers)
  paths       modulator, MF demodulator, ZF demodulator, ZF + 2 cancellation rounds
  blocks      1, 3, 4, 5 and 1027 (four blocks per workgroup: partial last workgroups, and more than one)
  alignment   every pointer aligned, and each of in, out, f_eq in turn one complex sample (8 bytes) off: the call must fall back
  expected    torch.equal with the 8-byte route on the same input, and the float64 oracle within 1e-5 (worst block, relative L2)

The inputs and the oracle's results are computed once per shape, for 1027 blocks; the smaller cases take their first blocks.
A stage whose knob is 0 in the build under test (GFDM_WIDE_* in gfdm_rowlane_impl.h; by default only the modulator's input stage is on)
runs its 8-byte code on both routes; built with all four knobs at 1 the same 13 tests pass on an MI355X."""
import numpy as np
import pytest

import gfdm_ref as R
from conftest import check_err, have_gpu, rel_err

pytestmark = pytest.mark.gpu

K, L, ALPHA = 64, 2, 0.2
SHAPES = (9, 8, 3)
BLOCKS = (1, 3, 4, 5, 1027)
BMAX = max(BLOCKS)
PATHS = ("modulate", "demod_mf", "demod_zf", "zf_ic2")
OFFSETS = ("aligned", "in", "out", "f_eq")
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@pytest.fixture(scope="module")
def jit_in_constructor():
    import gfdm_amd
    prev = gfdm_amd.set_jit(gfdm_amd.JIT_IN_CONSTRUCTOR)
    yield
    gfdm_amd.set_jit(prev)


_CASES = {}


def _case(M):
    """handles, inputs (device) and oracle results (host) of one shape, 1027 blocks; cached and never modified"""
    if M in _CASES:
        return _CASES[M]
    import torch
    import gfdm_amd
    from gfdm_amd import synth
    from gfdm_amd.filters import get_frequency_domain_filter
    dev = torch.device("cuda:0")
    N = M * K
    taps = get_frequency_domain_filter("rrc", ALPHA, M, K, L)
    nt = R.normalize_taps(taps, M)
    mod = gfdm_amd.Modulator(M, K, L, taps)
    dem = gfdm_amd.Demodulator(M, K, L, taps)
    adv = gfdm_amd.AdvancedReceiver(M, K, L, taps, np.arange(K), 2, R.qpsk_points())
    want = "rowlane" if M == 9 else "rowlane_jit"
    assert (mod.kernel_name(), dem.kernel_name(), adv.kernel_name()) == (want,) * 3
    sym = synth.qpsk_symbols(0, BMAX, N, dev)
    feq = synth.channel_response(0, BMAX, N, dev)
    prev = gfdm_amd.set_wide_access(False)
    try:
        x = mod.modulate(sym)
    finally:
        gfdm_amd.set_wide_access(prev)
    xe = synth.through_channel(x, feq)
    torch.cuda.synchronize()
    sym_h, x_h, xe_h, feq_h = (t.cpu().numpy() for t in (sym, x, xe, feq))
    c = {
        "N": N, "mod": mod, "dem": dem, "adv": adv,
        "in": {"modulate": sym, "demod_mf": x, "demod_zf": xe, "zf_ic2": xe},
        "f_eq": {"modulate": None, "demod_mf": None, "demod_zf": feq, "zf_ic2": feq},
        "ref": {
            "modulate": R.modulate(sym_h, nt, M, K, L),
            "demod_mf": R.demodulate(x_h, nt, M, K, L),
            "demod_zf": R.demodulate(xe_h, nt, M, K, L, f_eq=feq_h),
            "zf_ic2": R.advanced_receive(xe_h, nt, M, K, L, np.arange(K), R.qpsk_points(), 2, f_eq=feq_h, kind="qpsk"),
        },
    }
    _CASES[M] = c
    return c


def _placed(t, B, N, off, dev):
    """(buffer, view): a view of B blocks that starts on a 256-byte boundary of its buffer (off = 0) or 8 bytes behind one (off = 1), holding the
    first B blocks of t (t = None: NaN, as the two guard elements around the view)"""
    import torch
    buf = torch.full((B * N + 2,), float("nan"), dtype=torch.complex64, device=dev)
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + B * N]
    assert view.data_ptr() % 16 == 8 * off and view.is_contiguous()
    if t is not None:
        view.copy_(t[:B].reshape(-1))
    return buf, view


def _run(c, path, B, off):
    """one call of `path` on the first B blocks; `off` names the operand that lies 8 bytes off a 16-byte boundary"""
    import torch
    N, dev = c["N"], c["in"][path].device
    _, x = _placed(c["in"][path], B, N, 1 if off == "in" else 0, dev)
    o = 1 if off == "out" else 0
    obuf, out = _placed(None, B, N, o, dev)
    f = c["f_eq"][path]
    if f is not None:
        _, f = _placed(f, B, N, 1 if off == "f_eq" else 0, dev)
    if path == "modulate":
        c["mod"].modulate(x, out=out)
    elif path == "demod_mf":
        c["dem"].demodulate(x, out=out)
    elif path == "demod_zf":
        c["dem"].demodulate_equalize(x, f, out=out)
    else:
        c["adv"].demodulate_equalize(x, f, out=out)
    guards = torch.cat((obuf[:o], obuf[o + B * N:]))
    assert guards.numel() == 2 and bool(torch.isnan(guards).all()), "the call wrote outside its output (%s, B=%d, %s)" % (path, B, off)
    return out


@pytest.mark.parametrize("M", SHAPES)
@pytest.mark.parametrize("path", PATHS)
def test_wide_route_equals_narrow_route(M, path, jit_in_constructor):
    import torch
    import gfdm_amd
    c = _case(M)
    lines = []
    for B in BLOCKS:
        prev = gfdm_amd.set_wide_access(False)
        try:
            narrow = _run(c, path, B, "aligned")
        finally:
            assert gfdm_amd.set_wide_access(prev) == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(narrow).any())
        err = rel_err(narrow.cpu().numpy().reshape(B, -1), c["ref"][path][:B])
        print("M=%d %s B=%d: 8-byte route against the oracle %.2e" % (M, path, B, err))
        check_err("wide_%d_%s_%d_narrow" % (M, path, B), err, TOL)
        for off in OFFSETS:
            if off == "f_eq" and c["f_eq"][path] is None:
                continue
            got = _run(c, path, B, off)
            torch.cuda.synchronize()
            same = torch.equal(got, narrow)
            err = rel_err(got.cpu().numpy().reshape(B, -1), c["ref"][path][:B])
            print("M=%d %s B=%d %s: equal to the 8-byte route %s, against the oracle %.2e" % (M, path, B, off, same, err))
            if not same:
                bad = (torch.view_as_real(got) != torch.view_as_real(narrow)).reshape(B, -1).any(dim=1)
                lines.append("M=%d %s B=%d %s: differs from the 8-byte route in blocks %s" % (M, path, B, off, torch.nonzero(bad).flatten()[:8].tolist()))
            if not err < TOL:
                lines.append("M=%d %s B=%d %s: oracle error %.3e exceeds %.1e" % (M, path, B, off, err, TOL))
    assert not lines, "\n".join(lines)


def test_setter_returns_previous_setting():
    import gfdm_amd
    prev = gfdm_amd.set_wide_access(False)
    try:
        assert prev == 1 and gfdm_amd.set_wide_access(True) == 0 and gfdm_amd.set_wide_access(7) == 1 and gfdm_amd.set_wide_access(False) == 1
    finally:
        gfdm_amd.set_wide_access(prev)
