"""GPU poison tests: a zero, infinite or NaN equaliser bin, a non-finite sample, a NaN symbol or NaN junk next to the data of ONE block,
frame or burst stays in that block, frame or burst -- on every kernel route (tests/poison_cases.py: ROUTES).

Finite random data cannot see a lane, row or block that is blended in with a multiply-by-mask instead of a select, a read of samples
that should not be read, or a rotate that crosses a block boundary and is then multiplied by zero: 0 * x = 0 keeps the oracle
comparison green.  With x = NaN it does not.  So every comparison with the clean launch here is BIT equality (the raw 32-bit words);
only the clean launch itself is compared with the float64 oracle, within the project's TOL = 1e-5 (IC blocks guarded as in
tests/test_parity_gpu.py).  The predictions -- which rows a poisoned bin reaches -- are pinned on the oracle by tests/test_poison.py.

Infinite bins (+inf and inf + inf j): only the confinement is asserted; what the affected rows hold is recorded (printed, and appended
to the file named by GFDM_POISONLOG) -- include/gfdm_hip.h documents it per family."""
import contextlib
import os

import numpy as np
import pytest

import gfdm_ref as R
import poison_cases as P
from burst_receive_cases import CASES as BURST_CASES, make_case as make_burst_case
from conftest import check_err, have_gpu, rel_err

pytestmark = pytest.mark.gpu
TOL = P.TOL


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


def _record(line):
    print(line)
    log = os.environ.get("GFDM_POISONLOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


@contextlib.contextmanager
def _setting(setter, mode):
    """a process-wide creation-time switch (set_ic_matrix_cores / set_dft_matrix_cores), restored afterwards; None: untouched"""
    if mode is None:
        yield
        return
    prev = setter(mode)
    try:
        yield
    finally:
        setter(prev)


@contextlib.contextmanager
def _creating(route):
    """the context in which the handles of a route are created"""
    import gfdm_amd
    r = P.ROUTES[route]
    with contextlib.ExitStack() as es:
        if r.get("generic"):
            es.enter_context(gfdm_amd.generic_family_for_testing())
        es.enter_context(_setting(gfdm_amd.set_ic_matrix_cores, r.get("ic_mx")))
        es.enter_context(_setting(gfdm_amd.set_dft_matrix_cores, r.get("dft_mx")))
        yield


def _case(route):
    r = P.ROUTES[route]
    return P.make_case(*r["shape"], r["B"])


def _receivers(route, smap=None):
    """(Demodulator, AdvancedReceiver with IC_ITER rounds) of a route, kernel_name() asserted: a route cannot silently change"""
    import gfdm_amd
    c = _case(route)
    M, K, L = c["M"], c["K"], c["L"]
    with _creating(route):
        dem = gfdm_amd.Demodulator(M, K, L, c["taps"])
        adv = gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"] if smap is None else smap, P.IC_ITER, R.qpsk_points())
    assert (dem.kernel_name(), adv.kernel_name()) == (P.ROUTES[route]["kernel"],) * 2
    assert adv.decision_rule() == "qpsk" and adv.get_phase_compensation() == 0
    return dem, adv


def _run(rx, mode, x, feq):
    """one launch of `mode` on the (B, N) blocks x; (B, K, M) complex64"""
    dem, adv = rx
    if mode == "fd":
        out = dem.fft_filter_downsample(x) if feq is None else dem.fft_equalize_filter_downsample(x, feq)
    elif mode == "zf":
        out = dem.demodulate(x) if feq is None else dem.demodulate_equalize(x, feq)
    else:
        out = adv.demodulate(x) if feq is None else adv.demodulate_equalize(x, feq)
    assert out.dtype == np.complex64
    return out


def _same_where(a, b, where):
    """bit equality of the complex64 arrays a and b on the elements selected by `where`"""
    w = np.repeat(np.broadcast_to(where, a.shape), 2, axis=-1)
    return np.array_equal(P.bits(a)[w], P.bits(b)[w])


def _first_diff(a, b, where):
    w = np.broadcast_to(where, a.shape) & ((P.bits(a)[..., 0::2] != P.bits(b)[..., 0::2]) | (P.bits(a)[..., 1::2] != P.bits(b)[..., 1::2]))
    return np.argwhere(w)[:6].tolist()


def _block_mask(shape, blocks):
    m = np.zeros(shape, bool)
    m[list(blocks)] = True
    return m


def _check_confined(tag, got, clean, bad_mask, halo=None):
    """(c) + (d): the non-finite elements are exactly bad_mask; everything outside it (and outside `halo`) is bit-equal to the clean launch;
    the halo is finite"""
    halo = np.zeros(got.shape, bool) if halo is None else halo
    bad = ~np.isfinite(got)
    assert np.array_equal(bad, bad_mask), "%s: non-finite mask differs from the prediction at %s" % (tag, np.argwhere(bad != bad_mask)[:6].tolist())
    same = ~bad_mask & ~halo
    assert _same_where(got, clean, same), "%s: unaffected elements changed at %s" % (tag, _first_diff(got, clean, same))


def _anchor(tag, c, mode, clean, ref=None, keep=None):
    """(a): the clean launch against the float64 oracle"""
    ref = c["ref_" + mode] if ref is None else ref
    keep = (c["keep_ic"] if mode == "ic" else np.ones(c["B"], bool)) if keep is None else keep
    assert keep.sum() * 2 >= c["B"], "%s: the decision guard dropped most blocks" % tag
    check_err("poison_clean_" + tag, rel_err(clean.reshape(c["B"], -1)[keep], ref.reshape(c["B"], -1)[keep]), TOL)


# ---------------------------------------------------------------- equaliser bins

@pytest.mark.parametrize("route", sorted(P.ROUTES))
def test_equaliser_bin_stays_in_its_rows_and_block(route):
    """A zero, NaN or infinite f_eq bin in blocks 1 and B - 1: fft_equalize_filter_downsample, demodulate_equalize and
    AdvancedReceiver.demodulate_equalize.  Zero and NaN: the non-finite mask is the oracle's, everything else bit-equal to the clean
    launch (IC: outside the ic_iter halo, which stays finite).  +inf and inf + inf j: everything outside the affected rows is bit-equal;
    what the rows hold is recorded (x conj(e) / |e|^2 gives NaN where numpy's quotient for a real +inf is 0)."""
    c = _case(route)
    B, K, M = c["B"], c["K"], c["M"]
    rx = _receivers(route)
    xe, feq = np.asarray(c["xe"]), np.asarray(c["feq"])
    clean_blocks = _block_mask((B, K, M), P.clean_blocks(c))
    for mode in P.ROUTES[route]["modes"]:
        tag = "%s_%s" % (route, mode)
        clean = _run(rx, mode, xe, feq).reshape(B, K, M)
        _anchor(tag, c, mode, clean)                                                       # (a)
        assert np.isfinite(clean).all()
        assert np.array_equal(P.bits(_run(rx, mode, xe, feq).reshape(B, K, M)), P.bits(clean))      # the launch itself is reproducible
        for name in ("zero", "nan"):
            got = _run(rx, mode, xe, P.poisoned_feq(c, P.BINS[name])).reshape(B, K, M)    # (b)
            assert _same_where(got, clean, clean_blocks), "%s %s: a clean block changed at %s" % (tag, name, _first_diff(got, clean, clean_blocks))  # (c)
            want = ~np.isfinite(P.oracle(c, mode, P.poisoned_feq(c, P.BINS[name])))
            assert np.array_equal(want, P.predicted_mask(c, mode))
            _check_confined("%s %s" % (tag, name), got, clean, want, P.halo_mask(c, mode))                                     # (d)
            assert np.isfinite(got[P.halo_mask(c, mode)]).all()
        for name in ("inf", "infinf"):
            got = _run(rx, mode, xe, P.poisoned_feq(c, P.BINS[name])).reshape(B, K, M)
            assert _same_where(got, clean, clean_blocks), "%s %s: a clean block changed at %s" % (tag, name, _first_diff(got, clean, clean_blocks))
            # (e)  (IC: whatever the affected rows hold -- NaN here, 0-quotient symbols in numpy -- is decided differently from the clean
            # launch, so the ic_iter halo may change as in (d); it must stay finite)
            same = ~P.affected_mask(c) & ~P.halo_mask(c, mode)
            assert _same_where(got, clean, same), "%s %s: unaffected elements changed at %s" % (tag, name, _first_diff(got, clean, same))
            assert np.isfinite(got[~P.affected_mask(c)]).all()
            reach = P.predicted_mask(c, mode)                                              # the elements the bin reaches (fd: column m0 only)
            nf = ~np.isfinite(got)
            rest = P.affected_mask(c) & ~reach
            _record("poison_inf_bin route=%s kernel=%s mode=%s bin=%s: non-finite %d of %d reached elements, %d of %d others of the affected rows"
                    % (route, P.ROUTES[route]["kernel"], mode, name, int(nf[reach].sum()), int(reach.sum()), int(nf[rest].sum()), int(rest.sum())))


# ---------------------------------------------------------------- sample poison

@pytest.mark.parametrize("route", sorted(P.ROUTES))
def test_non_finite_sample_fills_its_block_only(route):
    """a NaN sample in block 1 and an inf sample in block B - 1 of demodulate, demodulate_equalize and AdvancedReceiver.demodulate: the
    poisoned blocks are wholly non-finite, every other block is bit-equal to the clean launch"""
    c = _case(route)
    B, K, M = c["B"], c["K"], c["M"]
    rx = _receivers(route)
    bad = _block_mask((B, K, M), P.poisoned_blocks(c))
    calls = [("ic", "x", None)] if P.ROUTES[route]["modes"] == ("ic",) else [("zf", "x", None), ("zf", "xe", np.asarray(c["feq"])), ("ic", "x", None)]
    for mode, src, feq in calls:
        tag = "%s_%s_%s" % (route, mode, src)
        clean = _run(rx, mode, np.asarray(c[src]), feq).reshape(B, K, M)
        if feq is None:
            ref = P.oracle(c, mode, None, np.asarray(c[src]))
            keep = None
            if mode == "ic":
                _, st = R.advanced_receive(c[src], c["nt"], M, K, c["L"], c["smap"], R.qpsk_points(), P.IC_ITER, kind="qpsk", return_stages=True)
                keep = P.guarded(st, c["smap"], K, M)
            _anchor(tag, c, mode, clean, ref, keep)
        else:
            _anchor(tag, c, mode, clean)
        xp = P.poisoned_samples(c, src)
        got = _run(rx, mode, xp, feq).reshape(B, K, M)
        assert np.array_equal(~np.isfinite(P.oracle(c, mode, feq, xp)), bad)
        _check_confined(tag, got, clean, bad)


# ---------------------------------------------------------------- symbol poison

@pytest.mark.parametrize("route", sorted(r for r in P.ROUTES if P.ROUTES[r]["modes"] == P.ALL))
def test_nan_symbol_fills_its_modulated_block_only(route):
    import gfdm_amd
    c = _case(route)
    B, K, M, N = c["B"], c["K"], c["M"], c["N"]
    with _creating(route):
        mod = gfdm_amd.Modulator(M, K, c["L"], c["taps"])
    assert mod.kernel_name() == P.ROUTES[route]["kernel"]
    clean = mod.modulate(np.asarray(c["sym"])).reshape(B, N)
    check_err("poison_clean_mod_" + route, rel_err(clean, c["x"]), TOL)
    sym = np.array(c["sym"])
    for b in P.poisoned_blocks(c):
        sym[b, (K // 2 + 3) % K * M + M // 2] = complex(P.NAN, P.NAN)
    got = mod.modulate(sym).reshape(B, N)
    _check_confined("mod_" + route, got, clean, _block_mask((B, N), P.poisoned_blocks(c)))


@pytest.mark.parametrize("shape,B,kernel", [((7, 12, 2), 5, "generic_lds"), ((7, 12, 2), 26, "rowlane_jit"), ((9, 64, 2), 11, "rowlane"), ((5, 32, 2), 19, "rowlane")])
def test_nan_symbol_fills_its_transmitted_frame_only(shape, B, kernel):
    """Transmitter.transmit, every port, cyclic prefix / suffix / ramp / preamble as in test_transmitter_generic_family_and_validation: the
    poisoned frames are non-finite behind their preamble, the preamble and every other frame are bit-equal to the clean launch"""
    import gfdm_amd
    M, K, L = shape
    c = P.make_case(M, K, L, B)
    rng = np.random.default_rng(5)
    smap, N = c["smap"], c["N"]
    A, cp, cs, ramp = len(smap), 5, 3, 2
    window = np.concatenate((np.linspace(0.1, 0.9, ramp), np.ones(N + cp + cs - 2 * ramp), np.linspace(0.9, 0.1, ramp))).astype(complex)
    pre = [rng.standard_normal(11) + 1j * rng.standard_normal(11) for _ in range(2)]
    for per_ts in (True, False):
        with (gfdm_amd.generic_family_for_testing() if kernel == "generic_lds" else contextlib.nullcontext()):
            tx = gfdm_amd.Transmitter(M, K, A, cp, cs, ramp, smap, per_ts, L, c["taps"], window, [0, 2], pre)
        assert tx.kernel_name() == kernel
        sym = np.array(R.demap_from_resources(c["sym"], M, K, smap, per_ts))
        clean = tx.transmit(sym)
        sp = sym.copy()
        for b in P.poisoned_blocks(c):
            sp[b, A * M // 2] = complex(P.NAN, 0.0)
        got = tx.transmit(sp)
        bad = _block_mask((B, 11 + cp + N + cs), P.poisoned_blocks(c))
        bad[:, :11] = False                                                                # the preamble
        for port, s in enumerate((0, 2)):
            ref = R.transmit(sym, c["nt"], M, K, L, smap, per_ts, cp, cs, ramp, window, s, pre[port])
            check_err("poison_clean_tx_%s_%d" % (kernel, port), rel_err(clean[port], ref), TOL)
            _check_confined("tx_%s_port%d" % (kernel, port), got[port], clean[port], bad)
        blocks, blocks_clean = tx.modulate(sp), tx.modulate(sym)
        _check_confined("tx_modulate_%s" % kernel, blocks, blocks_clean, _block_mask((B, N), P.poisoned_blocks(c)))


# ---------------------------------------------------------------- junk next to the data

def _estimator_inputs(c, A, rng):
    """known preamble (flat spectrum, two identical halves) and every block's received preamble behind the case's channel"""
    K, B = c["K"], c["B"]
    pre = np.tile(np.fft.ifft(np.exp(2j * np.pi * rng.random(K))) * np.sqrt(K), 2)
    gains = np.exp(0.3j * np.arange(B)) * (1 + 0.02 * np.arange(B))
    rx_pre = np.tile(np.fft.ifft(np.fft.fft(pre[:K]) * np.fft.fft(P.H, K)), 2)[None, :] * gains[:, None]
    return pre, (rx_pre + 1e-3 * (rng.standard_normal((B, 2 * K)) + 1j * rng.standard_normal((B, 2 * K)))).astype(np.complex64)


def _active(K):
    A = 2 * ((3 * K // 4) // 2)
    return A, np.concatenate((np.arange(1, 1 + A // 2), np.arange(K - A // 2, K)))


@pytest.mark.parametrize("route", sorted(P.ROUTES))
def test_junk_around_the_data_is_never_read_or_written(route):
    """Frames [cp | block | cs | 3 spare]: NaN everywhere outside the block gives the bits that zeros there give (with and without a
    subcarrier map, with f_eq and with the fused estimator, whose preambles lie preamble_stride > 2K apart with NaN in the gaps); with a
    truncating noutput_size block b writes out[b * noutput_size : (b + 1) * noutput_size] and nothing else -- the buffer is pre-filled with
    a sentinel, every slot must hold the first noutput_size symbols of the full output, the sentinel behind the last slot must survive"""
    import torch
    import gfdm_amd
    c = _case(route)
    B, K, M, N, L = c["B"], c["K"], c["M"], c["N"], c["L"]
    ic_only = P.ROUTES[route]["modes"] == ("ic",)
    rng = np.random.default_rng(K + M)
    cp, cs = max(1, K // 4), max(1, K // 8)
    F = cp + N + cs + 3
    A, smap = _active(K)
    rx = _receivers(route, smap)
    pre, rx_pre = _estimator_inputs(c, A, rng)
    with _creating(route):
        est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, pre)
    xe, feq = np.asarray(c["xe"]).astype(np.complex64), np.asarray(c["feq"]).astype(np.complex64)
    inside = np.zeros(F, bool)
    inside[cp:cp + N] = True
    frames0 = np.zeros((B, F), np.complex64)
    frames0[:, inside] = xe
    framesn = frames0.copy()
    framesn[:, ~inside] = complex(P.NAN, P.NAN)
    stride = 2 * K + 5
    gaps0 = np.zeros((B, stride), np.complex64)
    gaps0[:, :2 * K] = rx_pre
    gapsn = gaps0.copy()
    gapsn[:, 2 * K:] = complex(P.NAN, P.NAN)
    sentinel = complex(-12345.0, 54321.0)
    ref_ic, st = R.advanced_receive(c["xe"], c["nt"], M, K, L, smap, R.qpsk_points(), P.IC_ITER, f_eq=np.asarray(c["feq"]), kind="qpsk", return_stages=True)
    refs = {"zf": (np.asarray(c["ref_zf"]), np.ones(B, bool)), "ic": (ref_ic, P.guarded(st, smap, K, M))}
    for h, mode in zip(rx, ("zf", "ic")):
        if ic_only and mode != "ic":
            continue
        h.set_channel_estimator(est)
        for use_map in (True, False):
            tag = "%s_%s_%s" % (route, mode, "map" if use_map else "nomap")
            h.configure_frames(F, cp, smap[::-1] if use_map else None, True)
            a, b = h.demodulate_frames(frames0, feq), h.demodulate_frames(framesn, feq)
            ref, keep = refs[mode]
            want = R.demap_from_resources(ref, M, K, smap, True) if use_map else ref
            assert keep.sum() * 2 >= B
            check_err("poison_clean_frames_" + tag, rel_err(a[keep], want[keep]), TOL)
            assert np.isfinite(a).all() and np.array_equal(P.bits(a), P.bits(b)), "%s: junk around the block was read" % tag
            e0 = h.demodulate_estimated(frames0, gaps0, preamble_stride=stride)
            en = h.demodulate_estimated(framesn, gapsn, preamble_stride=stride)
            assert e0.shape == a.shape and np.isfinite(e0).all()
            assert np.array_equal(P.bits(e0), P.bits(en)), "%s: junk around the block or between the preambles was read" % tag
            assert np.array_equal(P.bits(h.demodulate_estimated(frames0, rx_pre)), P.bits(e0))          # packed preambles: the same bits
            if use_map:
                nshort = A * M - 5
                for est_call in (False, True):
                    buf = torch.full((B * nshort + A * M,), sentinel, dtype=torch.complex64, device="cuda:0")
                    out = buf[:B * nshort].view(B, nshort)
                    if est_call:
                        h.demodulate_estimated(torch.tensor(framesn, device="cuda:0"), torch.tensor(gapsn, device="cuda:0"), preamble_stride=stride,
                                               noutput_size=nshort, out=out)
                        full = en
                    else:
                        h.demodulate_frames(torch.tensor(framesn, device="cuda:0"), torch.tensor(feq, device="cuda:0"), noutput_size=nshort, out=out)
                        full = b
                    torch.cuda.synchronize()
                    res = buf.cpu().numpy()
                    assert np.array_equal(P.bits(res[:B * nshort].reshape(B, nshort)), P.bits(full[:, :nshort])), "%s: a truncated slot differs" % tag
                    assert np.all(res[B * nshort:] == np.complex64(sentinel)), "%s: written behind noutput_size" % tag
        h.set_channel_estimator(None)


# ---------------------------------------------------------------- fused estimator

@pytest.mark.parametrize("M,K,L,A,B,generic", [(9, 64, 2, 52, 11, False), (5, 32, 2, 24, 19, False), (7, 12, 2, 8, 5, True)])
def test_zero_or_nan_preamble_stays_in_its_block(M, K, L, A, B, generic):
    """demodulate_estimated with an all-zero received preamble in block 1 (the estimate is 0: every bin divides by zero) and one NaN
    preamble sample in block B - 1: those blocks are wholly non-finite, the others bit-equal to the clean launch.  Stand-alone
    estimate_frame: the zero preamble yields the exact zeros the oracle yields, the NaN sample a wholly non-finite estimate."""
    import gfdm_amd
    c = P.make_case(M, K, L, B)
    N = c["N"]
    rng = np.random.default_rng(M * K + A)
    smap = np.concatenate((np.arange(1, 1 + A // 2), np.arange(K - A // 2, K)))
    pre, rx_pre = _estimator_inputs(c, A, rng)
    kernel = "generic_lds" if generic else "rowlane"
    with (gfdm_amd.generic_family_for_testing() if generic else contextlib.nullcontext()):
        est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, pre)
        dem = gfdm_amd.Demodulator(M, K, L, c["taps"])
        adv = gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], smap, P.IC_ITER, R.qpsk_points())
    assert (est.kernel_name(), dem.kernel_name(), adv.kernel_name()) == (kernel,) * 3
    bad_pre = rx_pre.copy()
    bad_pre[1] = 0
    bad_pre[B - 1, K + 3] = complex(P.NAN, 0.0)
    bad = _block_mask((B, N), (1, B - 1))
    # stand-alone estimator
    feq = R.estimate_frame(rx_pre, pre.astype(np.complex64), M, K, A, True)
    e_clean, e_bad = est.estimate_frame(rx_pre), est.estimate_frame(bad_pre)
    check_err("poison_clean_estimate_%d_%d" % (M, K), rel_err(e_clean, feq), TOL)
    assert np.all(R.estimate_frame(bad_pre[1], pre.astype(np.complex64), M, K, A, True) == 0)
    assert np.all(e_bad[1] == 0)                                                            # exact zeros
    _check_confined("estimate_frame_%d_%d" % (M, K), e_bad, e_clean, _block_mask((B, N), (B - 1,)), halo=_block_mask((B, N), (1,)))
    # fused in front of both receivers, plain blocks and demapped frames
    xe = np.asarray(c["xe"])
    ref_ic, st = R.advanced_receive(xe, c["nt"], M, K, L, smap, R.qpsk_points(), P.IC_ITER, f_eq=feq, kind="qpsk", return_stages=True)
    keep = P.guarded(st, smap, K, M)
    assert keep.sum() * 2 >= B
    for rx, ref, kp in ((dem, R.demodulate(xe, c["nt"], M, K, L, feq), np.ones(B, bool)), (adv, ref_ic, keep)):
        rx.set_channel_estimator(est)
        clean = rx.demodulate_estimated(xe, rx_pre)
        check_err("poison_clean_estimated_%d_%d" % (M, K), rel_err(clean[kp], ref[kp]), TOL)
        _check_confined("estimated_%d_%d" % (M, K), rx.demodulate_estimated(xe, bad_pre), clean, bad)
        rx.configure_frames(N, 0, smap, True)
        clean = rx.demodulate_estimated(xe, rx_pre)
        check_err("poison_clean_estimated_demap_%d_%d" % (M, K), rel_err(clean[kp], R.demap_from_resources(ref, M, K, smap, True)[kp]), TOL)
        _check_confined("estimated_demap_%d_%d" % (M, K), rx.demodulate_estimated(xe, bad_pre), clean, _block_mask(clean.shape, (1, B - 1)))


# ---------------------------------------------------------------- bursts

BURST_KERNEL = {"rowlane_7": ("rowlane",), "rowlane_jit": ("rowlane_jit",), "generic_127": ("generic_lds", "generic_rader")}
BACKOFF = 17


@pytest.mark.parametrize("name", sorted(BURST_KERNEL))
def test_bursts_read_their_windows_only(name):
    """demodulate_bursts on a complex64 capture, backoff 17.  By the contract in include/gfdm_hip.h burst b reads s[off_b - backoff + n] for
    n in [cp_len, cp_len + block_size) and n in [preamble_offset, preamble_offset + 2 fft_len) and nothing else: NaN in every other sample
    of the capture leaves the output bit-equal; NaN inside burst 1's block window, or inside its preamble window, makes burst 1 non-finite
    and leaves the others bit-equal; bursts at or behind `count` yield exact zeros although their offsets point at NaN samples."""
    import torch
    import gfdm_amd
    M, K, L, A, nb, seed = BURST_CASES[name]
    c = make_burst_case(M, K, L, A, nb, seed)
    N, F, po = c["N"], c["F"], c["pre_off"]
    cpl = po + 2 * K + c["cp"]
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    rxs = (gfdm_amd.Demodulator(M, K, L, c["taps"]), gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], P.IC_ITER, R.qpsk_points()))
    t = lambda a, dtype=None: torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")
    s = np.array(c["stream"])
    base = np.asarray(c["starts"])                                   # off_b - backoff
    offs = t(base + BACKOFF)
    rot = t(c["sc_rot"])
    assert base[0] >= 0 and base[-1] + F <= s.size                   # every window lies inside the capture
    read = np.zeros(s.size, bool)
    blk, pre = [], []
    for b in range(nb):
        blk.append(slice(base[b] + cpl, base[b] + cpl + N))
        pre.append(slice(base[b] + po, base[b] + po + 2 * K))
        read[blk[b]] = read[pre[b]] = True
    assert (~read).sum() > nb * c["cp"]                              # the prefixes and the gaps between the bursts are junk
    nan = np.complex64(complex(P.NAN, P.NAN))
    s_junk = np.where(read, s, nan)
    s_blk, s_pre = s.copy(), s.copy()
    s_blk[blk[1].start + N // 2] = nan
    s_pre[pre[1].start + K + 1] = nan
    live = nb - 2 if nb > 3 else nb - 1
    s_dead = s.copy()
    for b in range(live, nb):
        s_dead[base[b]:base[b] + F] = nan
    for rx in rxs:
        assert rx.kernel_name() in BURST_KERNEL[name]
        rx.configure_frames(F, cpl, c["smap"], True)
        rx.set_channel_estimator(est)
        run = lambda cap, **kw: rx.demodulate_bursts(t(cap), offs, rot, backoff=BACKOFF, preamble_offset=po, **kw).cpu().numpy()
        clean = run(s)
        assert clean.shape == (nb, A * M) and np.isfinite(clean).all()
        if isinstance(rx, gfdm_amd.AdvancedReceiver):                # the anchor: the transmitted symbols are recovered (tests/test_burst_receive_gpu.py has the yardsticks)
            assert np.array_equal(clean.real > 0, c["sym"].real > 0) and np.array_equal(clean.imag > 0, c["sym"].imag > 0)
        assert np.array_equal(P.bits(run(s_junk)), P.bits(clean)), "%s: a sample outside the read windows was read" % name
        for tag, cap in (("block", s_blk), ("preamble", s_pre)):
            _check_confined("bursts_%s_%s" % (name, tag), run(cap), clean, _block_mask(clean.shape, (1,)))
        got = run(s_dead, count=t([live], torch.int64))
        assert _same_where(got, clean, _block_mask(clean.shape, range(live)))
        assert not P.bits(got[live:]).any(), "%s: a burst at or behind count is not exact zeros" % name
