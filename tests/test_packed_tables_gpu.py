"""GPU tests of every route that fetches the per-lane tables of the row-lane kernels (gfdm_rowlane_impl.h, "Per-lane tables in 16-byte
pairs"): the twiddles W_N^{q m} and the subcarrier-FFT roots, as [m][K] planes or pair-packed, whichever the build under test reads.

  shapes    (K, M, L) = (64, 9, 2), (128, 15, 4), (256, 31, 2), (32, 9, 2), (4, 16, 2), (96, 25, 2): every pass plan of the compiled shapes,
            odd and even M - 1, several blocks per wavefront, several wavefronts per block; and (16, 6, 2) instantiated at run time
  batches   1 block, and the smallest batch that puts a block into a second workgroup, whose other lane groups are then invalid:
            5 at K = 64 (four blocks per workgroup), 3 at K = 128 / 256 / 96, 9 at K = 32, 65 at K = 4, 17 at K = 16
  kinds     modulate; MF and ZF demodulate; fft_filter_downsample; MF + 2 and ZF + 2 cancellation rounds on the vector ALU, and on the
            matrix cores where that form is the default (K = 128, M = 15); the preamble-estimated receiver and demodulate_bursts, plain
            and with 2 rounds
  offsets   K = 64: modulate and demodulate with the input and output pointers 8 bytes off a 16-byte boundary (the 8-byte sample route)
  expected  the float64 oracle within TOL = 1e-5 (worst block, relative L2), the bound of tests/test_parity_gpu.py

The oracle's results are computed once per shape for the larger batch; the one-block case takes its first block.  Precondition of the
cancellation cases, asserted on the oracle: every decided component at least DECISION_GUARD away from zero, so no decision can flip."""
import functools

import numpy as np
import pytest

import gfdm_ref as R
from burst_receive_cases import MARGIN, make_case, restatement, virtual_bursts
from conftest import check_err, have_gpu, rel_err
from gfdm_amd.filters import get_frequency_domain_filter

pytestmark = pytest.mark.gpu

TOL = 1e-5
DECISION_GUARD = 1e-4
ALPHA = 0.1
# (K, M, L): the batch beyond one block, active subcarriers of the estimated kinds
SHAPES = {(64, 9, 2): (5, 52), (128, 15, 4): (3, 110), (256, 31, 2): (3, 220), (32, 9, 2): (9, 24), (4, 16, 2): (65, 2), (96, 25, 2): (3, 80)}
JIT_SHAPE, JIT_BATCH = (16, 6, 2), 17
MFMA_DEFAULT = {(128, 15, 4)}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@functools.lru_cache(maxsize=None)
def plain_case(K, M, L, B):
    """inputs (complex64) and float64 oracle results of the plain-block kinds for B blocks; never modified"""
    rng = np.random.default_rng(K * 1000 + M)
    N = M * K
    taps = get_frequency_domain_filter("rrc", ALPHA, M, K, L)
    nt = R.normalize_taps(taps, M)
    sym = (((1 - 2 * rng.integers(0, 2, (B, N))) + 1j * (1 - 2 * rng.integers(0, 2, (B, N)))) / np.sqrt(2)).astype(np.complex64)
    x = R.modulate(sym, nt, M, K, L).astype(np.complex64)
    feq = (np.fft.fft(np.array([1, .4 - .2j, .15j, .05]), N)[None, :] * np.exp(0.3j * np.arange(B))[:, None]).astype(np.complex64)
    xe = np.fft.ifft(np.fft.fft(x.astype(np.complex128), axis=-1) * feq, axis=-1).astype(np.complex64)
    smap = np.arange(K)
    ic_mf, st_mf = R.advanced_receive(x, nt, M, K, L, smap, R.qpsk_points(), 2, kind="qpsk", return_stages=True)
    ic_zf, st_zf = R.advanced_receive(xe, nt, M, K, L, smap, R.qpsk_points(), 2, f_eq=feq, kind="qpsk", return_stages=True)
    margin = float(min(np.min(st_mf["dec_margin"]), np.min(st_zf["dec_margin"])))
    return dict(taps=taps, sym=sym, x=x, xe=xe, feq=feq, margin=margin,
                ref=dict(modulate=R.modulate(sym, nt, M, K, L), demod_mf=R.demodulate(x, nt, M, K, L), demod_zf=R.demodulate(xe, nt, M, K, L, f_eq=feq),
                         fd=R.fft_filter_downsample(x, nt, M, K, L), ic_mf=ic_mf, ic_zf=ic_zf))


def _plain_handles(K, M, L, taps, want):
    """modulator, demodulator, IC receiver(s) with 2 rounds: [(name, handle)] -- on the vector ALU, and on the matrix cores where they are the default"""
    import gfdm_amd
    mod, dem = gfdm_amd.Modulator(M, K, L, taps), gfdm_amd.Demodulator(M, K, L, taps)
    prev = gfdm_amd.set_ic_matrix_cores(0)
    try:
        advs = [("valu", gfdm_amd.AdvancedReceiver(M, K, L, taps, np.arange(K), 2, R.qpsk_points()))]
    finally:
        gfdm_amd.set_ic_matrix_cores(prev)
    if (K, M, L) in MFMA_DEFAULT:
        assert prev == 1
        advs.append(("mfma", gfdm_amd.AdvancedReceiver(M, K, L, taps, np.arange(K), 2, R.qpsk_points())))
    assert {h.kernel_name() for h in [mod, dem] + [a for _, a in advs]} == {want}
    return mod, dem, advs


def _check_plain(K, M, L, batches, want):
    c = plain_case(K, M, L, max(batches))
    assert c["margin"] > DECISION_GUARD, "precondition: decision margin %.2e" % c["margin"]
    mod, dem, advs = _plain_handles(K, M, L, c["taps"], want)
    for B in batches:
        got = {"modulate": mod.modulate(c["sym"][:B]), "demod_mf": dem.demodulate(c["x"][:B]),
               "demod_zf": dem.demodulate_equalize(c["xe"][:B], c["feq"][:B]), "fd": dem.fft_filter_downsample(c["x"][:B])}
        for name, adv in advs:
            got["ic_mf_" + name] = adv.demodulate(c["x"][:B])
            got["ic_zf_" + name] = adv.demodulate_equalize(c["xe"][:B], c["feq"][:B])
        for kind, res in sorted(got.items()):
            ref = c["ref"][kind[:5] if kind.startswith("ic_") else kind][:B]
            err = rel_err(np.asarray(res).reshape(B, -1), ref)
            print("K=%d M=%d L=%d B=%d %-12s %.2e" % (K, M, L, B, kind, err))
            check_err("packed_%d_%d_%d_%s_%d" % (K, M, L, kind, B), err, TOL)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_plain_block_kinds_against_the_oracle(shape):
    K, M, L = shape
    _check_plain(K, M, L, (1, SHAPES[shape][0]), "rowlane")


def test_run_time_instantiated_shape_against_the_oracle():
    K, M, L = JIT_SHAPE
    _check_plain(K, M, L, (1, JIT_BATCH), "rowlane_jit")


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_estimated_receivers_against_the_oracle(shape):
    """demodulate_estimated (preamble columns ride through the subcarrier FFT) and demodulate_bursts (the gather-load kernels), plain and
    with 2 cancellation rounds, against the float64 restatement of tests/burst_receive_cases.py on the same virtual bursts"""
    import torch
    import gfdm_amd
    K, M, L = shape
    nb, A = SHAPES[shape]
    c = make_case(M, K, L, A, nb, 0)
    F, po = c["F"], c["pre_off"]
    e = virtual_bursts(c["stream"], c["starts"], c["sc_rot"], 0, F)
    est = gfdm_amd.ChannelEstimator(M, K, A, True, 1, c["preamble"])
    rxs = [("dem", None, gfdm_amd.Demodulator(M, K, L, c["taps"]))]
    prev = gfdm_amd.set_ic_matrix_cores(0)
    try:
        rxs.append(("ic_valu", 2, gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())))
    finally:
        gfdm_amd.set_ic_matrix_cores(prev)
    if shape in MFMA_DEFAULT:
        rxs.append(("ic_mfma", 2, gfdm_amd.AdvancedReceiver(M, K, L, c["taps"], c["smap"], 2, R.qpsk_points())))
    dev = torch.device("cuda:0")
    ds, offs, rot = (torch.tensor(c[k], device=dev) for k in ("stream", "starts", "sc_rot"))
    bursts = torch.tensor(e.astype(np.complex64), device=dev)
    for name, it, rx in rxs:
        assert rx.kernel_name() == "rowlane"
        rx.configure_frames(F, po + 2 * K + c["cp"], c["smap"], True)
        rx.set_channel_estimator(est)
        ref, margin = restatement(c, e, it)
        assert margin > MARGIN
        for B in (1, nb):
            est_out = rx.demodulate_estimated(bursts[:B].contiguous(), bursts[:B].contiguous().view(-1)[po:], preamble_stride=F)
            bur_out = rx.demodulate_bursts(ds, offs[:B].contiguous(), rot[:B].contiguous(), preamble_offset=po)
            torch.cuda.synchronize()
            for kind, res in (("estimated", est_out), ("bursts", bur_out)):
                err = rel_err(res.cpu().numpy(), ref[:B])
                print("K=%d M=%d L=%d B=%d %-9s %-7s %.2e" % (K, M, L, B, kind, name, err))
                check_err("packed_%d_%d_%d_%s_%s_%d" % (K, M, L, kind, name, B), err, TOL)


def test_pointers_eight_bytes_off_run_the_narrow_sample_route():
    """K = 64: input and output one complex sample behind a 16-byte boundary -- the 8-byte sample accesses next to the 16-byte table loads"""
    import torch
    import gfdm_amd
    K, M, L = 64, 9, 2
    B, N = SHAPES[(K, M, L)][0], M * K
    c = plain_case(K, M, L, B)
    mod, dem = gfdm_amd.Modulator(M, K, L, c["taps"]), gfdm_amd.Demodulator(M, K, L, c["taps"])
    dev = torch.device("cuda:0")
    for kind, h, src in (("modulate", mod.modulate, c["sym"]), ("demod_mf", dem.demodulate, c["x"])):
        ibuf = torch.zeros(B * N + 2, dtype=torch.complex64, device=dev)
        obuf = torch.full((B * N + 2,), float("nan"), dtype=torch.complex64, device=dev)
        x, out = ibuf[1:1 + B * N], obuf[1:1 + B * N]
        assert x.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
        x.copy_(torch.tensor(src, device=dev).reshape(-1))
        h(x, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(obuf[0])) and bool(torch.isnan(obuf[-1])), "the call wrote outside its output"
        err = rel_err(out.cpu().numpy().reshape(B, -1), c["ref"][kind])
        print("K=64 M=9 B=%d %s 8 bytes off: %.2e" % (B, kind, err))
        check_err("packed_offset_%s" % kind, err, TOL)
