"""The predictions of tests/poison_cases.py, pinned on the float64 oracle alone (no GPU): which elements a zero, NaN or infinite
equaliser bin, a non-finite sample or a NaN symbol of one block makes non-finite, and that everything else -- every other block, and
inside the block every row out of the bin's reach -- is bit-identical to the clean result.  tests/test_poison_gpu.py asserts the same
of the HIP kernels."""
import numpy as np
import pytest

import gfdm_ref as R
import poison_cases as P

B = 4


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_affected_rows_by_definition():
    """the set is { k : (k + i - L/2) mod K = j0 for a part i }, written out; with j0 = K - 1 it wraps"""
    for K, L in ((32, 2), (128, 4), (12, 2), (40, 5), (16, 2)):
        for j0 in (0, 3, K - 1):
            want = sorted({k for k in range(K) for i in range(L) if (k + i + K - L // 2) % K == j0})
            assert P.affected_rows(K, L, j0) == want and len(want) == L
        rows = P.affected_rows(K, L, K - 1)
        assert 0 in rows and K - 1 in rows                                  # wraps inside the block
        dist = lambda k: min(min((k - r) % K, (r - k) % K) for r in rows)   # cyclic distance from the set
        assert P.halo_rows(K, L, K - 1, 2) == [k for k in range(K) if 1 <= dist(k) <= 2]


@pytest.mark.parametrize("M,K,L", P.CPU_SHAPES)
@pytest.mark.parametrize("bin_name", ["zero", "nan", "infinf"])
def test_equaliser_bin_reaches_exactly_the_affected_rows(M, K, L, bin_name):
    c = P.make_case(M, K, L, B)
    assert np.all(c["nt"] != 0)                                             # a zero tap would take a row out of the set
    feq = P.poisoned_feq(c, P.BINS[bin_name])
    clean = P.clean_blocks(c)
    assert clean == [0, 2] and P.poisoned_blocks(c) == [1, 3]
    for mode, ref in (("fd", c["ref_fd"]), ("zf", c["ref_zf"]), ("ic", c["ref_ic"])):
        got = P.oracle(c, mode, feq)
        ref = ref.reshape(B, K, M)
        bad = ~np.isfinite(got)
        # demodulate: the affected rows in full; fft_equalize_filter_downsample: their column m0 only; advanced_receive: the rows again,
        # since a decision taken on NaN is a finite constellation point and S itself stays non-finite
        assert np.array_equal(bad, P.predicted_mask(c, mode)), (mode, np.argwhere(bad != P.predicted_mask(c, mode))[:5])
        assert bad.any() and not bad[clean].any()
        assert _same(got[clean], ref[clean])                                # cross-block isolation
        same = ~bad & ~P.halo_mask(c, mode)
        assert _same(got[same], ref[same])                                  # rows farther than ic_iter from the set are unchanged
    # the affected set of this shape, spelled out for block 1
    rows = P.affected_rows(K, L, K - 1)
    zf = P.oracle(c, "zf", feq)
    assert not np.isfinite(zf[1][rows]).any() and np.isfinite(np.delete(zf[1], rows, axis=0)).all()


@pytest.mark.parametrize("M,K,L", P.CPU_SHAPES)
def test_real_infinite_bin_is_a_zero_quotient_in_numpy(M, K, L):
    """x / (inf + 0j) = 0 in numpy: every mode stays finite (the HIP kernels' x conj(e) / |e|^2 forms give NaN instead: DEVIATION)"""
    c = P.make_case(M, K, L, B)
    feq = P.poisoned_feq(c, P.BINS["inf"])
    for mode, ref in (("fd", c["ref_fd"]), ("zf", c["ref_zf"]), ("ic", c["ref_ic"])):
        got = P.oracle(c, mode, feq)
        ref = ref.reshape(B, K, M)
        assert np.isfinite(got).all()
        clean = P.clean_blocks(c)
        assert _same(got[clean], ref[clean])
        same = ~P.affected_mask(c) & ~P.halo_mask(c, mode)
        assert _same(got[same], ref[same])


@pytest.mark.parametrize("M,K,L", P.CPU_SHAPES)
def test_sample_and_symbol_poison_fill_their_block_only(M, K, L):
    c = P.make_case(M, K, L, B)
    clean, bad = P.clean_blocks(c), P.poisoned_blocks(c)
    # one NaN (block 1) or inf (block B - 1) sample: the whole block of every receiver
    for src, feq in (("xe", np.asarray(c["feq"])), ("x", None)):
        xp = P.poisoned_samples(c, src)
        for mode in P.ALL:
            got, ref = P.oracle(c, mode, feq, xp), P.oracle(c, mode, feq, c[src])
            assert not np.isfinite(got[bad]).any() and _same(got[clean], ref[clean])
    # one NaN symbol: the whole block of the modulator and of the transmitter's frame behind the preamble
    sym = np.array(c["sym"])
    for b in bad:
        sym[b, (K // 2 + 3) % K * M + M // 2] = complex(P.NAN, P.NAN)
    with np.errstate(all="ignore"):
        got, ref = R.modulate(sym, c["nt"], M, K, L), R.modulate(c["sym"], c["nt"], M, K, L)
    assert not np.isfinite(got[bad]).any() and _same(got[clean], ref[clean])
    smap = c["smap"]
    A, cp, cs, ramp = len(smap), 5, 3, 2
    window = np.concatenate((np.linspace(0.1, 0.9, ramp), np.ones(c["N"] + cp + cs - 2 * ramp), np.linspace(0.9, 0.1, ramp))).astype(complex)
    pre = np.exp(0.7j * np.arange(11))
    s = np.array(R.demap_from_resources(c["sym"], M, K, smap, True))
    sp = s.copy()
    for b in bad:
        sp[b, A * M // 2] = complex(P.NAN, 0.0)
    for shift in (0, 2):
        with np.errstate(all="ignore"):
            got = R.transmit(sp, c["nt"], M, K, L, smap, True, cp, cs, ramp, window, shift, pre)
        ref = R.transmit(s, c["nt"], M, K, L, smap, True, cp, cs, ramp, window, shift, pre)
        assert not np.isfinite(got[bad][:, len(pre):]).any()
        assert _same(got[bad][:, :len(pre)], ref[bad][:, :len(pre)]) and _same(got[clean], ref[clean])
