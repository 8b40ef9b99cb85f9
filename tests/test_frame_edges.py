"""CPU side of the frame-edge tests (tests/frame_edge_cases.py): the three expectations of every transmitter case agree -- the float64
oracle, the plain-C float32 oracle and the frame written out by definition --, the table reaches every edge it is there for, the
receiver expectations have the sizes the library documents for its frame calls, and the decision guard keeps enough blocks of every
interference-cancellation case for the GPU comparison to mean something."""
import numpy as np
import pytest

import c_oracle
import frame_edge_cases as E
import gfdm_ref as R
import poison_cases as P
from conftest import rel_err

TOL = E.TOL
ROUTE_SHAPES = sorted({(P.ROUTES[r]["shape"], E.blocks(r)) for r in E.RX_ROUTES})


@pytest.mark.parametrize("shape", E.CPU_SHAPES)
@pytest.mark.parametrize("case", E.tx_cases(), ids=E.case_id)
def test_transmitter_expectations_agree(shape, case):
    M, K, L = shape
    c = E.tx_case(M, K, L, 2, case)
    N, ramp, w = c["N"], c["ramp"], np.asarray(c["window"])
    co = c_oracle.COracleTx(M, K, c["A"], c["cp"], c["cs"], ramp, c["smap"], c["per_ts"], L, c["taps"], w, c["shifts"],
                            np.stack(c["preambles"]).reshape(len(c["shifts"]), c["plen"]))
    assert co.n_out == c["F"] and co.n_in == c["A"] * M
    front, back = w[:ramp], w[len(w) - ramp:]
    for port, s in enumerate(c["shifts"]):
        ref = c["frames"][port]
        assert ref.shape == (2, c["F"])
        by_def = E.frames_by_definition(c["block"], c["cp"], c["cs"], ramp, front, back, s, c["preambles"][port])
        assert by_def.shape == ref.shape and rel_err(by_def, ref) < 1e-12
        got = co.work(np.asarray(c["sym"]), port)
        assert got.shape == ref.shape and rel_err(got, ref) < TOL
        seg = E.segments(c, port)
        assert seg["suffix"].stop == c["F"] and sum(v.stop - v.start for v in seg.values()) == c["window_len"]


def test_the_table_reaches_every_edge():
    """computed from the table itself: at least one case for every edge the tests are there for"""
    hit = {}
    for M, K, L in E.CPU_SHAPES:
        for case in E.tx_cases():
            for name, ok in E.tx_predicates(E.tx_case(M, K, L, 2, case)).items():
                hit[name] = hit.get(name, False) or bool(ok)
        for mname in E.MAPS:
            d = dict(M=M, K=K, N=M * K, smap=E.smap_of(mname, K), A=len(E.smap_of(mname, K)))
            for case in E.rx_cases(mname):
                for name, ok in E.rx_predicates(d, case).items():
                    hit["rx " + name] = hit.get("rx " + name, False) or bool(ok)
    want = ["scs == 0", "scp == N", "scs == N", "2*ramp == window_len", "ramp > cp + shift", "ramp > cs - shift", "plen == 0", "F odd",
            "nports == 8", "cp == 0 and cs == 0", "A == 1", "A == K", "0 in smap and K-1 in smap", "nin == 1",
            "rx frame_len == cp + N", "rx cp == 0", "rx cp > N", "rx noutput_size == 1", "rx A == 1", "rx A == K", "rx 0 in smap and K-1 in smap"]
    assert [name for name in want if not hit.get(name)] == []
    # ports8: shift == cs on the last port, and an odd frame length wherever the block length is even
    for M, K, L in E.CPU_SHAPES:
        c = E.tx_case(M, K, L, 2, ("ports8", "all", True, "full"))
        assert c["shifts"][-1] == c["cs"] and (c["F"] % 2 == 1) == (c["N"] % 2 == 0)
    # blocks per launch: a full first workgroup and a last one with a single block
    assert {r: E.bpw(r) for r in ("rowlane_2_per_wave", "rowlane_wave", "rowlane_multiwave", "rowlane_jit", "generic_lds_12", "rader")} == \
        {"rowlane_2_per_wave": 8, "rowlane_wave": 4, "rowlane_multiwave": 1, "rowlane_jit": 21, "generic_lds_12": 1, "rader": 1}
    assert E.blocks("generic_global") == 3
    assert set(E.TX_ROUTES) | {"rowlane_2_per_wave_ic_mx", "rowlane_wave_ic_mx"} == set(E.RX_ROUTES)


@pytest.mark.parametrize("shape,B", ROUTE_SHAPES)
@pytest.mark.parametrize("mname", E.MAPS)
def test_receiver_expectations_and_guard(shape, B, mname):
    """frames calls read frame_len samples and write noutput_size symbols per frame (all active symbols by default, the whole block without a
    map): the demapped oracle results have exactly those sizes; the decision guard keeps at least half of the blocks"""
    M, K, L = shape
    d = E.rx_data(M, K, L, B, mname)
    N, A = d["N"], d["A"]
    assert np.asarray(d["keep_ic"]).sum() * 2 >= B
    for case in E.rx_cases(mname):
        cp, frame_len = E.layout(case[0], N)
        assert 0 <= cp and cp + N <= frame_len
        n_out = N if not case[1] else E.nout_of(case[3], A, M)[1]
        assert 1 <= n_out <= (A * M if case[1] else N)
        for ref in (d["ref_zf"], d["ref_ic"]):
            assert E.rx_expected(d, np.asarray(ref), case).shape == (B, n_out)
    if mname == "tq":
        e = E.est_data(M, K, L, B)
        assert np.asarray(e["keep_ic"]).sum() * 2 >= B
        assert e["want_zf"].shape == e["want_ic"].shape == (B, e["A"] * M)
        rng = np.random.default_rng(0)
        for name in E.EST_LAYOUTS:
            frames, cp, frame_len, pre_at, stride = E.est_frames(e, name, rng)
            assert frames.shape == (B, frame_len) and np.array_equal(frames[:, cp:cp + N], np.asarray(e["xe"]).astype(np.complex64))
            if pre_at is not None:
                flat = frames.reshape(-1)
                assert all(np.array_equal(flat[pre_at + b * stride:pre_at + b * stride + 2 * K], e["rx_pre"][b]) for b in range(B))
                assert name != "pre_back" or pre_at + (B - 1) * stride + 2 * K == flat.size      # the last preamble ends the buffer
