"""GPU tests of the shapes of tests/codelet_cases.py: subcarrier pass radices, timeslot codelets, overlaps and eligibility edges of the
run-time row-lane family that no other test instantiates, by the budget method of tests/test_accuracy_gpu.py (its helpers, imported).

  budget  every shape that jit_eligible() accepts must report rowlane_jit, and every figure (l2, peak, pos) of modulate, fd, fdeq,
          demodulate, demodulate_equalize and to_td, with RRC and with `rand` taps, stays inside accuracy_cases.bounds of the C oracle's
          figure on the same inputs.  The two overlap shapes (L = 5, L = 7) also run the advanced receiver: 2 rounds, MF and ZF input,
          guarded blocks.  Tags acc_codelet_<shape>_<taps>_<entry>_<figure> (GFDM_ERRLOG; profiles/r03/codelet_budget_table.md).
  edges   one step outside each rule of jit_eligible() the handles must report generic_lds (a fallback, not a failed launch), and
          are held to TOL against the float64 oracle (tags accouter_codelet_...); the inner side is part of the budget test.

The cost of this module is hiprtc, not the GPU: the shapes and their compile times are in profiles/r03/codelet_budget_table.md."""
import pytest

import accuracy_cases as A
import codelet_cases as C
from test_accuracy_gpu import _budget, _Findings, _handles, _require_gpu  # noqa: F401  (the fixture applies to this module as well)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,kind", C.CASES)
def test_codelets_within_the_float32_budget(shape, kind):
    r = C.ROUTES[shape]
    c = C.make_case(shape, kind)
    ref = C.reference_figures(shape, kind)
    h = _handles(shape, c, routes=C.ROUTES)
    found = _Findings()
    _budget(found, "codelet_" + shape, kind, c, ref, h, r["entries"], r["margin"])
    found.done()


@pytest.mark.parametrize("inner,outer,kind", C.EDGE_CASES)
def test_codelets_one_step_outside_an_eligibility_rule_falls_back_to_the_generic_family(inner, outer, kind):
    """the outer shape of every edge: generic_lds, inside TOL on every entry point; the inner one reports rowlane_jit"""
    import gfdm_amd
    (M, K, L), c = C.ROUTES[inner]["shape"], C.make_case(inner, kind)
    assert gfdm_amd.Demodulator(M, K, L, c["taps"]).kernel_name() == C.ROUTES[inner]["kernel"] == "rowlane_jit"
    c = C.make_case(outer, kind)
    h = _handles(outer, c, routes=C.ROUTES)
    assert C.ROUTES[outer]["kernel"] == "generic_lds"
    found = _Findings()
    for e in C.ROUTES[outer]["entries"]:
        figs, got, want = h.figures(e, c)
        found.check("accouter_codelet_%s_%s_%s_l2" % (outer, kind, e), figs["l2"], A.TOL, A.where(got, want))
    found.done()
