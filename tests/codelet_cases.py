"""Shapes of the run-time row-lane family that instantiate what no other test does (tests/test_codelets.py on the CPU: the coverage
assertion against the plan table printed from csrc/gfdm_rowgeom.h; tests/test_codelets_gpu.py on the GPU: the budget method of
tests/test_accuracy_gpu.py on every shape).

  radix     every subcarrier pass radix 2 .. 32 that the other row-lane shapes of the suite leave out, the radices 18 .. 32 in the last-pass
            position, and a three-pass plan with factor limit 32.  The plans named in the comments are asserted against the table.
  timeslot  M = 14, 24, 32, 36, 43, 45, 47, 48 end to end (registers, tile stride, the compiler's device code; the complete check of the
            timeslot codelets is the host run of tests/test_codelets.py).  Each M rides on a K of the radix list, as large an M as the LDS
            rule allows there; 36 and 48 are the inner sides of two eligibility edges.
  overlap   5 and 7 on rowlane_jit, with an AdvancedReceiver (2 rounds, guarded blocks).
  edge      both sides of every rule of jit_eligible(): the inner shape runs rowlane_jit and is held to the budget, the outer one
            generic_lds and is held to TOL.

Blocks follow accuracy_cases._blocks: 67 where N <= 1024, 29 above, 4 at K = 1024; the last workgroup is part-filled."""
import functools

import accuracy_cases as A

RX = ("modulate", "fd", "fdeq", "demodulate", "demodulate_equalize", "to_td")

# (M, K, L): the plan of K, passes in the order they run (asserted against the table of csrc/gfdm_rowgeom.h)
RADIX = {
    (24, 88, 2): "8x11",
    (3, 63, 5): "7x9",              # overlap 5
    (47, 182, 2): "13x14",
    (43, 306, 2): "17x18",
    (45, 380, 2): "19x20",
    (3, 651, 2): "21x31",
    (32, 506, 2): "22x23",
    (3, 696, 2): "24x29",
    (4, 775, 2): "25x31",
    (3, 806, 2): "26x31",
    (4, 837, 2): "27x31",
    (3, 812, 2): "28x29",
    (4, 870, 2): "29x30",
    (14, 992, 2): "31x32",
    (4, 612, 7): "2x17x18",         # three passes, factor limit 32; overlap 7
    # the radices 19, 21, 22 and 24 .. 28 in the last-pass position (the last pass takes the LARGEST divisor <= 32: behind 17 they are it)
    (3, 323, 2): "17x19",
    (3, 357, 2): "17x21",
    (3, 374, 2): "17x22",
    (3, 408, 2): "17x24",
    (3, 425, 2): "17x25",
    (3, 442, 2): "17x26",
    (3, 459, 2): "17x27",
    (3, 476, 2): "17x28",
}
TIMESLOTS = (14, 24, 32, 36, 43, 45, 47, 48)
OVERLAP_IC = ((3, 63, 5), (4, 612, 7))
# (inner, outer): rowlane_jit on the inner side, generic_lds on the outer
EDGES = (
    ((36, 512, 2), (37, 512, 2)),          # lds_bytes(K, M + 2) + est_bytes(K) <= 160 KiB at K = 512
    ((16, 1024, 2), (17, 1024, 2)),        # ... at K = 1024
    ((48, 16, 2), (49, 16, 2)),            # M <= 48
    ((3, 3, 3), (3, 3, 4)),                # L <= K where K is not a power of two
)


def name(shape):
    return "%dx%dx%d" % shape


def _routes():
    r = {}
    for s in RADIX:
        r[name(s)] = dict(shape=s, kernel="rowlane_jit", entries=RX + (A.IC if s in OVERLAP_IC else ()))
    for inner, outer in EDGES:
        r[name(inner)] = dict(shape=inner, kernel="rowlane_jit", entries=RX)
        r[name(outer)] = dict(shape=outer, kernel="generic_lds", entries=RX, outer=True)
    for n, d in r.items():
        M, K, _ = d["shape"]
        d.update(B=A._blocks(M, K, n), adv=bool(set(d["entries"]) & set(A.IC)), margin=A.MARGIN, ic_mx=0)
    return r


ROUTES = _routes()
INNER = sorted(n for n, d in ROUTES.items() if not d.get("outer"))
CASES = [(n, kind) for n in INNER for kind in A.KINDS]
EDGE_CASES = [(name(i), name(o), kind) for i, o in EDGES for kind in A.KINDS]
# seed offsets of the cancellation cases, chosen so that the decision guard keeps at least half of the blocks (tests/test_codelets.py asserts it)
IC_SEED = {}


@functools.lru_cache(maxsize=None)
def make_case(route, kind):
    """accuracy_cases.make_shape_case on a shape of this list: inputs, float64 results, the cancellation case where the shape has one"""
    r = ROUTES[route]
    return A.make_shape_case(route, r["shape"], r["B"], kind, 0, IC_SEED.get((route, kind), 0), r["adv"])


@functools.lru_cache(maxsize=None)
def reference_figures(route, kind):
    """{entry: figures of the C oracle on the case's inputs}"""
    return A.case_reference_figures(make_case(route, kind), ROUTES[route]["entries"])
