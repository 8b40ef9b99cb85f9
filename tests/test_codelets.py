"""CPU side of the codelet tests (no GPU).

  codelets  Every timeslot codelet of csrc/gfdm_dft.h -- dft_inplace<N, INV>, N = 1 .. 48, both directions: 96 instantiations, each
            straight-line code with its own index maps and twiddle literals -- runs ON THE HOST: tests/dft_codelets_host.cc includes the
            unmodified header with __device__ redefined and is compiled here.  64 random complex64 vectors per instantiation are
            compared with a float64 direct DFT of the same float32 inputs by accuracy_cases.figures; the bound of every figure is
            accuracy_cases.bounds (MARGIN unchanged) of the figure a float32 direct-sum DFT (float32 accumulation, twiddles computed in
            float64 and rounded once) reaches on the same vectors, and l2 stays below REF_L2_CAP.  (A figure of exactly 0 -- N = 1 on
            both sides -- is inside any bound.)  Without tolerance: a unit impulse at n = 0 returns all ones in exact bits, and
            a power-of-two scaling of the input scales the output bits.
            The method bites: with inverse_mod() returning i + 1 (the Good-Thomas output map) and with the sign of sin2pi flipped in
            mul_root() (the Cooley-Tukey twiddles), each planted in a temporary copy of the header, the same judgement fails.
  plans     tests/rowgeom_table.cc prints the plan of every K = 1 .. 1024 from csrc/gfdm_rowgeom.h itself.  The row-lane shapes of the
            suite (codelet_cases, tap_cases.ROUTES, accuracy_cases.ROUTES, csrc/gfdm_row_shapes.h and the parameter list of
            test_row_lane_kernels_instantiated_at_run_time) must cover every radix 2 .. 32 as a pass factor, every radix 18 .. 32 as the
            LAST pass, a three-pass plan with factor limit 32 and every overlap 2 .. 8; a removed shape names the radix that lost its cover.
            The edges of codelet_cases.EDGES are edges of the table, and its cancellation cases keep half of their blocks."""
import os
import re
import subprocess

import numpy as np
import pytest

import accuracy_cases as A
import codelet_cases as C
import poison_cases as P
import tap_cases as T
from conftest import ROOT
from test_sanitizers import mutated_package

CSRC = os.path.join(ROOT, "gr-gfdm_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MAX_N, RANDOM = 48, 64
SCALED = (-40, 15, 40, -3)                       # vector i < 4 once more, times 2^SCALED[i]
B = RANDOM + 1 + len(SCALED)                     # per instantiation: the random vectors, the unit impulse, the scaled copies
MUTATIONS = {
    "inverse_mod": ("        if ((a * i) % m == 1) return i;\n", "        return i + 1;\n"),
    "mul_root_sin_sign": ("(float)(INV ? sin2pi(e, N) : -sin2pi(e, N))", "(float)(INV ? -sin2pi(e, N) : sin2pi(e, N))"),
}


# ---------------------------------------------------------------- the 96 codelets on the host

def _inputs():
    """{(N, inv): (B, N) complex64}"""
    rng = np.random.default_rng(A._seed("codelets"))
    x = {}
    for N in range(1, MAX_N + 1):
        for inv in (0, 1):
            v = np.zeros((B, N), np.complex64)
            v[:RANDOM] = T._gauss(rng, (RANDOM, N))
            v[RANDOM, 0] = 1
            v[RANDOM + 1:] = A.times(v[:len(SCALED)], np.ldexp(1.0, SCALED))
            x[N, inv] = v
    return x


def _compile(include, exe):
    """the host half alone (--offload-host-only), without optimisation: the judgement is about index maps and literals"""
    return subprocess.Popen([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O0", "-ffp-contract=off", "-I" + str(include),
                             os.path.join(ROOT, "tests", "dft_codelets_host.cc"), "-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


@pytest.fixture(scope="module")
def transforms(tmp_path_factory):
    """{header: {(N, inv): (B, N) complex64 results}} for the header as committed and for each mutation, compiled side by side"""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc is not installed: the codelets cannot be compiled")
    tmp = tmp_path_factory.mktemp("codelets")
    include = {"committed": CSRC}
    for name, (old, new) in MUTATIONS.items():
        include[name] = mutated_package(tmp / name, "csrc/gfdm_dft.h", old, new) / "csrc"
    jobs = {name: _compile(inc, tmp / ("dft_" + name)) for name, inc in include.items()}
    x = _inputs()
    order = [(N, inv) for N in range(1, MAX_N + 1) for inv in (0, 1)]
    np.concatenate([x[k].reshape(-1) for k in order]).tofile(tmp / "in.c64")
    out = {}
    for name, job in jobs.items():
        log = job.communicate(timeout=900)[0].decode(errors="replace")
        assert job.returncode == 0, log[-6000:]
        p = subprocess.run([str(tmp / ("dft_" + name)), str(tmp / "in.c64"), str(tmp / (name + ".c64")), str(B)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "%d instantiations, N = 1 .. %d" % (2 * MAX_N, MAX_N) in p.stdout, p.stdout + p.stderr
        y, at, out[name] = np.fromfile(tmp / (name + ".c64"), np.complex64), 0, {}
        for N, inv in order:
            out[name][N, inv] = y[at:at + B * N].reshape(B, N)
            at += B * N
        assert at == len(y)
    return x, out


def _twiddles(N, inv):
    n = np.arange(N)
    return np.exp((2j if inv else -2j) * np.pi * ((n[:, None] * n[None, :]) % N) / N)


def _float32_direct_sum(x, N, inv):
    """the reference of the bound: y[k] = sum_n x[n] W[n, k], W computed in float64 and rounded once, products and sums in float32"""
    W = _twiddles(N, inv).astype(np.complex64)
    acc = np.zeros(x.shape, np.complex64)
    for n in range(N):
        acc = acc + x[:, n, None] * W[None, n, :]
    assert acc.dtype == np.complex64
    return acc


def _judge(x, y):
    """(failures, worst l2): every instantiation against its bounds, the cap, the impulse and the scaled copies"""
    bad, worst = [], 0.0
    for (N, inv), v in sorted(x.items()):
        got = y[N, inv]
        r, want = slice(0, RANDOM), v[:RANDOM].astype(np.complex128) @ _twiddles(N, inv)
        figs = A.figures(got[r], want)
        ref = A.figures(_float32_direct_sum(v[r], N, inv), want)
        bound = A.bounds(ref, A.MARGIN)
        worst = max(worst, figs["l2"])
        what = "N = %d %s" % (N, "inverse" if inv else "forward")
        for f in A.FIGURES:
            if not (figs[f] < bound[f] or figs[f] == 0):
                bad.append("%s: %s %.3e exceeds %.3e (float32 direct sum: %.3e)" % (what, f, figs[f], bound[f], ref[f]))
        if not figs["l2"] < A.REF_L2_CAP:
            bad.append("%s: l2 %.3e above the cap %.1e" % (what, figs["l2"], A.REF_L2_CAP))
        if not np.array_equal(P.bits(got[RANDOM]), P.bits(np.ones(N, np.complex64))):
            bad.append("%s: the unit impulse does not return all ones in exact bits: %s" % (what, got[RANDOM]))
        if not np.array_equal(P.bits(got[RANDOM + 1:]), P.bits(A.times(got[:len(SCALED)], np.ldexp(1.0, SCALED)))):
            bad.append("%s: a power-of-two scaling of the input does not scale the output bits" % what)
    return bad, worst


def test_all_96_codelets_within_the_float32_budget_on_the_host(transforms):
    x, out = transforms
    assert len(x) == 96 and all(v.shape == (B, N) for (N, _), v in x.items())
    bad, worst = _judge(x, out["committed"])
    print("%d of 96 instantiations inside their bounds, worst l2 %.3e" % (96 - len({b.split(":")[0] for b in bad}), worst))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_planted_codelet_bug_fails_the_same_judgement(transforms, mutation):
    """sensitivity: the Good-Thomas sizes (coprime factors) go wrong with the output map, the Cooley-Tukey sizes with real twiddles with the sign"""
    x, out = transforms
    bad, _ = _judge(x, out[mutation])
    sizes = sorted({int(re.match(r"N = (\d+)", b).group(1)) for b in bad})
    print(mutation, "fails at N =", sizes)
    assert bad and set(sizes) >= {"inverse_mod": {6, 12, 35, 48}, "mul_root_sin_sign": {8, 9, 25, 48}}[mutation]
    assert not set(sizes) & {1, 2, 3, 4, 5, 7, 47}               # a prime, 1, 2 and 4 use neither (nor does 15 = 3 x 5 the first: both of its inverses ARE 2)


# ---------------------------------------------------------------- the plan table of gfdm_rowgeom.h and what the suite covers of it

M_COLUMNS = list(range(3, 51))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{K: dict(supported, pow2, lim, passes (the factors in the order they run), wg, bpw, bytes={M: lds_bytes(K, M + 2) + est_bytes(K)})}"""
    exe = str(tmp_path_factory.mktemp("rowgeom") / "rowgeom_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "rowgeom_table.cc"), "-o", exe])
    t = {}
    for line in subprocess.run([exe] + [str(m) for m in M_COLUMNS], capture_output=True, text=True, check=True).stdout.splitlines():
        v = [int(w) for w in line.split()]
        assert len(v) == 10 + len(M_COLUMNS)
        t[v[0]] = dict(supported=bool(v[1]), pow2=bool(v[2]), lim=v[3], passes=tuple(v[5:5 + v[4]]), wg=v[8], bpw=v[9], bytes=dict(zip(M_COLUMNS, v[10:])))
    assert sorted(t) == list(range(1, 1025))
    return t


def _row_lane_shapes():
    """{(M, K, L): where it is tested} for every row-lane shape of the suite"""
    import test_parity_gpu
    s = {}
    for shape in C.INNER:
        s.setdefault(C.ROUTES[shape]["shape"], "codelet_cases")
    for mod, routes in (("tap_cases", T.ROUTES), ("accuracy_cases", A.ROUTES)):
        for r in routes.values():
            if r["kernel"] in ("rowlane", "rowlane_jit"):
                s.setdefault(tuple(r["shape"]), mod)
    text = open(os.path.join(CSRC, "gfdm_row_shapes.h")).read()
    compiled = re.findall(r"^\s*X\((\d+), (\d+), (\d+)\)", text, flags=re.M)
    assert len(compiled) >= 13
    for K, M, L in compiled:
        s.setdefault((int(M), int(K), int(L)), "gfdm_row_shapes.h")
    mark, = [m for m in test_parity_gpu.test_row_lane_kernels_instantiated_at_run_time.pytestmark if m.name == "parametrize"]
    assert mark.args[0] == "M,K,L,alpha" and len(mark.args[1]) >= 26
    for M, K, L, _ in mark.args[1]:
        s.setdefault((M, K, L), "test_row_lane_kernels_instantiated_at_run_time")
    return s


def test_the_plans_are_the_ones_the_shapes_are_there_for(table):
    for (M, K, L), plan in C.RADIX.items():
        assert "x".join(str(r) for r in table[K]["passes"]) == plan, (K, table[K]["passes"], plan)
    assert table[612]["lim"] == 32 and len(table[612]["passes"]) == 3
    assert {C.ROUTES[s]["shape"][0] for s in C.INNER} >= set(C.TIMESLOTS)
    assert {L for _, _, L in C.OVERLAP_IC} == {5, 7} and all(C.ROUTES[C.name(s)]["adv"] and C.ROUTES[C.name(s)]["kernel"] == "rowlane_jit" for s in C.OVERLAP_IC)
    for s, r in C.ROUTES.items():
        M, K, _ = r["shape"]
        assert r["B"] == (4 if K == 1024 else 67 if M * K <= 1024 else 29)
        assert r["B"] % table[K]["bpw"] != 0 or table[K]["bpw"] == 1            # the last workgroup is part-filled


def test_every_shape_sits_on_the_side_of_the_rules_it_is_listed_on(table):
    """the rules of jit_eligible() with the table's numbers: K supported, 3 <= M <= 48, 2 <= L <= 8, L <= K unless K is a power of two, and
    lds_bytes(K, M + 2) + est_bytes(K) <= 160 KiB; every inner shape passes all of them, every outer shape fails exactly the one of its edge"""
    def failed(M, K, L):
        t = table[K]
        rules = dict(K=t["supported"], M=3 <= M <= 48, L=2 <= L <= 8, wrap=t["pow2"] or L <= K, lds=t["bytes"][M] <= 160 * 1024)
        return sorted(k for k, ok in rules.items() if not ok)
    for s in C.INNER:
        assert failed(*C.ROUTES[s]["shape"]) == [], s
    assert [failed(*outer) for _, outer in C.EDGES] == [["lds"], ["lds"], ["M"], ["wrap"]]
    for inner, outer in C.EDGES:
        assert sum(abs(a - b) for a, b in zip(inner, outer)) == 1               # one step apart
    # the edges the issue names, from the table: M <= 36 at K = 512, M <= 16 at K = 1024, M <= 17 at K = 1000
    assert [max(M for M in M_COLUMNS if table[K]["bytes"][M] <= 160 * 1024) for K in (512, 1024, 1000)] == [36, 16, 17]


def test_the_suite_covers_every_pass_radix_and_overlap_of_the_family(table):
    shapes = _row_lane_shapes()
    as_pass, as_last, three_pass_32, overlaps = {}, {}, [], {}
    for (M, K, L), where in sorted(shapes.items()):
        t = table[K]
        assert t["supported"], (M, K, L, where)
        overlaps.setdefault(L, (M, K, L))
        for r in t["passes"]:
            as_pass.setdefault(r, K)
        if t["passes"]:
            as_last.setdefault(t["passes"][-1], K)
            if len(t["passes"]) == 3 and t["lim"] == 32:
                three_pass_32.append(K)
    print("pass radix: K", as_pass, "\nlast pass: K", as_last, "\nthree passes, limit 32:", three_pass_32, "\noverlap:", overlaps)
    missing = [r for r in range(2, 33) if r not in as_pass]
    assert not missing, "no row-lane shape of the suite has a subcarrier pass of radix %s" % missing
    missing = [r for r in range(18, 33) if r not in as_last]
    assert not missing, "no row-lane shape of the suite has radix %s as its last subcarrier pass" % missing
    assert three_pass_32, "no row-lane shape of the suite has a three-pass plan with factor limit 32"
    missing = [L for L in range(2, 9) if L not in overlaps]
    assert not missing, "no row-lane shape of the suite has overlap %s" % missing
    # the table reaches nothing else: every factor of every supported K is one of 2 .. 32
    assert {r for t in table.values() if t["supported"] for r in t["passes"]} == set(range(2, 33))


@pytest.mark.parametrize("shape", [C.name(s) for s in C.OVERLAP_IC])
@pytest.mark.parametrize("kind", A.KINDS)
def test_decision_guard_keeps_at_least_half_of_the_blocks(shape, kind):
    """as tests/test_accuracy.py, on the two overlap shapes that run the advanced receiver"""
    c = C.make_case(shape, kind)
    for inp in ("mf", "zf"):
        k = c["keep_ic_" + inp]
        print(shape, kind, inp, int(k.sum()), "of", c["B"])
        assert 2 * k.sum() >= c["B"], (inp, int(k.sum()))


@pytest.mark.parametrize("shape,kind", C.CASES)
def test_reference_figures_stay_under_the_cap(shape, kind):
    """the C oracle's own l2 on every shape's inputs: the condition under which no l2 bound rises above 1e-6"""
    for e, f in C.reference_figures(shape, kind).items():
        print("%s %s %-20s l2 %.2e peak %.2e pos %.2e" % (shape, kind, e, f["l2"], f["peak"], f["pos"]))
        assert 0 < f["l2"] < A.REF_L2_CAP and A.bounds(f)["l2"] < 1e-6
