"""float64 numpy restatement of the amplifier model's contract (include/gfdm_hip.h, gfdm_hip_amplifier_model) on complex64 inputs, with
the error budgets, a plain numpy-float32 evaluation of every kind written operation by operation (what float32 arithmetic needs of the
budgets, apart from the kernel), the kinds and shapes of the GPU tests, the geometry cases, the grid-bound cases and the constants of the
end-to-end test.  Shared by tests/test_amplifier_model.py (CPU), tests/test_amplifier_model_gpu.py and
tests/test_amplifier_grid_bound_gpu.py, and the yardstick of all three: nothing here calls the library."""
import functools

import numpy as np

from channel_model_ref import GUARD_CAP, q16, sc16, share_of_budget, signal  # noqa: F401  (the sc16 rule and the seeded inputs are the channel model's)

KINDS = ("clip", "rapp", "saleh", "poly")
N_PARAMS = {"clip": 1, "rapp": 3, "saleh": 4, "poly": 0}
MAX_DELAYS, MAX_ORDERS = 16, 5
EPS = 2.0 ** -23


def spec(kind, *params, c=None):
    """a kind as the handle keeps it: the parameters rounded to float32 (held as float64), c complex64 of shape (Q, K)"""
    assert kind in KINDS and len(params) == N_PARAMS[kind]
    p = np.asarray(params, np.float64).astype(np.float32).astype(np.float64)
    if kind == "poly":
        c = np.asarray(c, np.complex64)
        c = c[None, :] if c.ndim == 1 else c
        assert c.ndim == 2 and 1 <= c.shape[0] <= MAX_DELAYS and 1 <= c.shape[1] <= MAX_ORDERS
    else:
        assert c is None
    return dict(kind=kind, p=p, c=c)


def tag(sp):
    return sp["kind"] + ("(%d,%d)" % sp["c"].shape if sp["kind"] == "poly" else "(" + ", ".join("%g" % v for v in sp["p"]) + ")")


def drive32(drive):
    return float(np.float32(drive))


# ---- the contract in float64 ----
def _u(x, drive):
    return drive32(drive) * np.asarray(x, np.complex64).astype(np.complex128)


def floor_of(kind):
    """the derived part of a closed form's budget, in units of 2^-23 |y|"""
    return {"clip": 8.0, "rapp": 8.0, "saleh": 16.0}[kind]


def apply(x, history, sp, drive=1.0):
    """the contract in float64 on complex64 inputs -> (y64, budget) for the n = len(x) - history samples behind the history, zeros before
    x.  budget: POLY (4 K + Q + 8) 2^-23 S_i; a closed form floor_of(kind) 2^-23 |y| (the tests widen it to B of closed_form_B)"""
    u = _u(x, drive)
    n = u.size - history
    kind, p = sp["kind"], sp["p"]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if kind == "poly":
            c = sp["c"].astype(np.complex128)
            Q, K = c.shape
            uz = np.concatenate((np.zeros(Q - 1, np.complex128), u))
            r = np.abs(uz) ** 2
            lo = Q - 1 + history
            y, S = np.zeros(n, np.complex128), np.zeros(n)
            for k in range(K):
                y += np.convolve(uz * r ** k, c[:, k])[lo:lo + n]
                S += np.convolve(np.abs(uz) ** (2 * k + 1), np.abs(c[:, k]))[lo:lo + n]
            return y, (4 * K + Q + 8) * EPS * S
        u = u[history:]
        r = u.real ** 2 + u.imag ** 2
        if kind == "clip":
            A = p[0]
            y = np.where(r <= A * A, u, u * A / np.sqrt(r))
        elif kind == "rapp":
            g, A, pp = p
            t = g * g * r / (A * A)
            low = g * u * (1.0 + np.minimum(t, 1.0) ** pp) ** (-0.5 / pp)
            high = A * u / np.sqrt(r) * (1.0 + np.maximum(t, 1.0) ** -pp) ** (-0.5 / pp)             # the same curve: g u / sqrt t = A u / sqrt r
            y = np.where(t <= 1.0, low, high)
        else:
            aa, ba, ap, bp = p
            y = u * aa / (1.0 + ba * r) * np.exp(1j * ap * r / (1.0 + bp * r))
        return y, floor_of(kind) * EPS * np.abs(y)


# ---- plain numpy float32, operation by operation (no fused multiply-add) ----
def apply32(x, history, sp, drive=1.0):
    """every kind as float32 arithmetic forms it, in the order the contract names -> complex128 of float32 values"""
    f = np.float32
    x = np.asarray(x, np.complex64)
    d = f(drive)
    kind = sp["kind"]
    p = sp["p"].astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ur, ui = d * x.real, d * x.imag
        r = ur * ur + ui * ui
        assert ur.dtype == r.dtype == np.float32
        if kind == "poly":
            c = sp["c"]
            Q, K = c.shape
            n = x.size - history
            z = np.zeros(Q - 1, np.float32)
            ur, ui, r = np.concatenate((z, ur)), np.concatenate((z, ui)), np.concatenate((z, r))
            yr, yi = np.zeros(n, np.float32), np.zeros(n, np.float32)
            for q in range(Q):
                s = slice(Q - 1 + history - q, Q - 1 + history - q + n)
                gr, gi = np.full(n, c[q, K - 1].real, np.float32), np.full(n, c[q, K - 1].imag, np.float32)
                for k in range(K - 2, -1, -1):
                    gr, gi = gr * r[s] + f(c[q, k].real), gi * r[s] + f(c[q, k].imag)
                yr = yr + gr * ur[s] - gi * ui[s]
                yi = yi + gr * ui[s] + gi * ur[s]
            assert yr.dtype == np.float32
            return yr.astype(np.float64) + 1j * yi.astype(np.float64)
        ur, ui, r = ur[history:], ui[history:], r[history:]
        if kind == "clip":
            A = p[0]
            s = np.where(r <= f(np.float64(A) * np.float64(A)), f(1), A / np.sqrt(r))
            yr, yi = np.where(s == 1, ur, ur * s), np.where(s == 1, ui, ui * s)
        elif kind == "rapp":
            g, A, pp = p
            k = f(np.float64(g) ** 2 / np.float64(A) ** 2)
            h = f(1.0 / (2.0 * np.float64(pp)))
            t = k * r
            low = g * np.power(f(1) + np.power(np.minimum(t, f(1)), pp), -h)
            high = (A / np.sqrt(r)) * np.power(f(1) + np.power(np.maximum(t, f(1)), -pp), -h)
            s = np.where(t <= 1, low, high)
            assert s.dtype == np.float32
            yr, yi = ur * s, ui * s
        else:
            aa, ba, ap, bp = p
            am = aa / (ba * r + f(1))
            ph = (ap * r) / (bp * r + f(1))
            cs, sn = np.cos(ph), np.sin(ph)
            assert cs.dtype == np.float32
            vr, vi = ur * am, ui * am
            yr, yi = vr * cs - vi * sn, vr * sn + vi * cs
        return yr.astype(np.float64) + 1j * yi.astype(np.float64)


def rapp32_naive(x, sp, drive=1.0):
    """the formula of the table written as it stands in float32: t^p overflows and y comes out 0 (what the contract's second branch is for)"""
    f = np.float32
    x = np.asarray(x, np.complex64)
    g, A, pp = sp["p"].astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ur, ui = f(drive) * x.real, f(drive) * x.imag
        t = g * g * (ur * ur + ui * ui) / (A * A)
        s = g * np.power(f(1) + np.power(t, pp), -f(0.5) / pp)
        return (ur * s).astype(np.float64) + 1j * (ui * s).astype(np.float64)


def need_of(got, y):
    """what an evaluation needs of a closed form's budget: the worst |got - y| / (2^-23 |y|)"""
    err = np.abs(np.asarray(got).astype(np.complex128) - y)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(err == 0, 0.0, err / (EPS * np.abs(y)))
    return float(np.max(share)) if share.size else 0.0


def closed_form_B(x, sp, drive=1.0):
    """B of a closed form on these inputs: the larger of the derived floor and twice what the float32 numpy evaluation needs"""
    y, _ = apply(x, 0, sp, drive)
    return max(floor_of(sp["kind"]), 2.0 * need_of(apply32(x, 0, sp, drive), y))


# ---- the kinds and inputs of the accuracy test ----
SALEH_CLASSIC = (2.1587, 1.1517, 4.0033, 9.1040)
SALEH_PI = (2.0, 1.0, float(np.pi), 1.0)           # the phase climbs to pi (as float32: just below it) and never passes it
RAPP_PS = (0.5, 1.0, 2.0, 3.0, 10.0)
POLY_SHAPES = ((1, 1), (1, 2), (3, 3), (4, 5), (16, 5))


@functools.lru_cache(maxsize=None)
def poly_coefficients(Q, K, real=False, seed=0):
    """c (Q, K) complex64: c[0][0] = 1, decaying with the delay and by a factor of ten an order"""
    rng = np.random.default_rng([2300, Q, K, seed])
    c = (rng.standard_normal((Q, K)) + (0 if real else 1j) * rng.standard_normal((Q, K))) * 0.5 ** (1 + np.arange(Q)[:, None] / 2.0) * 0.1 ** np.arange(K)[None, :]
    c[0, 0] = 1.0
    return c.astype(np.complex64)


def closed_forms():
    return ([spec("clip", 1.0)] + [spec("rapp", 2.0, 1.5, p) for p in RAPP_PS] + [spec("saleh", *SALEH_CLASSIC), spec("saleh", *SALEH_PI)])


def polys():
    return [spec("poly", c=poly_coefficients(Q, K)) for Q, K in POLY_SHAPES]


def wide_signal(seed, n):
    """amplitudes spread over e^-6 .. e^3 times a unit Gaussian: straddles every knee"""
    rng = np.random.default_rng([2301, seed])
    return (np.exp(rng.uniform(-6.0, 3.0, n)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


# ---- the kernel's constants, MIRRORED (tests/test_amplifier_model.py holds them to the source) ----
SOURCE = "gr-gfdm_amd/csrc/gfdm_amplifier.hip"
K_TILE, K_MAX_TILES, K_LANES = 2048, 2048, 256

# ---- the geometry cases ----
GEOMETRY_NS = (1, 2, 3, K_TILE - 1, K_TILE, K_TILE + 1)


def geometry_kinds():
    return [spec("clip", 1.0), spec("rapp", 2.0, 1.5, 2.0), spec("saleh", *SALEH_CLASSIC), spec("poly", c=poly_coefficients(3, 3)),
            spec("poly", c=poly_coefficients(16, 5, real=True))]


def delays(sp):
    return sp["c"].shape[0] if sp["kind"] == "poly" else 1


def histories(sp):
    Q = delays(sp)
    return (0, Q - 1, Q + 4)


def geometry_signal(seed, n):
    """unit Gaussian samples at half scale: around the knees, and a polynomial of order nine stays far from the int16 range"""
    return (0.5 * signal(seed, n).astype(np.complex128)).astype(np.complex64)


def sc16_gain(sp):
    """the gain of the sc16 cases: far from saturation, and the guard band gain * budget around every step of q stays under GUARD_CAP of a
    case's components on the restatement alone (tests/test_amplifier_model.py asserts it)"""
    return 64.0 if sp["kind"] == "poly" else 256.0


@functools.lru_cache(maxsize=None)
def geometry_cases(kind_index):
    """per n and history one input; per format every alignment of in (0, 1) and of out (0, 1; sc16 0 .. 3)"""
    sp = geometry_kinds()[kind_index]
    out = []
    for ni, n in enumerate(GEOMETRY_NS):
        for hi, history in enumerate(histories(sp)):
            out.append(dict(n=n, history=history, seed=2310 + 100 * kind_index + 10 * ni + hi,
                            aligns=[(fmt, i, o) for fmt in ("c64", "sc16") for i in (0, 1) for o in range(4 if fmt == "sc16" else 2)]))
    return out


def pieces_with_history(sp, n, history, parts=3):
    """[(a, b, h)]: the stream cut into nearly equal pieces, each with the history it may pass"""
    cuts = [n * p // parts for p in range(parts + 1)]
    return [(a, b, min(delays(sp) - 1, history + a)) for a, b in zip(cuts[:-1], cuts[1:])]


# ---- past the bounded grid ----
GRID_CASES = [
    dict(id="c64-poly-3-3-mis", sc16=False, kind="poly", mis=1, seed=81),
    dict(id="sc16-rapp-mis", sc16=True, kind="rapp", mis=1, seed=82),
]


def grid_spec(case):
    return spec("poly", c=poly_coefficients(3, 3)) if case["kind"] == "poly" else spec("rapp", 2.0, 1.5, 2.0)


def grid_geometry(case):
    """n and the Tiling of a grid-bound case: 2 G + 3 tiles with a ragged last one (grid_bound_cases' Tiling and sizing rule)"""
    import grid_bound_cases as G
    n = G.sized(K_MAX_TILES, K_TILE, 1, case["mis"]) - K_TILE // 3
    return dict(n=n, tiling=G.Tiling(K_MAX_TILES, K_TILE, n, case["mis"]))


# ---- two tones through a third-order polynomial ----
TONE_NFFT, TONE_K1, TONE_K2, TONE_A, TONE_C3, TONE_SEGMENTS = 1024, 100, 110, 0.25, -0.2 + 0.05j, 4


def two_tones():
    n = np.arange(TONE_NFFT * TONE_SEGMENTS)
    return (TONE_A * (np.exp(2j * np.pi * TONE_K1 * n / TONE_NFFT) + np.exp(2j * np.pi * TONE_K2 * n / TONE_NFFT))).astype(np.complex64)


def two_tone_answer():
    """{bin: power} of the fundamentals and the third-order products for psd() of a rect window"""
    a, c3 = TONE_A, complex(np.complex64(TONE_C3))
    return {TONE_K1: abs(1 + 3 * c3 * a * a) ** 2 * a * a, TONE_K2: abs(1 + 3 * c3 * a * a) ** 2 * a * a,
            2 * TONE_K1 - TONE_K2: abs(c3) ** 2 * a ** 6, 2 * TONE_K2 - TONE_K1: abs(c3) ** 2 * a ** 6}


def two_tone_slack():
    """the largest error of one output sample: the budget of POLY(1, 2) at the peak of the envelope 2 a, and what the rounding of the tones
    to complex64 (2^-23 |x| at most) becomes behind y = u + c3 u |u|^2, whose derivative is at most 1 + 3 |c3| r.  An error sequence
    bounded by b moves a bin's amplitude by at most b."""
    a2, c3 = 2 * TONE_A, abs(TONE_C3)
    return (4 * 2 + 1 + 8) * EPS * (a2 + c3 * a2 ** 3) + EPS * a2 * (1 + 3 * c3 * a2 * a2)


# ---- end to end: burst_shaper_ref.loop_case() through a Rapp amplifier, then the channel loop's CFO and noise ----
LOOP_P = 2.0
LOOP_BACKOFF_LADDER = (12.0, 9.0, 6.0, 4.0, 3.0)          # dB; the smallest at which the margins hold is used
LOOP_BACKOFF = 6.0                                      # chosen by tests/test_amplifier_model.py::test_loop_preconditions, which asserts the choice


def loop_spec():
    return spec("rapp", 1.0, 1.0, LOOP_P)


def backoff_drive(mean_power, backoff_db, A=1.0):
    return float(A * np.sqrt(10.0 ** (-backoff_db / 10.0) / mean_power))


@functools.lru_cache(maxsize=None)
def loop_stream(backoff_db=LOOP_BACKOFF):
    """(x, d, z, y, budget): the placed stream of the loop case, the drive that puts its mean power backoff_db below A^2 = 1, the
    amplifier's output (float64), and the channel model's output for it rounded to complex64, with the tap 1 / d that takes the level back
    (the channel loop's CFO, noise and seed)"""
    import channel_model_ref as C
    x = C.loop_stream()[0]
    d = backoff_drive(float(np.mean(np.abs(x.astype(np.complex128)) ** 2)), backoff_db)
    z, _ = apply(x, 0, loop_spec(), d)
    y, budget = C.apply(z.astype(np.complex64), 0, [np.float32(1.0 / d)], C.LOOP_F, C.LOOP_NOISE_VOLTAGE, C.LOOP_SEED, 0)
    return x, d, z, y, budget
