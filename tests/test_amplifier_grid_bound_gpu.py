"""The amplifier model past its bounded grid, as tests/test_fading_grid_bound_gpu.py does it for the fading model: k_amplify launches at
most G = 2048 workgroups and strides over the remaining tiles, and the other GPU tests stay far below G tiles, so a workgroup's second
trip through its tile loop -- POLY's two LDS arrays reused behind a barrier, index arithmetic at tile numbers of 2048 and above -- runs
here and nowhere else.  One complex64 POLY(3, 3) case and one sc16 RAPP case of 2 G + 3 tiles with a ragged last one and the output one
sample past a 16-byte boundary (the case arithmetic: tests/amplifier_model_ref.py, held to the kernel's constants by
tests/test_amplifier_model.py), three checks each:
  1. against the restatement under the error budget (sc16: the guard-band rule), on windows: the sample ranges under the tiles 0,
     G - 1 | G, 2 G - 1 | 2 G and the last two, and 64 seeded ranges of 4096 samples, each from the stream's own history;
  2. against the same handle called in three pieces that each stay below G tiles, over the WHOLE output, on the device, bit for bit;
  3. canaries on both sides of every buffer.
The input is made on the device from a fixed seed; only the windows travel to the host."""
import gc

import numpy as np
import pytest

import amplifier_model_ref as Am
import grid_bound_cases as G
from conftest import have_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
FILL = {"int16": 0x5A5A, "complex64": 7 + 7j}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    if not have_gpu():
        pytest.fail("no MI355X visible: the HIP path cannot run (there is no CPU fallback to test instead)")


@pytest.fixture(autouse=True)
def _give_the_memory_back():
    yield
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _h(t):
    return t.cpu().numpy()


def _same(a, b):
    import torch
    if a.is_complex():
        a, b = torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32)
    return torch.equal(a, b)


class Guarded:
    """n elements of `dtype` inside a larger device buffer, `shift` elements past a 16-byte boundary, canaries on either side that are
    checked on the device"""

    def __init__(self, dtype, n, shift=0):
        import torch
        self.fill, self.lo, self.n = FILL[dtype], GUARD + shift, n
        self.buf = torch.full((self.lo + n + GUARD,), self.fill, dtype=getattr(torch, dtype), device=DEV)
        self.view = self.buf[self.lo:self.lo + n]
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * self.buf.element_size()) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.lo + self.n:] == self.fill).all())


@pytest.mark.parametrize("case", Am.GRID_CASES, ids=G.case_id)
def test_amplifier(case):
    import torch
    import gfdm_amd
    geo = Am.grid_geometry(case)
    n, sc16 = geo["n"], case["sc16"]
    sp = Am.grid_spec(case)
    Q = Am.delays(sp)
    gain = Am.sc16_gain(sp) if sc16 else 1.0
    am = gfdm_amd.AmplifierModel(sp["kind"], tuple(sp["p"]), sp["c"])
    hist = Q - 1
    gen = torch.Generator(device=DEV)
    gen.manual_seed(G.SEED + case["seed"])
    x = Guarded("complex64", hist + n, 0)
    x.view.copy_(torch.view_as_complex(torch.randn((hist + n, 2), device=DEV, generator=gen)) * 0.5)
    per = 2 if sc16 else 1
    kw = dict(sc16=True, gain=gain) if sc16 else {}
    out = Guarded("int16" if sc16 else "complex64", n * per, case["mis"] * per)
    am.apply(x.view, hist, out=out.view, **kw)
    # 1. every window from the stream's own contract: its history
    worst, in_guard, seen = 0.0, 0, 0
    for a, b in G.stream_windows(geo["tiling"], 9):
        hw = min(Q - 1, hist + a)
        y, budget = Am.apply(_h(x.view[hist + a - hw:hist + b]), hw, sp)
        got = _h(out.view[a * per:b * per])
        if sc16:
            want, guard = Am.sc16(y, budget, gain)
            got = got.reshape(-1, 2)
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            assert np.array_equal(got[~guard], want[~guard]) and d.max(initial=0) <= 1, (a, b)
            in_guard += int(guard.sum())
            seen += guard.size
        else:
            share = Am.share_of_budget(got, y, budget)
            worst = max(worst, share)
            assert share <= 1.0, (a, b, share)
    print("%s: worst error %.3f of the budget, %d of %d components inside the sc16 guard band" % (case["id"], worst, in_guard, seen))
    assert in_guard <= Am.GUARD_CAP * max(seen, 1)
    # 2. the stream cut into three
    again = Guarded("int16" if sc16 else "complex64", n * per, 0)
    for a, b in G.pieces(n):
        hp = min(Q - 1, hist + a)
        am.apply(x.view[hist + a - hp:hist + b], hp, out=again.view[a * per:b * per], **kw)
    assert _same(out.view, again.view)
    # 3.
    assert out.intact() and again.intact() and x.intact()
