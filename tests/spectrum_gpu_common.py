"""What tests/test_spectrum_meter_gpu.py and tests/test_spectrum_grid_bound_gpu.py share: device inputs between canaries, the comparison of
two reads, and the check of psd_sum against the restatement of tests/spectrum_meter_ref.py under both yardsticks.  Every check prints its
figures ("spectrum accuracy: ...") before it asserts; profiles/r22/spectrum_accuracy.json is made of those lines."""
import numpy as np

import spectrum_meter_ref as R

DEV = "cuda:0"
GUARD = 8
INT = ("segments", "bad_segments", "samples", "bad_samples", "peak_bits")


def to_device(a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


class Guarded:
    """the samples x (complex64 (n,) or int16 (n, 2)) inside a larger device buffer, `shift` samples past a 16-byte boundary, with
    canaries on either side"""

    def __init__(self, x, shift=0):
        import torch
        x = np.asarray(x)
        self.sc16 = x.dtype == np.int16
        flat = x.reshape(-1)
        per = 2 if self.sc16 else 1
        self.fill = 0x5A5A if self.sc16 else 7 + 7j
        self.lo, self.n = (GUARD + shift) * per, flat.size
        self.buf = torch.full((self.lo + self.n + GUARD * per,), self.fill, dtype=torch.int16 if self.sc16 else torch.complex64, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.lo:self.lo + self.n] = to_device(flat)
        self.before = self.buf.clone()
        self.view = self.buf[self.lo:self.lo + self.n]
        if self.sc16:
            self.view = self.view.view(-1, 2)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (shift * (4 if self.sc16 else 8)) % 16

    def unchanged(self):
        import torch
        a, b = self.buf, self.before
        if not self.sc16:
            a, b = torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32)
        return torch.equal(a, b)


def same_totals(a, b):
    """are two reads equal to the bit; prints the fields that are not"""
    differ = [k for k in INT + ("power_sum",) if a[k] != b[k]] + [k for k in ("psd_sum", "hist") if not np.array_equal(a[k], b[k])]
    if differ:
        print("the totals differ in", differ)
    return not differ


def check_psd(t, r, label, yardstick=True):
    share = R.budget_share(t["psd_sum"], r)
    ratio = R.yardstick_ratio(t["psd_sum"], r) if yardstick else float("nan")
    print("spectrum accuracy: %s: yardstick ratio %.3f (numpy's own %.3f of the floor), worst budget share %.4f"
          % (label, ratio, r["numpy_error"] / (2.0 ** -24 * r["norm"]) if r["norm"] else 0.0, share))
    assert (t["segments"], t["bad_segments"]) == (r["segments"], r["bad_segments"]), label
    assert share <= 1.0, (label, share)
    if yardstick:
        assert ratio <= R.YARDSTICK, (label, ratio)
