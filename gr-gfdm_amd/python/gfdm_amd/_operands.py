"""The operands of a C-ABI call, for the host flavour (numpy arrays) and the device flavour (torch device tensors) alike.

A call has a leading operand; its kind -- host array or device tensor -- picks the flavour, and every other array of the call must be of
that kind.  The functions here answer, once, what every class of capi.py asks about an array argument: kind, element type, layout
(contiguity, GPU ordinal, element count), pointer, and a result of the leading operand's kind.  Nothing here touches a handle, the
library or the device beyond allocating a result, so whatever they raise, they raise before the C call.  torch is imported only where a
tensor has already been seen, or has to be made.
"""
import math

import numpy as np


class _TorchDtypes(dict):
    """numpy scalar type -> torch dtype; torch is imported when the first tensor asks"""

    def __missing__(self, dtype):
        import torch
        t = self[dtype] = getattr(torch, np.dtype(dtype).name)
        return t


_TORCH_DTYPE = _TorchDtypes()


def is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def on_device(x):
    """is_tensor() of an operand that operand() has checked: what is no numpy array there is a device tensor"""
    return not isinstance(x, np.ndarray)


def size(x):
    numel = getattr(x, "numel", None)
    return numel() if numel is not None else np.asarray(x).size


def ptr(a):
    """the address of a checked operand (None stays None); the caller holds `a` until the C call has returned"""
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _kind(tensor, host="a host array"):
    return "a CUDA/HIP tensor" if tensor else host


def bound(x, dtype, what, dev, like=None, as_what="the input", floating=False, address=True):
    """x as a C-contiguous operand of `dtype`, with what the C call takes of it, in ONE call (the block calls users put in loops spend their
    host time here): (operand, its address -- None without `address` --, its element count).  A device tensor must be of `dtype`,
    contiguous and on GPU `dev` already (TypeError / RuntimeError); a host array is converted where it is not (no copy where it is), except
    that packed bytes (uint8) must be uint8 and, with `floating`, integer input where complex samples are expected is a TypeError.
    `like`: the leading operand (`as_what`, checked already), whose kind x must have."""
    tensor = is_tensor(x)
    if like is not None and tensor != on_device(like):
        raise TypeError("%s must be %s, as %s is" % (what, _kind(not tensor), as_what))
    if tensor:
        if x.dtype != _TORCH_DTYPE[dtype] or not x.is_cuda or not x.is_contiguous():
            raise TypeError("%s must be a contiguous %s CUDA/HIP tensor" % (what, np.dtype(dtype).name))
        if x.device.index != dev:
            raise RuntimeError("%s lives on GPU %d, the handle on GPU %d" % (what, x.device.index, dev))
        return x, x.data_ptr() if address else None, x.numel()
    x = np.asarray(x)
    if dtype == np.uint8 and x.dtype != np.uint8:
        raise TypeError("%s must be uint8 (packed bytes), not %s" % (what, x.dtype))
    if floating and not (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.complexfloating)):
        raise TypeError("%s must be complex samples, not %s" % (what, x.dtype))
    x = np.ascontiguousarray(x, dtype=dtype)
    return x, x.ctypes.data if address else None, x.size


def operand(x, dtype, what, dev, like=None, as_what="the input", floating=False):
    """the operand of bound(), alone"""
    return bound(x, dtype, what, dev, like, as_what, floating, False)[0]


def vector(x, dtype, what, dev, like, n=None, as_what="the input"):
    """operand() as a flat vector, of exactly n elements where n is given"""
    x = operand(x, dtype, what, dev, like, as_what)
    if not on_device(x):
        x = x.ravel()
    return x if n is None else sized(x, n, what)


def sized(x, n, what):
    if size(x) != n:
        raise RuntimeError("%s has %d elements, expected %d" % (what, size(x), n))
    return x


def at_least(x, n, what):
    if size(x) < n:
        raise RuntimeError("%s size(%d) MUST be at least %d!" % (what, size(x), n))
    return x


def batches(x, n, message):
    """size(x) / n where that is whole; else RuntimeError(message % (size, n))"""
    s = size(x)
    if n <= 0 or s % n:
        raise RuntimeError(message % (s, n))
    return s // n


def rows(x, dtype, what, dev, width=None, like=None, as_what="the input"):
    """x as rows of `dtype` -> (x, n_rows, width, was 1-D): (n_rows, n), or one row (n,)"""
    x = operand(x, dtype, what, dev, like, as_what, floating=dtype == np.complex64)
    if x.ndim not in (1, 2):
        raise ValueError("%s must be (n_rows, n) or one row (n,), not %s" % (what, tuple(x.shape)))
    flat = x.ndim == 1
    n_rows, w = (1, x.shape[0]) if flat else (x.shape[0], x.shape[1])
    if width is not None and w != width:
        raise RuntimeError("%s has rows of %d elements, expected %d" % (what, w, width))
    return x, int(n_rows), int(w), flat


def sc16_pairs(shape, what, reshape=None):
    """number of samples of an sc16 array of `shape` -- (n, 2) or flat (2n,) -- or, with `reshape`, the array as (n, 2)"""
    shape = tuple(shape)
    if len(shape) == 2 and shape[1] == 2:
        n = shape[0]
    elif len(shape) == 1:
        if shape[0] % 2:
            raise ValueError("%s: a flat sc16 array holds I, Q pairs, its length(%d) is odd" % (what, shape[0]))
        n = shape[0] // 2
    else:
        raise ValueError("%s: an sc16 array has shape (n, 2) or (2n,), not %s" % (what, shape))
    return n if reshape is None else reshape(n, 2)


def check_result(out, like, dtype, dev, what="out", as_what="the input", n=None, unit="elements", off_device=TypeError):
    """A caller's `out`: of `like`'s kind (a numpy array proper on the host path, so that the call writes in place), of `dtype`,
    contiguous, on GPU `dev`; int16 means sc16, of shape (n, 2) or (2n,).  n: the elements it must hold, whatever its shape (None: what
    can be said before the size is known).  off_device: what a tensor that is on no GPU raises -- SymbolMapper and LinkMeter have
    always answered that with the RuntimeError of a tensor on the wrong GPU, the other classes with the TypeError of a wrong layout."""
    if out is None:
        return
    tensor = on_device(like)
    if is_tensor(out) != tensor or not (tensor or isinstance(out, np.ndarray)):
        raise TypeError("%s must be %s, as %s is" % (what, _kind(tensor, "a numpy array"), as_what))
    if out.dtype != (_TORCH_DTYPE[dtype] if tensor else dtype):
        raise TypeError("%s must be %s, not %s" % (what, "int16 I/Q (sc16)" if dtype == np.int16 else np.dtype(dtype).name,
                                                   str(out.dtype).replace("torch.", "")))
    if tensor:
        if not out.is_cuda and off_device is RuntimeError:
            raise RuntimeError("%s must live on GPU %d, as the handle does" % (what, dev))
        if not out.is_cuda or not out.is_contiguous():
            raise TypeError("%s must be a contiguous %s CUDA/HIP tensor" % (what, np.dtype(dtype).name))
        if out.device.index != dev:
            raise RuntimeError("%s lives on GPU %d, the handle on GPU %d" % (what, out.device.index, dev))
    elif not out.flags.c_contiguous:
        raise TypeError("%s must be contiguous" % what)
    if dtype == np.int16:
        sc16_pairs(out.shape, what)
    if n is not None and (out.numel() if tensor else out.size) != n:
        per = 2 if dtype == np.int16 else 1                  # sc16: counted in samples
        raise RuntimeError("%s holds %d %s, expected %d" % (what, size(out) // per, unit, n // per))


def result(like, shape, dtype, dev, out=None, what="out", as_what="the input", unit="elements", off_device=TypeError):
    """A result of `like`'s kind: a new array / tensor of `shape` and `dtype` (on like's device), or the caller's `out` after
    check_result, with as many elements as `shape` has."""
    if out is None:
        if not on_device(like):
            return np.empty(shape, dtype)
        import torch
        return torch.empty(shape, dtype=_TORCH_DTYPE[dtype], device=like.device)
    check_result(out, like, dtype, dev, what, as_what, math.prod(shape), unit, off_device)
    return out


def stream_result(like, n, sc16, dev, out=None, as_what="the input"):
    """result() for n samples of a stream: complex64 (n,), or with sc16 int16 I/Q of shape (n, 2)"""
    return result(like, (n, 2) if sc16 else (n,), np.int16 if sc16 else np.complex64, dev, out, "out", as_what, "samples")


def count_arg(count, like, dev):
    """The optional live count of a call (None: everything) as the one-element int64 operand the C-ABI reads: on the host path from an
    int, on the device path an int (uploaded) or a one-element int64 tensor such as detect's."""
    if count is None:
        return None
    if not on_device(like):
        if is_tensor(count):
            raise TypeError("count must be an int on the host path")
        return sized(np.ascontiguousarray(count, dtype=np.int64).ravel(), 1, "count")
    if not is_tensor(count):
        import torch
        count = torch.full((1,), int(count), dtype=torch.int64, device=like.device)
    return sized(operand(count, np.int64, "count", dev), 1, "count")


def workspace(ws, like, need, dev):
    """the device scratch of a call: `ws`, a uint8 tensor of at least `need` bytes on GPU `dev`, or a new one beside `like`"""
    import torch
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=like.device)
    if not is_tensor(ws) or ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need or ws.device.index != dev:
        raise TypeError("workspace must be a contiguous uint8 CUDA/HIP tensor of at least %d bytes on GPU %d" % (need, dev))
    return ws


def capture(samples, dev, what="samples"):
    """A capture argument -> (operand, n_samples, name infix): complex64 (anything operand() takes on the host path, a contiguous
    complex64 tensor on the device path: infix "") or sc16 (a contiguous int16 array / tensor of shape (n, 2) or (2n,): infix "_sc16",
    passed on as it is, never widened).  Any other integer dtype is a TypeError."""
    tensor = is_tensor(samples)
    a = samples if tensor else np.asarray(samples)
    if a.dtype == (_TORCH_DTYPE[np.int16] if tensor else np.int16):
        n = sc16_pairs(a.shape, what)
        if tensor:
            operand(a, np.int16, what, dev)
        elif not a.flags.c_contiguous:
            raise TypeError("%s must be a C-contiguous int16 array" % what)
        return a, n, "_sc16"
    integer = not (a.dtype.is_floating_point or a.dtype.is_complex) if tensor else np.issubdtype(a.dtype, np.integer)
    if integer:
        raise TypeError("%s: integer captures must be int16 (sc16), not %s" % (what, a.dtype))
    a = operand(a, np.complex64, what, dev)
    if not tensor:
        a = a.ravel()
    return a, size(a), ""
