"""ctypes binding of the C-ABI in include/gfdm_hip.h (gr-gfdm_amd/lib/libgfdm_hip.so).

Host-side mirror of the reference's kernel-class surface for Python callers that
work on whole batches and on device-resident torch tensors (bench.py, the
multi-GPU sharding helper).  The pybind11 module `gfdm_python` is the drop-in for
the reference's own binding; this module adds nothing numerically, it only
forwards pointers.  There is no CPU fallback: a missing library or GPU raises.
"""
import ctypes
import mmap

import numpy as np

from . import _abi
from . import _operands as ops
from ._abi import (EHIP, EINVAL, EINVAL_OVERLAP, EINVAL_TAPS, ENODEV, ENOMEM, EUNSUPPORTED, LIB_DIR, LIB_PATH, OK, GfdmHipError, _check,  # noqa: F401
                   exported_symbols, lib)

DECIDE = {"auto": -1, "nearest": 0, "qpsk": 1, "bpsk": 2}
DECIDE_AUTO, DECIDE_NEAREST, DECIDE_QPSK, DECIDE_BPSK = "auto", "nearest", "qpsk", "bpsk"      # the keys of DECIDE, as decision_rule() reports them
PAGE = mmap.PAGESIZE
C64, F32, I64, I32, I16, U8 = np.complex64, np.float32, np.int64, np.int32, np.int16, np.uint8


def _c64(a):
    """a host-side configuration array (taps, points, preambles) as C-contiguous complex64"""
    return np.ascontiguousarray(a, dtype=np.complex64)


def to_sc16(signal, peak=0.9 * 2048):
    """pygfdm's convert_to_sc16 (python/pygfdm/converter.py): the signal scaled so that its largest |re| or |im| equals `peak` (default: 0.9 of
    a 12-bit ADC's full scale), then truncated toward zero.  Returns int16 of shape (n, 2): columns I, Q.  The input is left as it is."""
    x = np.asarray(signal, dtype=np.complex128).ravel()
    if not 0 < peak <= np.iinfo(np.int16).max:
        raise ValueError("peak must lie in (0, 32767]")
    iq = np.stack((x.real, x.imag), axis=1)
    top = float(np.max(np.abs(iq))) if iq.size else 0.0
    if top > 0.0:
        iq = iq * (peak / top)
    return np.trunc(iq).astype(np.int16)


def from_sc16(iq):
    """pygfdm's convert_from_sc16: int16 I/Q of shape (n, 2) or flat (2n,) -> complex64 (float)I + j (float)Q, unscaled (exact)."""
    a = np.asarray(iq)
    if a.dtype != np.int16:
        raise TypeError("from_sc16 takes int16 I/Q values, not %s" % a.dtype)
    a = ops.sc16_pairs(a.shape, "iq", a.reshape)
    out = np.empty(a.shape[0], np.complex64)
    out.real = a[:, 0]
    out.imag = a[:, 1]
    return out


class generic_family_for_testing:
    """TEST HOOK: `with generic_family_for_testing(): h = Demodulator(...)` creates h on the generic kernel family even where the
    tuned row-lane family serves the shape (gfdm_hip_force_generic_family_for_testing); used by tests/ to run both families."""

    def __enter__(self):
        self._prev = lib().gfdm_hip_force_generic_family_for_testing(1)
        return self

    def __exit__(self, *exc):
        lib().gfdm_hip_force_generic_family_for_testing(self._prev)
        return False


JIT_OFF, JIT_IN_CONSTRUCTOR, JIT_BACKGROUND, JIT_AUTO = 0, 1, 2, 3


def set_jit(mode):
    """gfdm_hip_set_jit: when the row-lane kernels of a shape outside the compiled list are instantiated (hiprtc) -- JIT_OFF never (generic
    family), JIT_IN_CONSTRUCTOR, JIT_BACKGROUND (the handle starts on the generic family and switches over), JIT_AUTO (default: in the
    constructor when cached or quick, else in the background).  True / False mean JIT_IN_CONSTRUCTOR / JIT_OFF.  Returns the previous mode."""
    if mode is True:
        mode = JIT_IN_CONSTRUCTOR
    elif mode is False:
        mode = JIT_OFF
    return lib().gfdm_hip_set_jit(int(mode))


def precompile(timeslots, subcarriers, overlap, parts=0):
    """gfdm_hip_precompile: compile the tuned kernels of a shape into the disk cache without creating a handle (no GPU needed).
    parts: bit mask (receive 1, receive + IC 2, preamble-equalised receive 4, modulate 8, estimator 16, preamble-equalised receive
    straight from a capture -- demodulate_bursts -- 32), 0 = all."""
    _check(lib().gfdm_hip_precompile(int(timeslots), int(subcarriers), int(overlap), int(parts)))


def set_ic_matrix_cores(mode):
    """gfdm_hip_set_ic_matrix_cores: where handles created afterwards run the interference-cancellation rounds -- 0 / False vector ALU
    only, 1 / True (default) matrix cores where they are the faster form (subcarriers >= 128), 2 matrix cores wherever the form applies.
    Returns the previous mode."""
    return lib().gfdm_hip_set_ic_matrix_cores(int(mode))


def set_wide_access(enable):
    """gfdm_hip_set_wide_access: False keeps every later call of the 64-subcarrier row-lane kernels on 8-byte sample accesses; True (default)
    lets a call whose device pointers all lie on 16-byte boundaries move two samples per access.  Same results either way.  Returns the
    previous setting."""
    return lib().gfdm_hip_set_wide_access(int(bool(enable)))


def quiesce():
    """gfdm_hip_quiesce: drop the queued background builds of the run-time instantiated kernels, wait for the ones in flight (they finish
    their compile without touching the GPU).  Registered with atexit when the library is loaded."""
    lib().gfdm_hip_quiesce()


def build_id():
    """gfdm_hip_build_id: hash of the sources and flags the loaded library was built from."""
    return lib().gfdm_hip_build_id().decode()


HOST_ZERO_COPY, HOST_COPY_ENGINES = 0, 1


def set_host_pipeline(mode=-1, chunk_bytes=-1, depth=-1, copy_threads=-1, kernel_streams=-1):
    """gfdm_hip_set_host_pipeline: tuning of the *_host calls' bounce through pinned staging (negative / omitted = unchanged).  Returns the
    previous (mode, chunk_bytes, depth, copy_threads, kernel_streams)."""
    prev = get_host_pipeline()
    _check(lib().gfdm_hip_set_host_pipeline(int(mode), int(chunk_bytes), int(depth), int(copy_threads), int(kernel_streams)))
    return prev


def get_host_pipeline():
    m, c, d, t, k = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().gfdm_hip_get_host_pipeline(ctypes.byref(m), ctypes.byref(c), ctypes.byref(d), ctypes.byref(t), ctypes.byref(k)))
    return m.value, c.value, d.value, t.value, k.value


def host_call_stats():
    """What the calling thread's last *_host call did: dict(chunks, chunk_blocks, staged_bytes, direct_mask, mode, copy_threads)."""
    ch, cb, sb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    dm, md, ct = ctypes.c_uint(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().gfdm_hip_host_call_stats(ctypes.byref(ch), ctypes.byref(cb), ctypes.byref(sb), ctypes.byref(dm), ctypes.byref(md), ctypes.byref(ct)))
    ns = (ctypes.c_int64 * 5)()
    _check(lib().gfdm_hip_host_call_times(ns))
    return dict(chunks=ch.value, chunk_blocks=cb.value, staged_bytes=sb.value, direct_mask=dm.value, mode=md.value, copy_threads=ct.value,
                ns=dict(setup=ns[0], copy=ns[1], launch=ns[2], post=ns[3], wait=ns[4]))


class registered_host:
    """gfdm_hip_register_host as a context manager: `with registered_host(a, b): dem.demodulate(a, out=b)` -- the numpy arrays are pinned and
    mapped for the GPUs, *_host calls on them run in place (no bounce).  A long-lived buffer is registered once with register_host()."""

    def __init__(self, *arrays):
        self._arrays = arrays

    def __enter__(self):
        done = []
        try:
            for a in self._arrays:
                register_host(a)
                done.append(a)
        except Exception:
            for a in done:
                unregister_host(a)
            raise
        return self

    def __exit__(self, *exc):
        for a in self._arrays:
            unregister_host(a)
        return False


def aligned_empty(shape, dtype=np.complex64):
    """An uninitialised C-contiguous array that starts on a page boundary and owns its pages to the end of the last one: what register_host takes
    (gfdm_hip_register_host pins whole pages).  The backing buffer stays alive with the array."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    size = max(PAGE, -(-n // PAGE) * PAGE)
    buf = mmap.mmap(-1, size)                          # anonymous, page aligned, page granular
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def aligned_copy(array):
    out = aligned_empty(array.shape, array.dtype)
    out[...] = array
    return out


def register_host(array):
    """gfdm_hip_register_host on an array from aligned_empty / aligned_copy (or any array that starts on a page boundary and owns the rest of its last page)."""
    if array.ctypes.data % PAGE:
        raise ValueError("register_host: the array must start on a page boundary (gfdm_amd.aligned_empty / aligned_copy)")
    _check(lib().gfdm_hip_register_host(array.ctypes.data, -(-array.nbytes // PAGE) * PAGE))


def unregister_host(array):
    _check(lib().gfdm_hip_unregister_host(array.ctypes.data))


def set_dft_matrix_cores(mode):
    """gfdm_hip_set_dft_matrix_cores: where the generic kernel family of handles created afterwards runs its timeslot transforms on the
    matrix cores (f32 MFMA; from 32 timeslots on) -- 0 / False never, 1 / True (default) where that is the faster form, 2 wherever the form
    fits.  Returns the previous mode."""
    return lib().gfdm_hip_set_dft_matrix_cores(int(mode))


def _device_out(out, lead, refuse=False):
    """`out` of a call whose host flavour takes none: there it returns a new array whatever `out` is (refuse: it raises a TypeError)"""
    if ops.on_device(lead):
        return out
    if refuse and out is not None:
        raise TypeError("out is for device tensors; the numpy path returns a new array")
    return None


_ABSENT = object()                 # _blockwise: the entry point takes no second input


class _Kernel:
    """Shared plumbing: one handle on one GPU, and the one way a batched call reaches its host (numpy) or device (torch) entry point.
    A method checks and sizes its operands with _operands (ops), then hands their pointers to _run."""
    _destroy = None
    _dev = 0                       # GPU the handle was created on: every tensor and the stream of a call must belong to it

    def _sp(self, stream):
        """the stream of a device call as the C-ABI takes it: a torch stream, a raw hipStream_t, or None for the current one"""
        if stream is None:
            import torch
            return torch.cuda.current_stream(self._dev).cuda_stream      # the current stream of the HANDLE's GPU, not of torch's current one
        if hasattr(stream, "cuda_stream"):
            return stream.cuda_stream
        return int(stream)

    def __del__(self, loaded=_abi.loaded):              # (bound here: module globals may be gone when the interpreter shuts down)
        h = getattr(self, "_h", None)
        L = loaded()
        if h and L is not None and self._destroy:
            getattr(L, self._destroy)(h)
            self._h = None

    def _run(self, stem, lead, args, stream=None, scratch=None):
        """<stem>_device(handle, *args, [workspace,] stream) where the leading operand is a device tensor, else <stem>_host(handle, *args).
        Entry points with a device workspace give `scratch`: a callable that returns the workspace tensor of this call, or None for NULL."""
        if not ops.on_device(lead):
            return _check(getattr(lib(), stem + "_host")(self._h, *args))
        if scratch is not None:
            ws = scratch()                                     # alive until the call has returned
            args += (ops.ptr(ws),)
        _check(getattr(lib(), stem + "_device")(self._h, *args, self._sp(stream)))

    def _nblocks(self, size, what="Input"):
        n = self.block_size()
        if size % n:
            raise RuntimeError("%s vector size(%d) MUST be a multiple of block_size(%d)!" % (what, size, n))
        return size // n

    def _blockwise(self, stem, x, out, stream, vector=_ABSENT, vector_ok_none=False):
        """out = f(x[, vector]), all of x's size, any whole number of blocks: numpy in -> numpy out, a torch device tensor in -> `out` tensor,
        asynchronous on `stream`.  `out` may be an existing array (e.g. one registered with register_host: the call runs in place on it).
        vector: the second input of the entry points that have one (an equaliser, the other domain's symbols), None for NULL."""
        x, px, n = ops.bound(x, C64, "in", self._dev)
        host = not ops.on_device(x)
        nb = self._nblocks(n)
        pv = None
        if vector is not None and vector is not _ABSENT:
            vector, pv, nv = ops.bound(vector, C64, "extra input", self._dev, x)
            if nv != n:
                raise RuntimeError("Channel vector size(%d) MUST be equal to input size(%d)!" % (nv, n))
        elif vector is None and host and not vector_ok_none:   # (the device flavour reads a missing vector as "none")
            raise RuntimeError("missing input vector")
        if out is None:
            out = ops.result(x, x.shape, C64, self._dev)
            po = ops.ptr(out)
        else:
            if host and not isinstance(out, np.ndarray):
                raise TypeError("out must be a C-contiguous complex64 numpy array of the input's size")
            checked, po, n_out = ops.bound(out, C64, "out", self._dev, x)
            if host and (checked is not out or n_out != n):    # a host result is written in place: nothing bound() had to convert
                raise TypeError("out must be a C-contiguous complex64 numpy array of the input's size")
            if n_out != n:
                raise RuntimeError("out has %d elements, expected %d" % (n_out, n))
        self._run(stem, x, (po, px, nb) if vector is _ABSENT else (po, px, pv, nb), stream)
        return out

    def _batched(self, stem, x, n_in, n_out, args, stream, out):
        """(nblocks, n_out) = f(x of nblocks * n_in, *args); the host flavour gives one block that came 1-D back 1-D"""
        nb = ops.batches(x, n_in, "input size(%d) MUST be a multiple of %d!")
        x = ops.operand(x, C64, "in", self._dev)
        res = ops.result(x, (nb, n_out), C64, self._dev, _device_out(out, x))
        self._run(stem, x, (ops.ptr(res), ops.ptr(x), *args, nb), stream)
        return res[0] if (not ops.on_device(x) and x.ndim == 1 and nb == 1) else res


class _Receiver(_Kernel):
    """What Demodulator and AdvancedReceiver share: frames in / demapped symbols out, the fused channel estimator, bursts straight from a
    capture.  The C-ABI names are <_stem>_<name> for the settings and <_stem>_<_verb>_<call kind>[_sc16]_{host,device} for the calls."""
    _stem = None                   # "gfdm_hip_receiver" | "gfdm_hip_advanced_receiver"
    _verb = None                   # "demodulate" | "work"

    def _fn(self, name):
        return getattr(lib(), self._stem + "_" + name)

    def _call_stem(self, kind):
        return "%s_%s_%s" % (self._stem, self._verb, kind)

    @property
    def _bursts_prefix(self):
        return self._call_stem("bursts")

    def _layout(self, estimated, nout_arg):
        """(n_in, n_out, estimator fft_len) of one frames / estimated call, asked from the library (gfdm_hip_*_io_layout): it alone
        knows what its kernels write for this configuration, so no output buffer is ever sized from Python-side bookkeeping."""
        n_in, n_out, fft_len = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(self._fn("io_layout")(self._h, int(estimated), int(nout_arg), ctypes.byref(n_in), ctypes.byref(n_out), ctypes.byref(fft_len)))
        return n_in.value, n_out.value, fft_len.value

    # ---- raw frames in, demapped symbols out ----
    def configure_frames(self, frame_len, cp_len, subcarrier_map=None, per_timeslot=True):
        """Declare the frame layout once: frames of frame_len samples whose block starts cp_len samples in; with a
        subcarrier_map only the active subcarriers' symbols are emitted, in resource-mapper order."""
        smap = np.ascontiguousarray([] if subcarrier_map is None else subcarrier_map, dtype=np.int32)
        fn = self._fn("configure_frames")
        _check(fn(self._h, int(frame_len), int(cp_len), smap.ctypes.data if smap.size else None, smap.size, int(bool(per_timeslot))))

    def demodulate_frames(self, frames, f_eq=None, noutput_size=None, out=None, stream=None):
        """frames: nframes * frame_len samples; returns (nframes, noutput_size) symbols (all active symbols by default)."""
        nout_arg = -1 if noutput_size is None else int(noutput_size)
        frame_len, nout, _ = self._layout(False, nout_arg)
        N = self.block_size()
        x = ops.operand(frames, C64, "frames", self._dev)
        nb = ops.batches(x, frame_len, "frames size(%d) MUST be a multiple of frame_len(%d)!")
        e = None if f_eq is None else ops.operand(f_eq, C64, "f_eq", self._dev, x, "frames")
        if e is not None and ops.size(e) != nb * N:
            raise RuntimeError("Channel vector size(%d) MUST be equal to nframes * block_size(%d)!" % (ops.size(e), nb * N))
        res = ops.result(x, (nb, nout), C64, self._dev, _device_out(out, x))
        self._run(self._call_stem("frames"), x, (ops.ptr(res), ops.ptr(x), ops.ptr(e), nout_arg, nb), stream)
        return res

    # ---- channel estimator fused in front of the receiver ----
    def set_channel_estimator(self, estimator):
        """Attach a ChannelEstimator (or None): demodulate_estimated then derives the equaliser from each block's received preamble."""
        _check(self._fn("set_channel_estimator")(self._h, None if estimator is None else estimator._h))
        self._estimator = estimator                    # keeps the handle alive

    def demodulate_estimated(self, x, rx_preamble, preamble_stride=0, noutput_size=None, out=None, stream=None):
        """x: blocks (frames when configure_frames was called); rx_preamble: the received core preamble of every block, preamble b at
        b * preamble_stride (0 = packed, 2 * subcarriers).  Equals estimate_frame + demodulate_equalize, in one kernel."""
        if getattr(self, "_estimator", None) is None:
            raise ValueError("set_channel_estimator has not been called on this handle")
        nout_arg = -1 if noutput_size is None else int(noutput_size)
        n_in, nout, fft_len = self._layout(True, nout_arg)
        stride = int(preamble_stride) if preamble_stride else 2 * fft_len
        x = ops.operand(x, C64, "in", self._dev)
        nb = ops.batches(x, n_in, "Input size(%d) MUST be a multiple of %d!")
        pre = ops.operand(rx_preamble, C64, "rx_preamble", self._dev, x)
        ops.at_least(pre, (nb - 1) * stride + 2 * fft_len if nb else 0, "rx_preamble")
        res = ops.result(x, (nb, nout), C64, self._dev, _device_out(out, x))
        self._run(self._call_stem("estimated"), x, (ops.ptr(res), ops.ptr(x), ops.ptr(pre), int(preamble_stride), nout_arg, nb), stream)
        return res

    def demodulate_bursts(self, samples, offsets, sc_rot=None, count=None, backoff=0, preamble_offset=0, cfo_correction=True, noutput_size=None,
                          out=None, stream=None):
        """The bursts at `offsets` of the capture `samples`, demodulated straight from it: BurstExtractor.extract (offset - backoff, zero
        outside the capture, CFO rotation by sc_rot) as the load stage of demodulate_estimated, preamble at preamble_offset of each burst.
        Needs configure_frames and set_channel_estimator.  count (one int64, e.g. detect's): rows from count on are zeros.
        r = sync.detect(...) feeds it as demodulate_bursts(samples, r["frame_start"], r["sc_rot"], r["count"], ...).
        Torch device tensors run the device entry point (no allocation beyond `out`, no synchronisation), numpy arrays the host one.
        An int16 capture, shape (n, 2) or (2n,), is read as sc16 (the *_sc16_* entry points): bit-equal to the call on from_sc16(samples)."""
        s, slen, fmt = ops.capture(samples, self._dev)
        if getattr(self, "_estimator", None) is None:
            raise ValueError("set_channel_estimator has not been called on this handle")
        nout_arg = -1 if noutput_size is None else int(noutput_size)
        _, nout, _ = self._layout(True, nout_arg)
        off = ops.vector(offsets, I64, "offsets", self._dev, s, as_what="samples")
        n = ops.size(off)
        rot = None if sc_rot is None else ops.vector(sc_rot, C64, "sc_rot", self._dev, s, n, "samples")
        cnt = ops.count_arg(count, s, self._dev)
        res = ops.result(s, (n, nout), C64, self._dev, _device_out(out, s))
        self._run(self._bursts_prefix + fmt, s, (ops.ptr(res), ops.ptr(s), slen, ops.ptr(off), ops.ptr(rot), ops.ptr(cnt), int(backoff),
                                                       int(preamble_offset), int(bool(cfo_correction)), nout_arg, n), stream)
        return res


def _taps_arg(taps):
    t = _c64(np.asarray(taps).ravel())
    return t, t.ctypes.data, t.size


class Modulator(_Kernel):
    """gr::gfdm::modulator_kernel_cc (include/gfdm/modulator_kernel_cc.h:41-51) on the GPU."""
    _destroy = "gfdm_hip_modulator_destroy"

    def __init__(self, timeslots, subcarriers, overlap, taps, device=0):
        L = lib()
        t, tp, tn = _taps_arg(taps)
        h = ctypes.c_void_p()
        _check(L.gfdm_hip_modulator_create(ctypes.byref(h), timeslots, subcarriers, overlap, tp, tn, device))
        self._h = h
        self._dev = int(device)
        self._n = timeslots * subcarriers
        self._ntaps = tn

    def block_size(self):
        return self._n

    def kernel_name(self):
        return lib().gfdm_hip_modulator_kernel_name(self._h).decode()

    def filter_taps(self):
        out = np.empty(self._ntaps, np.complex64)
        _check(lib().gfdm_hip_modulator_filter_taps(self._h, out.ctypes.data))
        return out

    def modulate(self, x, out=None, stream=None):
        """numpy in -> numpy out (any whole number of blocks); torch CUDA tensor in -> `out` tensor, async on `stream`."""
        return self._blockwise("gfdm_hip_modulator_work", x, out, stream)


class Demodulator(_Receiver):
    """gr::gfdm::receiver_kernel_cc (include/gfdm/receiver_kernel_cc.h:52-89) on the GPU."""
    _destroy = "gfdm_hip_receiver_destroy"
    _stem, _verb = "gfdm_hip_receiver", "demodulate"

    def __init__(self, timeslots, subcarriers, overlap, taps, device=0):
        L = lib()
        t, tp, tn = _taps_arg(taps)
        h = ctypes.c_void_p()
        _check(L.gfdm_hip_receiver_create(ctypes.byref(h), timeslots, subcarriers, overlap, tp, tn, device))
        self._h = h
        self._dev = int(device)
        self._M, self._K, self._L = timeslots, subcarriers, overlap

    def timeslots(self):
        return lib().gfdm_hip_receiver_timeslots(self._h)

    def subcarriers(self):
        return lib().gfdm_hip_receiver_subcarriers(self._h)

    def overlap(self):
        return lib().gfdm_hip_receiver_overlap(self._h)

    def block_size(self):
        return self._M * self._K

    def kernel_name(self):
        return lib().gfdm_hip_receiver_kernel_name(self._h).decode()

    def filter_taps(self):
        out = np.empty(self._M * self._L, np.complex64)
        _check(lib().gfdm_hip_receiver_filter_taps(self._h, out.ctypes.data))
        return out

    def ic_filter_taps(self):
        out = np.empty(self._M, np.complex64)
        _check(lib().gfdm_hip_receiver_ic_filter_taps(self._h, out.ctypes.data))
        return out

    def demodulate(self, x, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_demodulate", x, out, stream, None, True)

    def demodulate_equalize(self, x, f_eq, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_demodulate", x, out, stream, f_eq)

    def fft_filter_downsample(self, x, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_fft_filter_downsample", x, out, stream, None, True)

    def fft_equalize_filter_downsample(self, x, f_eq, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_fft_filter_downsample", x, out, stream, f_eq)

    def transform_subcarriers_to_td(self, x, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_transform_subcarriers_to_td", x, out, stream)

    def cancel_sc_interference(self, td, fd, out=None, stream=None):
        return self._blockwise("gfdm_hip_receiver_cancel_sc_interference", td, out, stream, fd)


class AdvancedReceiver(_Receiver):
    """gr::gfdm::advanced_receiver_kernel_cc (include/gfdm/advanced_receiver_kernel_cc.h:37-78) on the GPU.

    The reference takes a gr::digital::constellation_sptr; here the constellation is its points() array plus a
    decision rule ('auto' picks the QPSK/BPSK sign tests when the points are those constellations).  Only GNU Radio's UNIT constellations
    -- (+-1 +-j)/sqrt 2 in the order --, +-, -+, ++ and -1, +1, every component within four float32 ulps -- take the sign tests (and the
    matrix-core cancellation rounds); scaled or rotated points are decided by the nearest-point rule over the points as given, also when
    'qpsk' / 'bpsk' was asked for.  decision_rule() reports the rule the handle runs."""
    _destroy = "gfdm_hip_advanced_receiver_destroy"
    _stem, _verb = "gfdm_hip_advanced_receiver", "work"

    def __init__(self, timeslots, subcarriers, overlap, taps, subcarrier_map, ic_iter, constellation_points,
                 do_phase_compensation=0, decision="auto", device=0):
        L = lib()
        t, tp, tn = _taps_arg(taps)
        smap = np.ascontiguousarray(subcarrier_map, dtype=np.int32)
        pts = _c64(np.asarray(constellation_points).ravel())
        h = ctypes.c_void_p()
        _check(L.gfdm_hip_advanced_receiver_create(ctypes.byref(h), timeslots, subcarriers, overlap, tp, tn,
                                                   smap.ctypes.data, smap.size, ic_iter, pts.ctypes.data, pts.size,
                                                   DECIDE[decision], do_phase_compensation, device))
        self._h = h
        self._dev = int(device)
        self._n = timeslots * subcarriers

    def block_size(self):
        return self._n

    def kernel_name(self):
        return lib().gfdm_hip_advanced_receiver_kernel_name(self._h).decode()

    def decision_rule(self):
        """'nearest' | 'qpsk' | 'bpsk': the rule this handle runs (gfdm_hip_advanced_receiver_decision)"""
        code = lib().gfdm_hip_advanced_receiver_decision(self._h)
        return {v: k for k, v in DECIDE.items() if k != "auto"}[code]

    def set_ic(self, ic_iter):
        _check(lib().gfdm_hip_advanced_receiver_set_ic(self._h, ic_iter))

    def get_ic(self):
        return lib().gfdm_hip_advanced_receiver_get_ic(self._h)

    def set_phase_compensation(self, enable):
        _check(lib().gfdm_hip_advanced_receiver_set_phase_compensation(self._h, enable))

    def get_phase_compensation(self):
        return lib().gfdm_hip_advanced_receiver_get_phase_compensation(self._h)

    def demodulate(self, x, out=None, stream=None):
        """generic_work: IC receiver without equaliser."""
        return self._blockwise("gfdm_hip_advanced_receiver_work", x, out, stream, None, True)

    def demodulate_equalize(self, x, f_eq, out=None, stream=None):
        """generic_work_equalize: one f_eq vector per block."""
        return self._blockwise("gfdm_hip_advanced_receiver_work", x, out, stream, f_eq, True)


class Transmitter(_Kernel):
    """gr::gfdm::transmitter_kernel (include/gfdm/transmitter_kernel.h:43-85) on the GPU: resource mapper -> modulator ->
    cyclic prefix/suffix with cyclic shift + window ramp -> preamble as ONE kernel, every cyclic shift ("port") at once."""
    _destroy = "gfdm_hip_transmitter_destroy"

    def __init__(self, timeslots, subcarriers, active_subcarriers, cp_len, cs_len, ramp_len, subcarrier_map, per_timeslot, overlap,
                 frequency_taps, window_taps, cyclic_shifts, preambles, device=0):
        L = lib()
        t, tp, tn = _taps_arg(frequency_taps)
        w = _c64(np.asarray(window_taps).ravel())
        smap = np.ascontiguousarray(subcarrier_map, dtype=np.int32)
        shifts = np.ascontiguousarray(cyclic_shifts, dtype=np.int32)
        pre = [np.asarray(p).ravel() for p in preambles]
        if len(pre) != shifts.size:
            raise ValueError("Number of cyclic shifts and number of preambles do not match!")
        if any(p.size != pre[0].size for p in pre):
            raise ValueError("All preambles must have equal size!")
        pre = _c64(np.stack(pre)) if pre else np.zeros((0, 0), np.complex64)
        h = ctypes.c_void_p()
        _check(L.gfdm_hip_transmitter_create(ctypes.byref(h), timeslots, subcarriers, active_subcarriers, cp_len, cs_len, ramp_len,
                                             smap.ctypes.data, smap.size, int(bool(per_timeslot)), overlap, tp, tn, w.ctypes.data, w.size,
                                             shifts.ctypes.data, shifts.size, pre.ctypes.data, pre.shape[1] if pre.size else 0, device))
        self._h = h
        self._dev = int(device)
        self._shifts = [int(x) for x in shifts]

    def input_vector_size(self):
        return lib().gfdm_hip_transmitter_input_vector_size(self._h)

    def output_vector_size(self):
        return lib().gfdm_hip_transmitter_output_vector_size(self._h)

    def block_size(self):
        return lib().gfdm_hip_transmitter_block_size(self._h)

    def cyclic_shifts(self):
        return list(self._shifts)

    def kernel_name(self):
        return lib().gfdm_hip_transmitter_kernel_name(self._h).decode()

    def _split(self, x, ninput_size):
        n = self.input_vector_size() if ninput_size is None else int(ninput_size)
        return n, ops.batches(x, n, "input size(%d) MUST be a multiple of ninput_size(%d)!")

    def transmit(self, symbols, ninput_size=None, n_ports=None, stream=None, outs=None):
        """All ports (or the first n_ports): list of (nblocks, output_vector_size) arrays / tensors, one per cyclic shift.
        `outs` (device path only): one tensor of nblocks * output_vector_size elements per port to write into."""
        n, nb = self._split(symbols, ninput_size)
        ports = len(self._shifts) if n_ports is None else n_ports
        F = self.output_vector_size()
        x = ops.operand(symbols, C64, "in", self._dev)
        if outs is None:
            outs = [None] * ports
        elif not ops.on_device(x):
            raise TypeError("outs is for device tensors; the numpy path returns new arrays")
        elif len(outs) != ports:
            raise RuntimeError("outs has %d tensors, expected one per port (%d)" % (len(outs), ports))
        outs = [ops.result(x, (nb, F), C64, self._dev, o, "outs[%d]" % i) for i, o in enumerate(outs)]
        arr = (ctypes.c_void_p * ports)(*[ops.ptr(o) for o in outs])
        self._run("gfdm_hip_transmitter_work", x, (arr, ports, ops.ptr(x), n, nb), stream)
        return outs

    def generic_work(self, symbols, ninput_size=None):
        """transmitter_kernel::generic_work: the frame of cyclic_shifts[0]."""
        return self.transmit(symbols, ninput_size, 1)[0]

    def modulate(self, symbols, ninput_size=None, stream=None, out=None):
        n, nb = self._split(symbols, ninput_size)
        N = self.block_size()
        x = ops.operand(symbols, C64, "in", self._dev)
        out = ops.result(x, (nb, N), C64, self._dev, _device_out(out, x, refuse=True))
        self._run("gfdm_hip_transmitter_modulate", x, (ops.ptr(out), ops.ptr(x), n, nb), stream)
        return out

    def add_frame(self, blocks, cyclic_shift, stream=None, out=None):
        N, F = self.block_size(), self.output_vector_size()
        x = ops.operand(blocks, C64, "in", self._dev)
        nb = ops.size(x) // N
        if ops.on_device(x):                                   # (the host flavour leaves an incomplete last block unread)
            ops.sized(x, nb * N, "in")
        out = ops.result(x, (nb, F), C64, self._dev, _device_out(out, x, refuse=True))
        self._run("gfdm_hip_transmitter_add_frame", x, (ops.ptr(out), ops.ptr(x), int(cyclic_shift), nb), stream)
        return out


class ResourceMapper(_Kernel):
    """gr::gfdm::resource_mapper_kernel_cc (include/gfdm/resource_mapper_kernel_cc.h:38-60; pybind name Resource_mapper): data symbols
    <-> the [subcarriers][timeslots] grid, stand-alone (Transmitter and the receivers' frame interface have it fused).  One block or a
    batch ([nblocks][size]); numpy in -> numpy out (host path), torch in -> torch out (device path, current stream unless given)."""
    _destroy = "gfdm_hip_resource_mapper_destroy"

    def __init__(self, timeslots, subcarriers, active_subcarriers, subcarrier_map, per_timeslot=True, device=0):
        smap = np.ascontiguousarray(subcarrier_map, dtype=np.int32)
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_resource_mapper_create(ctypes.byref(h), timeslots, subcarriers, active_subcarriers, smap.ctypes.data, smap.size,
                                                     int(bool(per_timeslot)), device))
        self._h = h
        self._dev = int(device)

    def block_size(self):
        return lib().gfdm_hip_resource_mapper_block_size(self._h)

    def frame_size(self):
        return lib().gfdm_hip_resource_mapper_frame_size(self._h)

    def map_to_resources(self, symbols, ninput_size=None, stream=None, out=None):
        """ninput_size symbols per block (default block_size) -> frame_size grid values per block, unfilled slots zero."""
        n = self.block_size() if ninput_size is None else int(ninput_size)
        if n == 0:
            raise RuntimeError("ninput_size 0: give the number of blocks through a [nblocks][0] input of the C-ABI instead")
        return self._batched("gfdm_hip_resource_mapper_map", symbols, n, self.frame_size(), (n,), stream, out)

    def demap_from_resources(self, grid, noutput_size=None, stream=None, out=None):
        n = self.block_size() if noutput_size is None else int(noutput_size)
        return self._batched("gfdm_hip_resource_mapper_demap", grid, self.frame_size(), n, (n,), stream, out)


class CyclicPrefixer(_Kernel):
    """gr::gfdm::add_cyclic_prefix_cc (include/gfdm/add_cyclic_prefix_cc.h:40-60; pybind name Cyclic_prefixer): cyclic prefix / suffix
    with cyclic shift + window ramps, and prefix removal, stand-alone.  One block or a batch; numpy -> numpy, torch -> torch."""
    _destroy = "gfdm_hip_cyclic_prefixer_destroy"

    def __init__(self, block_len, cp_len, cs_len, ramp_len, window_taps, cyclic_shift=0, device=0):
        w = _c64(np.asarray(window_taps).ravel())
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_cyclic_prefixer_create(ctypes.byref(h), block_len, cp_len, cs_len, ramp_len, w.ctypes.data, w.size, int(cyclic_shift),
                                                     device))
        self._h = h
        self._dev = int(device)

    def block_size(self):
        return lib().gfdm_hip_cyclic_prefixer_block_size(self._h)

    def frame_size(self):
        return lib().gfdm_hip_cyclic_prefixer_frame_size(self._h)

    def cyclic_shift(self):
        return lib().gfdm_hip_cyclic_prefixer_cyclic_shift(self._h)

    def add_cyclic_prefix(self, blocks, cyclic_shift=None, stream=None, out=None):
        s = self.cyclic_shift() if cyclic_shift is None else int(cyclic_shift)
        return self._batched("gfdm_hip_cyclic_prefixer_add", blocks, self.block_size(), self.frame_size(), (s,), stream, out)

    generic_work = add_cyclic_prefix

    def remove_cyclic_prefix(self, frames, stream=None, out=None):
        return self._batched("gfdm_hip_cyclic_prefixer_remove", frames, self.frame_size(), self.block_size(), (), stream, out)


class ChannelEstimator(_Kernel):
    """preamble_channel_estimator_cc (include/gfdm/preamble_channel_estimator_cc.h:45-78; pybind name
    Preamble_channel_estimator, python/bindings/preamble_channel_estimator_python.cc): received preamble -> frame channel
    estimate.  Every call takes one preamble / estimate or a batch of them ([nframes][len]); numpy in -> numpy out (host path),
    torch in -> torch out (device path, current stream unless given)."""
    _destroy = "gfdm_hip_channel_estimator_destroy"

    def __init__(self, timeslots, fft_len, active_subcarriers, is_dc_free, which_estimator, preamble, device=0):
        L = lib()
        p = _c64(preamble).ravel()
        h = ctypes.c_void_p()
        _check(L.gfdm_hip_channel_estimator_create(ctypes.byref(h), timeslots, fft_len, active_subcarriers, int(bool(is_dc_free)),
                                                   int(which_estimator), p.ctypes.data, p.size, device))
        self._h = h
        self._dev = int(device)

    def timeslots(self):
        return lib().gfdm_hip_channel_estimator_timeslots(self._h)

    def fft_len(self):
        return lib().gfdm_hip_channel_estimator_fft_len(self._h)

    subcarriers = fft_len                   # the pybind property is called `subcarriers` (preamble_channel_estimator_python.cc:52)

    def active_subcarriers(self):
        return lib().gfdm_hip_channel_estimator_active_subcarriers(self._h)

    def frame_len(self):
        return lib().gfdm_hip_channel_estimator_frame_len(self._h)

    def is_dc_free(self):
        return bool(lib().gfdm_hip_channel_estimator_is_dc_free(self._h))

    def filtered_len(self):
        return lib().gfdm_hip_channel_estimator_filtered_len(self._h)

    def kernel_name(self):
        return lib().gfdm_hip_channel_estimator_kernel_name(self._h).decode()

    def preamble_filter_taps(self):
        out = np.empty(9, np.float32)
        lib().gfdm_hip_channel_estimator_preamble_filter_taps(self._h, out.ctypes.data)
        return out

    def _lens(self):
        return {"rx": 2 * self.fft_len(), "est": self.fft_len(), "filt": self.filtered_len(), "frame": self.frame_len()}

    def _frames(self, x, n_in):
        """x checked, and its number of frames of n_in"""
        x = ops.operand(x, C64, "in", self._dev)
        return x, ops.batches(x, n_in, "Input size %d is not a multiple of %d")

    def _stage(self, name, x, n_in, n_out, stream):
        lens = self._lens()
        x, nf = self._frames(x, lens[n_in])
        n_out = lens[n_out]
        out = ops.result(x, (nf, n_out) if x.ndim > 1 or nf != 1 else (n_out,), C64, self._dev)
        self._run("gfdm_hip_channel_estimator_" + name, x, (ops.ptr(out), ops.ptr(x), nf), stream)
        return out

    def estimate_frame(self, rx_preamble, stream=None):
        return self._stage("estimate_frame", rx_preamble, "rx", "frame", stream)

    def estimate_preamble_channel(self, rx_preamble, stream=None):
        return self._stage("estimate_preamble_channel", rx_preamble, "rx", "est", stream)

    def filter_preamble_estimate(self, estimate, stream=None):
        return self._stage("filter_preamble_estimate", estimate, "est", "filt", stream)

    def interpolate_frame(self, filtered, stream=None):
        return self._stage("interpolate_frame", filtered, "filt", "frame", stream)

    def prepare_for_zf(self, frame_estimate, stream=None):
        return self._stage("prepare_for_zf", frame_estimate, "frame", "frame", stream)

    def estimate_snr(self, rx_preamble, stream=None):
        """(snr_lin, cnrs): scalars / [active] for one preamble, [nframes] / [nframes][active] for a batch."""
        x, nf = self._frames(rx_preamble, 2 * self.fft_len())
        snr = ops.result(x, (nf,), F32, self._dev)
        cnrs = ops.result(x, (nf, self.active_subcarriers()), F32, self._dev)
        self._run("gfdm_hip_channel_estimator_estimate_snr", x, (ops.ptr(snr), ops.ptr(cnrs), ops.ptr(x), nf), stream)
        if not ops.on_device(x) and x.ndim <= 1 and nf == 1:                    # (the device flavour keeps the batch shape)
            return float(snr[0]), cnrs[0]
        return snr, cnrs


def threshold_factor(false_alarm_prob):
    """pygfdm's calculate_threshold_factor (python/pygfdm/synchronization.py:239-243): sqrt(-(4 / pi) ln p), the detection threshold
    relative to the noise level for a false-alarm probability p < 1."""
    if not false_alarm_prob < 1.0:
        raise ValueError("False alarm probability MUST be smaller 1.0!")
    return float(np.sqrt(-(4 / np.pi) * np.log(false_alarm_prob)))


class BurstSync(_Kernel):
    """Preamble timing / CFO synchronisation: pygfdm's find_frame_start (python/pygfdm/synchronization.py:154-263) on every window
    stream[first + b * stride : ... + window_len] of a capture buffer (contract in include/gfdm_hip.h).  numpy samples -> numpy results
    (host path), a torch complex64 device tensor -> torch results on its device (device path, current stream unless given).  Every call that
    takes `samples` also takes an sc16 capture -- int16 I/Q of shape (n, 2) or (2n,), numpy or torch -- and reads it as it is (the *_sc16_*
    entry points): bit-equal to the call on from_sc16(samples)."""
    _destroy = "gfdm_hip_burst_sync_destroy"
    _OUT = (("frame_start", I64), ("coarse", I64), ("cfo", F32), ("metric", F32), ("sc_rot", C64))

    def __init__(self, fft_len, cp_len, core_preamble, window_len, device=0):
        p = _c64(core_preamble).ravel()
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_burst_sync_create(ctypes.byref(h), int(fft_len), int(cp_len), p.ctypes.data, p.size, int(window_len), device))
        self._h = h
        self._dev = int(device)

    def fft_len(self):
        return lib().gfdm_hip_burst_sync_fft_len(self._h)

    def cp_len(self):
        return lib().gfdm_hip_burst_sync_cp_len(self._h)

    def window_len(self):
        return lib().gfdm_hip_burst_sync_window_len(self._h)

    def corr_len(self):
        """ac / ic values per window: window_len - 2 fft_len"""
        return lib().gfdm_hip_burst_sync_corr_len(self._h)

    def _grid(self, first, stride, n_windows):
        return int(first), self.window_len() if stride is None else int(stride), int(n_windows)

    def _outputs(self, n, like):
        """the five per-window result arrays, of `like`'s kind, and their pointers in the C-ABI's order"""
        r = {key: ops.result(like, (n,), dtype, self._dev) for key, dtype in self._OUT}
        return r, [ops.ptr(a) for a in r.values()]

    def find_frame_start(self, samples, first=0, stride=None, n_windows=1, stream=None):
        """dict of per-window arrays: frame_start, coarse (stream indices, int64), cfo, metric (float32), sc_rot (complex64).
        stride defaults to window_len (windows back to back)."""
        s, n, fmt = ops.capture(samples, self._dev)
        first, stride, nw = self._grid(first, stride, n_windows)
        r, ptrs = self._outputs(nw, s)
        self._run("gfdm_hip_burst_sync_find_frame_start" + fmt, s, (*ptrs, ops.ptr(s), n, first, stride, nw), stream)
        return r

    def find_frame_start_at(self, samples, starts, stream=None):
        """find_frame_start on the windows samples[st : st + window_len], st = clamp(starts[w], 0, len(samples) - window_len): the same
        dict, bit-equal per window to find_frame_start(first=st).  starts: int64 (a device tensor when samples is one)."""
        s, n, fmt = ops.capture(samples, self._dev)
        st = ops.vector(starts, I64, "starts", self._dev, s, as_what="samples")
        nw = ops.size(st)
        r, ptrs = self._outputs(nw, s)
        self._run("gfdm_hip_burst_sync_find_frame_start_at" + fmt, s, (*ptrs, ops.ptr(s), n, ops.ptr(st), nw), stream)
        return r

    def detect(self, samples, threshold, min_distance, lead=None, max_bursts=None, stream=None):
        """Every burst of a stream (contract in include/gfdm_hip.h): peaks of ic over the whole stream that reach `threshold` and are
        the first maximum within +-min_distance, in ascending position; each one's window starts `lead` before it.  Returns a dict:
        count (total peaks found: int on the host path, a one-element int64 tensor on the device path, which does not synchronise) and
        the five find_frame_start arrays with max_bursts slots, those from min(count, max_bursts) on at frame_start = coarse = -1.
        Defaults: lead = cp_len + fft_len // 2, max_bursts = ceil(P / (min_distance + 1)), the most peaks P positions can hold."""
        s, n, fmt = ops.capture(samples, self._dev)
        L = lib()
        R = int(min_distance)
        lead = self.cp_len() + self.fft_len() // 2 if lead is None else int(lead)
        if max_bursts is None:
            max_bursts = max(0, -(-(n - 2 * self.fft_len()) // (max(R, 0) + 1)))
        nb = int(max_bursts)
        _check(L.gfdm_hip_burst_sync_detect_check(self.fft_len(), self.cp_len(), self.window_len(), n, threshold, R, lead, nb))
        r, ptrs = self._outputs(nb, s)
        host = not ops.on_device(s)
        count = np.zeros(1, np.int64) if host else ops.result(s, (1,), I64, self._dev)
        self._run("gfdm_hip_burst_sync_detect" + fmt, s, (ops.ptr(count), *ptrs, ops.ptr(s), n, threshold, R, lead, nb), stream,
                  scratch=lambda: ops.workspace(None, s, L.gfdm_hip_burst_sync_detect_workspace_bytes(self._h, n), self._dev))
        r["count"] = int(count[0]) if host else count
        return r

    def auto_correlate(self, samples, first=0, stride=None, n_windows=1, stream=None):
        """(ac, ic): [n_windows][corr_len] complex64 / float32 (pygfdm's auto_correlate_signal and abs_integrate)."""
        s, n, fmt = ops.capture(samples, self._dev)
        first, stride, nw = self._grid(first, stride, n_windows)
        P = self.corr_len()
        ac = ops.result(s, (nw, P), C64, self._dev)
        ic = ops.result(s, (nw, P), F32, self._dev)
        self._run("gfdm_hip_burst_sync_auto_correlate" + fmt, s, (ops.ptr(ac), ops.ptr(ic), ops.ptr(s), n, first, stride, nw), stream)
        return ac, ic


class BurstExtractor(_Kernel):
    """extract_burst_cc (lib/extract_burst_cc_impl.cc:72-242): burst_len samples from each offset - tag_backoff, scaled and (with CFO
    correction on) rotated by (conj(r) / |r|)^n; samples outside the stream read as zero.  numpy in -> numpy out (host path); torch
    device tensors in (samples, offsets int64, scale float32, sc_rot complex64) -> torch out (device path)."""
    _destroy = "gfdm_hip_burst_extractor_destroy"

    def __init__(self, burst_len, tag_backoff=0, activate_cfo_correction=True, device=0):
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_burst_extractor_create(ctypes.byref(h), int(burst_len), int(tag_backoff), int(bool(activate_cfo_correction)), device))
        self._h = h
        self._dev = int(device)

    def burst_len(self):
        return lib().gfdm_hip_burst_extractor_burst_len(self._h)

    def tag_backoff(self):
        return lib().gfdm_hip_burst_extractor_tag_backoff(self._h)

    def activate_cfo_compensation(self, activate):
        _check(lib().gfdm_hip_burst_extractor_set_cfo_correction(self._h, int(bool(activate))))

    set_cfo_correction = activate_cfo_compensation

    def cfo_correction(self):
        return bool(lib().gfdm_hip_burst_extractor_get_cfo_correction(self._h))

    def extract(self, samples, offsets, scale=None, sc_rot=None, stream=None):
        """[n][burst_len] bursts; offsets are tag positions in `samples` (the extractor subtracts tag_backoff).  An int16 capture, shape (n, 2)
        or (2n,), is read as sc16, unscaled: scale = 1 / 32768 gives unit full scale."""
        s, slen, fmt = ops.capture(samples, self._dev)
        B = self.burst_len()
        off = ops.vector(offsets, I64, "offsets", self._dev, s, as_what="samples")
        n = ops.size(off)
        sc = None if scale is None else ops.vector(scale, F32, "scale", self._dev, s, n, "samples")
        rot = None if sc_rot is None else ops.vector(sc_rot, C64, "sc_rot", self._dev, s, n, "samples")
        out = ops.result(s, (n, B), C64, self._dev)
        self._run("gfdm_hip_burst_extractor_extract" + fmt, s, (ops.ptr(out), ops.ptr(s), slen, ops.ptr(off), ops.ptr(sc), ops.ptr(rot), n), stream)
        return out


class BurstShaper(_Kernel):
    """Scaled frames in a TX stream (contract in include/gfdm_hip.h, gfdm_hip_burst_shaper): shape() is gr-gfdm's short_burst_shaper
    (lib/short_burst_shaper_impl.cc:161-182) on a batch of frames, place() puts the frames at given sample positions of a stream of
    out_len samples and writes the silence between them.  numpy frames -> numpy stream (host path); a torch complex64 device tensor ->
    a tensor on its device (device path, current stream unless given).  sc16=True writes int16 I/Q of shape (n, 2) -- what the burst
    calls read as a capture -- truncated and saturated; with `peak` the largest component of the scaled frames of the call goes to
    `peak` (to_sc16's rule, found on the device), without it the scale alone carries the gain.  `frames` may be a list of per-port
    arrays as Transmitter.transmit returns them: the result is then a list, one call (and one normalisation) per port."""
    _destroy = "gfdm_hip_burst_shaper_destroy"

    def __init__(self, frame_len, pre_padding=0, post_padding=0, scale=1.0, device=0):
        h = ctypes.c_void_p()
        sc = complex(scale)
        _check(lib().gfdm_hip_burst_shaper_create(ctypes.byref(h), int(frame_len), int(pre_padding), int(post_padding), sc.real, sc.imag, device))
        self._h = h
        self._dev = int(device)

    def frame_len(self):
        return lib().gfdm_hip_burst_shaper_frame_len(self._h)

    def pre_padding(self):
        return lib().gfdm_hip_burst_shaper_pre_padding(self._h)

    def post_padding(self):
        return lib().gfdm_hip_burst_shaper_post_padding(self._h)

    def slot_len(self):
        """samples per burst of shape(): pre_padding + frame_len + post_padding"""
        return self.pre_padding() + self.frame_len() + self.post_padding()

    def scale(self):
        v = (ctypes.c_float * 2)()
        _check(lib().gfdm_hip_burst_shaper_scale(self._h, v))
        return complex(v[0], v[1])

    def workspace_bytes(self, n_bursts, out_len):
        """bytes of device scratch a device call on n_bursts frames and out_len samples needs (used by normalised sc16 output only)"""
        n = lib().gfdm_hip_burst_shaper_workspace_bytes(self._h, int(n_bursts), int(out_len))
        if n < 0:
            _check(n)
        return n

    @staticmethod
    def _ports(call, frames, out):
        """`frames` a list of per-port arrays: call(frames[p], out[p]) for every port, `out` (if given) holding one array per port"""
        if out is not None and len(out) != len(frames):
            raise ValueError("out must hold one array per port")
        return [call(f, None if out is None else out[p]) for p, f in enumerate(frames)]

    def _arguments(self, frames, out, sc16, peak):
        """(frames, peak) as the C-ABI takes them: what can be said of frames, out and peak without the handle is raised here"""
        if peak is None:
            pk = 0.0
        elif not sc16:
            raise ValueError("peak normalises sc16 output: pass sc16=True (complex64 output is scaled by `scale` alone)")
        elif not 0 < peak <= 32767:
            raise ValueError("peak must lie in (0, 32767]")
        else:
            pk = float(peak)
        frames = ops.operand(frames, C64, "frames", self._dev, floating=True)
        ops.check_result(out, frames, I16 if sc16 else C64, self._dev, as_what="frames")
        return frames, pk

    def _geometry(self, pk, n, out_len):
        """the library's own check of a call's geometry: before anything else is said of starts and count, or allocated"""
        _check(lib().gfdm_hip_burst_shaper_check(self.frame_len(), self.pre_padding(), self.post_padding(), pk, n, out_len))

    def _call(self, name, frames, n, out_len, sc16, pk, out, stream, workspace, *args):
        """make the result of out_len samples and run gfdm_hip_burst_shaper_<name>[_sc16](handle, result, *args[, peak])"""
        res = ops.stream_result(frames, out_len, sc16, self._dev, out, "frames")
        self._run("gfdm_hip_burst_shaper_" + name + ("_sc16" if sc16 else ""), frames, (ops.ptr(res),) + args + ((pk,) if sc16 else ()), stream,
                  scratch=lambda: ops.workspace(workspace, frames, self.workspace_bytes(n, out_len), self._dev) if pk else None)
        return res

    def shape(self, frames, sc16=False, peak=None, out=None, stream=None, workspace=None):
        """n_bursts * slot_len() samples: every frame scaled, behind pre_padding and in front of post_padding zeros.  workspace (device path,
        normalised sc16 only): a uint8 tensor of workspace_bytes() to use instead of a new one; afterwards its first two floats are the gain
        and the largest component found."""
        if isinstance(frames, (list, tuple)):
            return self._ports(lambda f, out: self.shape(f, sc16, peak, out, stream, workspace), frames, out)
        frames, pk = self._arguments(frames, out, sc16, peak)
        n = ops.batches(frames, self.frame_len(), "frames size(%d) MUST be a multiple of frame_len(%d)!")
        self._geometry(pk, n, n * self.slot_len())
        return self._call("shape", frames, n, n * self.slot_len(), sc16, pk, out, stream, workspace, ops.ptr(frames), n)

    def place(self, frames, starts, out_len, count=None, sc16=False, peak=None, out=None, stream=None, workspace=None):
        """out_len samples: frame b from sample starts[b] on (starts ascending, int64; a device tensor when frames is one), zeros
        elsewhere.  count (an int, or on the device path a one-element int64 tensor such as detect's) limits the call to the first
        count frames; it is clamped to [0, n_bursts].  workspace: as in shape()."""
        if isinstance(frames, (list, tuple)):
            return self._ports(lambda f, out: self.place(f, starts, out_len, count, sc16, peak, out, stream, workspace), frames, out)
        frames, pk = self._arguments(frames, out, sc16, peak)
        st = ops.vector(starts, I64, "starts", self._dev, frames, as_what="frames")
        n = ops.batches(frames, self.frame_len(), "frames size(%d) MUST be a multiple of frame_len(%d)!")
        out_len = int(out_len)
        self._geometry(pk, n, out_len)
        ops.sized(st, n, "starts")
        cnt = ops.count_arg(count, frames, self._dev)
        return self._call("place", frames, n, out_len, sc16, pk, out, stream, workspace, out_len, ops.ptr(frames), ops.ptr(st), ops.ptr(cnt), n)


class _Rows(_Kernel):
    """What SymbolMapper and LinkMeter share: a constellation handle of the C-ABI kind `_kind`, calls on rows of symbols."""
    _kind = None                   # "gfdm_hip_symbol_mapper" | "gfdm_hip_link_meter"

    def __init__(self, points, decision=DECIDE_AUTO, device=0):
        pts = _c64(np.asarray(points).ravel())
        h = ctypes.c_void_p()
        _check(getattr(lib(), self._kind + "_create")(ctypes.byref(h), pts.ctypes.data, pts.size, DECIDE.get(decision, decision), device))
        self._h = h
        self._dev = int(device)
        self._k = getattr(lib(), self._kind + "_bits_per_symbol")(h)

    def bits_per_symbol(self):
        return self._k

    def decision_rule(self):
        """'nearest' | 'qpsk' | 'bpsk': the rule SymbolMapper.decode and LinkMeter.measure decide by (gfdm_hip_*_decision)"""
        code = getattr(lib(), self._kind + "_decision")(self._h)
        return {v: k for k, v in DECIDE.items() if k != "auto"}[code]

    def row_bytes(self, n_sym):
        """bytes of a packed row of n_sym symbols: ceil(n_sym * k / 8)"""
        return _bytes(getattr(lib(), self._kind + "_row_bytes")(self._h, int(n_sym)))


def _bytes(n):
    """a byte count of the C-ABI: negative values are its status codes"""
    if n < 0:
        _check(n)
    return n


class SymbolMapper(_Rows):
    """Payload bytes <-> constellation symbols, and max-log soft bits (contract in include/gfdm_hip.h, gfdm_hip_symbol_mapper): map() is
    repack_bits_bb(8 -> k, MSB first) + chunks_to_symbols in front of Transmitter.transmit, decode() is constellation_decoder_cb +
    repack_bits_bb(k -> 8) behind demodulate_frames / demodulate_estimated / demodulate_bursts, soft() feeds a decoder instead.  Rows are
    frames or bursts: symbols are (n_rows, n_sym), packed bytes (n_rows, row_bytes(n_sym)), soft bits (n_rows, n_sym * k); a 1-D input is
    one row and gives a 1-D result.  numpy arrays run the host flavour; torch device tensors (uint8 / complex64 / float32) the device
    flavour on the current stream unless given.  count (an int, or on the device path a one-element int64 tensor such as detect's) limits
    the call to the first count rows, the rest is written as zeros; it is clamped to [0, n_rows]."""
    _destroy = "gfdm_hip_symbol_mapper_destroy"
    _kind = "gfdm_hip_symbol_mapper"

    def points(self):
        """the points as given to the constructor (complex64, bit for bit)"""
        p = np.empty(lib().gfdm_hip_symbol_mapper_n_points(self._h), np.complex64)
        _check(lib().gfdm_hip_symbol_mapper_points(self._h, p.ctypes.data))
        return p

    def _symbols(self, symbols):
        symbols, n_rows, n_sym, flat = ops.rows(symbols, C64, "symbols", self._dev)
        _check(lib().gfdm_hip_symbol_mapper_check(1 << self._k, n_sym, n_rows))
        return symbols, n_rows, n_sym, flat

    def _call(self, name, x, extra, width, dtype, flat, count, out, n_sym, n_rows, stream):
        res = ops.result(x, (width,) if flat else (n_rows, width), dtype, self._dev, out, off_device=RuntimeError)
        cnt = ops.count_arg(count, x, self._dev)
        _check(lib().gfdm_hip_symbol_mapper_check(1 << self._k, n_sym, n_rows))
        self._run("gfdm_hip_symbol_mapper_" + name, x, (ops.ptr(res), ops.ptr(x), *extra, ops.ptr(cnt), n_sym, n_rows), stream)
        return res

    def map(self, data, n_sym, count=None, out=None, stream=None):
        """packed bytes (n_rows, row_bytes(n_sym)) uint8 -> symbols (n_rows, n_sym) complex64: points[index], a bit copy"""
        n_sym = int(n_sym)
        data, n_rows, _, flat = ops.rows(data, U8, "data", self._dev, self.row_bytes(n_sym))
        return self._call("map", data, (), n_sym, C64, flat, count, out, n_sym, n_rows, stream)

    def decode(self, symbols, count=None, out=None, stream=None):
        """symbols (n_rows, n_sym) complex64 -> packed bytes (n_rows, row_bytes(n_sym)) uint8, by the rule of decision_rule()"""
        symbols, n_rows, n_sym, flat = self._symbols(symbols)
        return self._call("decode", symbols, (), self.row_bytes(n_sym), U8, flat, count, out, n_sym, n_rows, stream)

    def soft(self, symbols, scale=None, count=None, out=None, stream=None):
        """symbols (n_rows, n_sym) complex64 -> max-log LLRs (n_rows, n_sym * k) float32, positive for bit 0; scale: float32 (n_rows,), one
        factor per row (typically 1 / sigma^2), a device tensor when symbols is one"""
        symbols, n_rows, n_sym, flat = self._symbols(symbols)
        sc = None if scale is None else ops.vector(scale, F32, "scale", self._dev, symbols, n_rows, "symbols")
        return self._call("soft", symbols, (ops.ptr(sc),), n_sym * self._k, F32, flat, count, out, n_sym, n_rows, stream)


def awgn_noise_voltage(signal, snr_db, rate=1.0):
    """ChannelModel's noise_voltage for `snr_db` on `signal`: sqrt(2 * v), v pygfdm's calculate_awgn_noise_variance (python/pygfdm/utils.py:
    106-110, the variance PER COMPONENT: average sample energy / (2 * rate * 10^(snr_db / 10))) -- the noise power of the channel model is
    noise_voltage^2 = 2 v.  `signal` is a numpy array or a torch tensor; the energy of a tensor is summed on its device."""
    if ops.is_tensor(signal):
        flat = signal.reshape(-1)
        energy, n = float((flat.real.double() ** 2 + flat.imag.double() ** 2).sum().item()) if flat.is_complex() else float((flat.double() ** 2).sum().item()), flat.numel()
    else:
        flat = np.asarray(signal).ravel()
        energy, n = float(np.sum(flat.real.astype(np.float64) ** 2 + flat.imag.astype(np.float64) ** 2)), flat.size
    if n == 0:
        raise ValueError("signal is empty")
    if not rate > 0:
        raise ValueError("rate must be > 0")
    variance = (energy / n) / (2 * rate * 10.0 ** (snr_db / 10.0))
    return float(np.sqrt(2.0 * variance))


def _apply_stream(kernel, stem, x, history, offset, sc16, gain, out, stream):
    """what ChannelModel.apply, FadingModel.apply and AmplifierModel.apply share: <stem>[_sc16] on the history + n complex64 samples of x,
    n samples out; offset None: the call takes none"""
    x = ops.operand(x, C64, "x", kernel._dev, floating=True)
    ops.check_result(out, x, I16 if sc16 else C64, kernel._dev, as_what="x")
    history = int(history)
    size = ops.size(x)
    if history < 0 or history > size:
        raise ValueError("history(%d) must lie in 0 .. the size of x(%d)" % (history, size))
    n = size - history
    res = ops.stream_result(x, n, sc16, kernel._dev, out, "x")
    where = () if offset is None else (int(offset),)
    kernel._run(stem + ("_sc16" if sc16 else ""), x, (ops.ptr(res), ops.ptr(x) + 8 * history, n, history) + where + ((float(gain),) if sc16 else ()), stream)
    return res


class ChannelModel(_Kernel):
    """Multipath, frequency offset and noise on a stream, on the device (contract in include/gfdm_hip.h, gfdm_hip_channel_model): GNU
    Radio's channels.channel_model in its argument order, between BurstShaper.place and BurstSync.detect.  y = FIR(taps) of x, times
    exp(j 2 pi frequency_offset n), plus white Gaussian noise of power noise_voltage^2 that is a pure function of (noise_seed, absolute
    sample index).  epsilon (the timing offset) must be 1.0: resampling is not part of this, Resampler in front of apply is.  The taps are fixed; frequency_offset,
    noise_voltage and seed have setters, and a captured graph keeps the values it was captured with."""
    _destroy = "gfdm_hip_channel_model_destroy"

    def __init__(self, noise_voltage=0.0, frequency_offset=0.0, epsilon=1.0, taps=(1,), noise_seed=0, device=None):
        if float(epsilon) != 1.0:
            raise ValueError("epsilon must be 1.0: the timing offset (resampling) of channel_model is not part of this")
        t = _c64(np.asarray(taps).ravel())
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        _check(lib().gfdm_hip_channel_model_create(ctypes.byref(h), t.ctypes.data, t.size, float(frequency_offset), float(noise_voltage),
                                                   int(noise_seed) & 0xFFFFFFFFFFFFFFFF, dev))
        self._h = h
        self._dev = dev

    def n_taps(self):
        return lib().gfdm_hip_channel_model_n_taps(self._h)

    def taps(self):
        """the taps as given to the constructor (complex64, bit for bit)"""
        t = np.empty(self.n_taps(), np.complex64)
        _check(lib().gfdm_hip_channel_model_taps(self._h, t.ctypes.data))
        return t

    def frequency_offset(self):
        v = ctypes.c_double()
        _check(lib().gfdm_hip_channel_model_frequency_offset(self._h, ctypes.byref(v)))
        return v.value

    def noise_voltage(self):
        v = ctypes.c_double()
        _check(lib().gfdm_hip_channel_model_noise_voltage(self._h, ctypes.byref(v)))
        return v.value

    def seed(self):
        v = ctypes.c_uint64()
        _check(lib().gfdm_hip_channel_model_seed(self._h, ctypes.byref(v)))
        return v.value

    def set_frequency_offset(self, frequency_offset):
        _check(lib().gfdm_hip_channel_model_set_frequency_offset(self._h, float(frequency_offset)))

    def set_noise_voltage(self, noise_voltage):
        _check(lib().gfdm_hip_channel_model_set_noise_voltage(self._h, float(noise_voltage)))

    def set_seed(self, noise_seed):
        _check(lib().gfdm_hip_channel_model_set_seed(self._h, int(noise_seed) & 0xFFFFFFFFFFFFFFFF))

    def apply(self, x, history=0, offset=0, sc16=False, gain=1.0, out=None, stream=None):
        """x holds history + n samples, the result has n: sample i of the result is the channel's output for x[history + i], whose absolute
        index is offset + i; the first `history` samples are the FIR's past (GNU Radio's history; what lies before them is zeros).  A stream
        cut into calls gives the samples of one call when each piece passes history = min(n_taps - 1, samples before it) and its offset.
        numpy x -> numpy result (host path); a torch complex64 device tensor -> a tensor on its device (device path, current stream unless
        given).  sc16=True writes int16 I/Q of shape (n, 2), truncated and saturated, of y * gain."""
        if not sc16 and float(gain) != 1.0:
            raise ValueError("gain scales sc16 output: pass sc16=True (complex64 output is not scaled)")
        return _apply_stream(self, "gfdm_hip_channel_model_apply", x, history, offset, sc16, gain, out, stream)


_U64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z):
    """the splitmix64 finaliser on a Python int below 2^64 (what synth._mix64 does on tensors)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def _fading_hash(seed, p, s, w):
    return _mix64((_mix64(((int(seed) & _U64) * _GOLDEN + (p << 40 | s << 8 | w)) & _U64) + _GOLDEN) & _U64)


def fading_taps(delays, mags, ntaps):
    """FadingModel's delay-line table: c[p][k] = mags[p] * sinc(k - delays[p]), float32 of shape (len(delays), ntaps), computed in float64;
    delays in samples within [0, ntaps - 1] (an integer delay gives a one-hot row times mags[p] exactly).  The truncated sinc of GNU
    Radio's selective_fading_model, without its window; numpy alone, no device."""
    d = np.atleast_1d(np.asarray(delays, np.float64))
    m = np.atleast_1d(np.asarray(mags, np.float64))
    T = int(ntaps)
    if d.ndim != 1 or m.shape != d.shape or d.size < 1:
        raise ValueError("delays and mags must be two vectors of one length >= 1")
    if T < 1 or T > 64:
        raise ValueError("ntaps(%d) must lie in 1 .. 64" % T)
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(m))) or d.min() < 0 or d.max() > T - 1:
        raise ValueError("delays must be finite and lie in [0, ntaps - 1], mags must be finite")
    u = np.arange(T)[None, :] - d[:, None]
    s = np.sinc(u)
    whole = u == np.rint(u)
    s[whole] = (u[whole] == 0).astype(np.float64)
    return (m[:, None] * s).astype(np.float32)


def fading_sinusoids(n_paths, N, fDTs, seed, los=False, k_factor=0.0):
    """FadingModel's sinusoid tables (A float32, F int64, phase0 uint64), each of shape (n_paths, N + (1 if los else 0)): a stratified
    Monte-Carlo Clarke model.  With hash(seed, p, s, w) = mix(mix(seed * 0x9E3779B97F4A7C15 + (p << 40 | s << 8 | w)) + 0x9E3779B97F4A7C15)
    in uint64 wrap-around, mix the splitmix64 finaliser: scatter sinusoid s of path p arrives at alpha = 2 pi (s + u) / N with
    u = hash(seed, p, s, 0) 2^-64, F = rint(fDTs cos(alpha) 2^64), phase0 = hash(seed, p, s, 1), A = sqrt(1 / (N (1 + k))), k = k_factor on
    path 0 when los is set and 0 otherwise.  With los every path has sinusoid number N: on path 0 at the angle 2 pi hash(seed, 0, N, 0) 2^-64
    with phase hash(seed, 0, N, 1) and A = sqrt(k / (k + 1)), on the other paths A = 0.  The ensemble autocorrelation of a path is
    J0(2 pi fDTs tau) and E|g|^2 = 1.  Not bit-compatible with GNU Radio's fader (unpinned); numpy alone, no device."""
    P, N, fd, k_factor = int(n_paths), int(N), float(fDTs), float(k_factor)
    S = N + (1 if los else 0)
    if P < 1 or P > 8:
        raise ValueError("n_paths(%d) must lie in 1 .. 8" % P)
    if N < 1 or S > 17:
        raise ValueError("N(%d) must be >= 1 and give at most 17 sinusoids a path" % N)
    if not np.isfinite(fd) or abs(fd) > 0.5:
        raise ValueError("fDTs must be finite and lie in [-0.5, 0.5] cycles per sample")
    if not np.isfinite(k_factor) or k_factor < 0:
        raise ValueError("k_factor must be finite and >= 0")
    A, F, ph = np.zeros((P, S), np.float32), np.zeros((P, S), np.int64), np.zeros((P, S), np.uint64)

    def freq(alpha):
        return min(int(np.rint(fd * np.cos(alpha) * 2.0 ** 64)), (1 << 63) - 1)          # float64; +0.5 cycles is the one value past int64

    for p in range(P):
        k = k_factor if (los and p == 0) else 0.0
        for s in range(N):
            u = _fading_hash(seed, p, s, 0) * 2.0 ** -64
            F[p, s] = freq(2 * np.pi * (s + u) / N)
            ph[p, s] = _fading_hash(seed, p, s, 1)
            A[p, s] = np.sqrt(1.0 / (N * (1.0 + k)))
        if los and p == 0:
            F[p, N] = freq(2 * np.pi * (_fading_hash(seed, 0, N, 0) * 2.0 ** -64))
            ph[p, N] = _fading_hash(seed, 0, N, 1)
            A[p, N] = np.sqrt(k / (k + 1.0))
    return A, F, ph


class FadingModel(_Kernel):
    """Time-varying multipath on a stream, on the device (contract in include/gfdm_hip.h, gfdm_hip_fading_model): GNU Radio's
    channels.selective_fading_model in its argument order -- N sinusoids a path, fDTs the maximum Doppler in cycles per sample, LOS / K a
    Rician first path, delays and mags of the paths, ntaps of the delay lines -- in front of ChannelModel.apply(taps = [1]), which keeps
    the frequency offset and the noise.  y[i] = sum_p g_p(offset + i) * sum_k c[p][k] x[i - k] with g_p a sum of sinusoids of the absolute
    index, from fading_sinusoids(len(delays), N, fDTs, seed, LOS, K) and fading_taps(delays, mags, ntaps); from_tables takes the four
    tables as they are.  Everything is fixed at create: another Doppler is another FadingModel.  Not bit-compatible with GNU Radio's
    fader (unpinned)."""
    _destroy = "gfdm_hip_fading_model_destroy"

    def __init__(self, N=8, fDTs=0.0, LOS=False, K=4.0, seed=0, delays=(0.0,), mags=(1.0,), ntaps=1, device=None):
        c = fading_taps(delays, mags, ntaps)
        A, F, ph = fading_sinusoids(c.shape[0], N, fDTs, seed, bool(LOS), K)
        self._create(c, A, F, ph, device)

    @classmethod
    def from_tables(cls, c, A, F, phase0, device=None):
        """c float32 (P, T), A float32 (P, S), F int64 (P, S) in 2^-64 cycles per sample, phase0 uint64 (P, S) in 2^-64 turns"""
        self = object.__new__(cls)
        self._create(c, A, F, phase0, device)
        return self

    def _create(self, c, A, F, ph, device):
        c, A = np.ascontiguousarray(c, dtype=np.float32), np.ascontiguousarray(A, dtype=np.float32)
        F, ph = np.asarray(F), np.asarray(ph)
        if F.dtype.kind not in "iu" or ph.dtype.kind not in "iu":
            raise TypeError("F and phase0 must be integers (2^-64 cycles per sample, 2^-64 turns), not %s and %s" % (F.dtype, ph.dtype))
        F, ph = np.ascontiguousarray(F.astype(np.int64)), np.ascontiguousarray(ph.astype(np.uint64))       # (two's complement either way)
        if c.ndim != 2 or A.ndim != 2 or c.shape[0] != A.shape[0] or F.shape != A.shape or ph.shape != A.shape:
            raise ValueError("the tables must have the shapes c (P, T) and A, F, phase0 (P, S), not %s, %s, %s, %s"
                             % (tuple(c.shape), tuple(A.shape), tuple(F.shape), tuple(ph.shape)))
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        _check(lib().gfdm_hip_fading_model_create(ctypes.byref(h), c.ctypes.data, A.ctypes.data, F.ctypes.data, ph.ctypes.data, A.shape[0], A.shape[1],
                                                  c.shape[1], dev))
        self._h = h
        self._dev = dev

    def n_paths(self):
        return lib().gfdm_hip_fading_model_n_paths(self._h)

    def n_sinusoids(self):
        return lib().gfdm_hip_fading_model_n_sinusoids(self._h)

    def n_taps(self):
        return lib().gfdm_hip_fading_model_n_taps(self._h)

    def _table(self, name, width, dtype):
        t = np.empty((self.n_paths(), width), dtype)
        _check(getattr(lib(), "gfdm_hip_fading_model_" + name)(self._h, t.ctypes.data))
        return t

    def taps(self):
        """c as given at create (float32 (P, T), bit for bit)"""
        return self._table("taps", self.n_taps(), np.float32)

    def amplitudes(self):
        return self._table("amplitudes", self.n_sinusoids(), np.float32)

    def frequencies(self):
        return self._table("frequencies", self.n_sinusoids(), np.int64)

    def phases(self):
        return self._table("phases", self.n_sinusoids(), np.uint64)

    def apply(self, x, history=0, offset=0, out=None, gain=1.0, sc16=None, stream=None):
        """x holds history + n samples, the result has n: sample i of the result is the faded x[history + i], whose absolute index is
        offset + i; the first `history` samples are the delay lines' past (what lies before them is zeros).  A stream cut into calls
        gives the samples of one call, to the bit, when each piece passes history = min(n_taps - 1, samples before it) and its offset.
        numpy x -> numpy result (host path); a torch complex64 device tensor -> a tensor on its device (device path, current stream
        unless given).  An int16 `out` (or sc16=True) selects int16 I/Q of shape (n, 2), truncated and saturated, of y * gain."""
        if sc16 is None:
            sc16 = out is not None and str(getattr(out, "dtype", "")).replace("torch.", "") == "int16"
        sc16 = bool(sc16)
        if not sc16 and float(gain) != 1.0:
            raise ValueError("gain scales sc16 output: pass an int16 out or sc16=True (complex64 output is not scaled)")
        return _apply_stream(self, "gfdm_hip_fading_model_apply", x, history, offset, sc16, gain, out, stream)


AMPLIFIER_KINDS = {"clip": 0, "rapp": 1, "saleh": 2, "poly": 3}
_AMPLIFIER_PARAMS = {"clip": ("A",), "rapp": ("g", "A", "p"), "saleh": ("aa", "ba", "ap", "bp"), "poly": ()}


def _amplifier_spec(kind, params, c):
    """(kind name, float64 params as the handle keeps them (rounded to float32), complex64 c (Q, K) or None), checked as far as numpy can"""
    name = {v: k for k, v in AMPLIFIER_KINDS.items()}.get(kind, kind)
    if name not in AMPLIFIER_KINDS:
        raise ValueError("kind must be one of %s" % ", ".join(sorted(AMPLIFIER_KINDS)))
    p = np.asarray(params, dtype=np.float64).ravel()
    if p.size != len(_AMPLIFIER_PARAMS[name]):
        raise ValueError("kind %s takes the parameters (%s), got %d" % (name, ", ".join(_AMPLIFIER_PARAMS[name]), p.size))
    with np.errstate(over="ignore"):
        p = p.astype(np.float32).astype(np.float64)
    if name != "poly":
        if c is not None:
            raise ValueError("kind %s takes no coefficients" % name)
        return name, p, None
    c = np.asarray(c)
    if c.ndim == 1:
        c = c[None, :]                                   # one delay: the memoryless polynomial
    if c.ndim != 2:
        raise ValueError("c must have the shape (n_delays, n_orders)")
    return name, p, _c64(c).reshape(c.shape)


def amplifier_curve(model_or_params, amplitudes):
    """(am, pm): the output amplitude and the phase shift in radians of a kind for the input amplitudes |u| (behind the drive), float64
    arrays of amplitudes' shape; numpy alone, no device.  model_or_params: an AmplifierModel, or (kind, *params) with kind "clip" (A),
    "rapp" (g, A, p), "saleh" (aa, ba, ap, bp) or ("poly", c) -- for a memory polynomial the curve of a constant envelope, where every
    delay sees the same sample."""
    if isinstance(model_or_params, AmplifierModel):
        name, p, c = model_or_params.kind(), model_or_params.params(), model_or_params.coefficients()
    else:
        kind, rest = model_or_params[0], tuple(model_or_params[1:])
        name, p, c = _amplifier_spec(kind, () if kind in ("poly", 3) else rest, rest[0] if kind in ("poly", 3) and rest else None)
    a = np.asarray(amplitudes, dtype=np.float64)
    r = a * a
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if name == "clip":
            y = np.minimum(a, p[0]) + 0j
        elif name == "rapp":
            t = p[0] ** 2 * r / p[1] ** 2
            low = p[0] * a * (1.0 + np.minimum(t, 1.0) ** p[2]) ** (-0.5 / p[2])
            high = p[1] * (1.0 + np.maximum(t, 1.0) ** -p[2]) ** (-0.5 / p[2])
            y = np.where(t <= 1.0, low, high) + 0j
        elif name == "saleh":
            y = a * p[0] / (1.0 + p[1] * r) * np.exp(1j * p[2] * r / (1.0 + p[3] * r))
        else:
            c = c.astype(np.complex128)
            y = sum(c[:, k].sum() * a * r ** k for k in range(c.shape[1]))
    return np.abs(y), np.angle(y)


def amplifier_drive(mean_power, backoff_db, A=1.0):
    """AmplifierModel's drive d that puts mean |d x|^2 backoff_db below A^2, for a stream of mean power mean_power (SpectrumMeter.power then
    mean_power() supplies it): A sqrt(10^(-backoff_db / 10) / mean_power)"""
    mean_power, A = float(mean_power), float(A)
    if not (np.isfinite(mean_power) and mean_power > 0.0):
        raise ValueError("mean_power must be finite and > 0")
    if not (np.isfinite(A) and A > 0.0):
        raise ValueError("A must be finite and > 0")
    return float(A * np.sqrt(10.0 ** (-float(backoff_db) / 10.0) / mean_power))


class AmplifierModel(_Kernel):
    """The transmitter's power amplifier on a stream, on the device (contract in include/gfdm_hip.h, gfdm_hip_amplifier_model), between
    BurstShaper.place (or Resampler.resample) and FadingModel.apply / ChannelModel.apply.  With u = drive * x and r = |u|^2:
    clip(A): u where r <= A^2, else u A / |u|;  rapp(g, A, p): g u (1 + (g^2 r / A^2)^p)^(-1 / (2 p));  saleh(aa, ba, ap, bp): u aa / (1 +
    ba r) exp(j ap r / (1 + bp r));  poly(c): y[i] = sum_q sum_k c[q][k] u[i - q] r[i - q]^k, c complex of shape (n_delays <= 16, n_orders
    <= 5), the odd orders 1, 3, ...  The kind and its parameters (kept as float32) are fixed; drive has a setter that is read when a call is
    enqueued, and a captured graph keeps the value it was captured with."""
    _destroy = "gfdm_hip_amplifier_model_destroy"

    def __init__(self, kind, params=(), c=None, drive=1.0, device=None):
        name, p, c = _amplifier_spec(kind, params, c)
        Q, K = (0, 0) if c is None else c.shape
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        _check(lib().gfdm_hip_amplifier_model_create(ctypes.byref(h), AMPLIFIER_KINDS[name], p.ctypes.data if p.size else None, p.size,
                                                     None if c is None else c.ctypes.data, Q, K, float(drive), dev))
        self._h = h
        self._dev = dev

    @classmethod
    def clip(cls, A, drive=1.0, device=None):
        return cls("clip", (A,), drive=drive, device=device)

    @classmethod
    def rapp(cls, g, A, p, drive=1.0, device=None):
        return cls("rapp", (g, A, p), drive=drive, device=device)

    @classmethod
    def saleh(cls, aa, ba, ap, bp, drive=1.0, device=None):
        return cls("saleh", (aa, ba, ap, bp), drive=drive, device=device)

    @classmethod
    def poly(cls, c, drive=1.0, device=None):
        return cls("poly", (), c, drive=drive, device=device)

    def kind(self):
        """'clip' | 'rapp' | 'saleh' | 'poly'"""
        return {v: k for k, v in AMPLIFIER_KINDS.items()}[lib().gfdm_hip_amplifier_model_kind(self._h)]

    def params(self):
        """the kind's parameters as the handle keeps them: float64 values of the float32 roundings"""
        p = np.empty(lib().gfdm_hip_amplifier_model_n_params(self._h), np.float64)
        _check(lib().gfdm_hip_amplifier_model_params(self._h, p.ctypes.data))
        return p

    def n_delays(self):
        return lib().gfdm_hip_amplifier_model_n_delays(self._h)

    def n_orders(self):
        return lib().gfdm_hip_amplifier_model_n_orders(self._h)

    def coefficients(self):
        """c as given at create (complex64 (n_delays, n_orders), bit for bit); None for a kind without"""
        if self.kind() != "poly":
            return None
        c = np.empty((self.n_delays(), self.n_orders()), np.complex64)
        _check(lib().gfdm_hip_amplifier_model_coefficients(self._h, c.ctypes.data))
        return c

    @property
    def drive(self):
        v = ctypes.c_double()
        _check(lib().gfdm_hip_amplifier_model_drive(self._h, ctypes.byref(v)))
        return v.value

    @drive.setter
    def drive(self, drive):
        _check(lib().gfdm_hip_amplifier_model_set_drive(self._h, float(drive)))

    def set_drive(self, drive):
        self.drive = drive

    def apply(self, x, history=0, out=None, sc16=None, gain=1.0, stream=None):
        """x holds history + n samples, the result has n: sample i of the result is the amplifier's output for x[history + i]; the first
        `history` samples are the memory polynomial's past (what lies before them is zeros; the memoryless kinds read none of it).  A
        stream cut into calls gives the samples of one call, to the bit, when each piece passes history = min(n_delays - 1, samples before
        it).  numpy x -> numpy result (host path); a torch complex64 device tensor -> a tensor on its device (device path, current stream
        unless given).  An int16 `out` (or sc16=True) selects int16 I/Q of shape (n, 2), truncated and saturated, of y * gain."""
        if sc16 is None:
            sc16 = out is not None and str(getattr(out, "dtype", "")).replace("torch.", "") == "int16"
        sc16 = bool(sc16)
        if not sc16 and float(gain) != 1.0:
            raise ValueError("gain scales sc16 output: pass an int16 out or sc16=True (complex64 output is not scaled)")
        return _apply_stream(self, "gfdm_hip_amplifier_model_apply", x, history, None, sc16, gain, out, stream)


def resampler_step(x):
    """Resampler's step for a rate `x` (input samples per output sample, a float or a fractions.Fraction): x * 2^32 rounded to the nearest
    integer (ties to even), the unsigned Q32.32 of the contract.  1.0 -> 2^32.  A Fraction is converted exactly."""
    import fractions
    q = round(fractions.Fraction(x) * (1 << 32))
    if not (1 << 29) <= q <= (1 << 35):
        raise ValueError("the rate(%s) must lie in 1/8 .. 8" % (x,))
    return int(q)


def resampler_taps(n_phases=128, n_taps=16, cutoff=1.0, beta=8.0):
    """The default table of Resampler: float32 of shape (n_phases + 1, n_taps).  Row p, tap t is the Kaiser-windowed sinc
    cutoff * sinc(cutoff * u) * I0(beta * sqrt(1 - (u / W)^2)) / I0(beta) at u = t - D - p / n_phases (D = (n_taps - 1) // 2, W = D + 1, zero
    from |u| = W on), computed in float64, every row normalised to unit DC gain, then rounded to float32.  Where cutoff * u is an integer
    the sinc is exactly 0 or 1, so with cutoff = 1 row 0 is exactly the unit impulse at tap D; row n_phases is exactly row 0 moved by one tap.
    cutoff is a fraction of the input's Nyquist band: below 1 for decimation (step > 1).  The table is this project's own:
    bit-compatibility with GNU Radio's MMSE table is unpinned."""
    L, T = int(n_phases), int(n_taps)
    if T < 2 or T > 64:
        raise ValueError("n_taps(%d) must lie in 2 .. 64: one tap cannot hold row 0 moved by one tap" % T)
    if L < 1 or L > 1024 or L & (L - 1):
        raise ValueError("n_phases(%d) must be a power of two in 1 .. 1024" % L)
    if not 0.0 < float(cutoff) <= 1.0:
        raise ValueError("cutoff must lie in (0, 1]")
    if not float(beta) >= 0.0:
        raise ValueError("beta must be >= 0")
    D = (T - 1) // 2
    W = D + 1
    num = L * (np.arange(T)[None, :] - D) - np.arange(L + 1)[:, None]              # u * L, exact
    u = num / float(L)
    v = float(cutoff) * u
    s = np.sinc(v)
    whole = v == np.rint(v)
    s[whole] = (v[whole] == 0).astype(np.float64)
    inside = np.abs(num) < W * L
    win = np.where(inside, np.i0(float(beta) * np.sqrt(np.where(inside, 1.0 - (u / W) ** 2, 0.0))) / np.i0(float(beta)), 0.0)
    h = float(cutoff) * s * win
    h /= h.sum(axis=1, keepdims=True)
    h = h.astype(np.float32)
    h[L, 1:] = h[0, :-1]
    h[L, 0] = 0.0
    return h


class Resampler(_Kernel):
    """Fractional-rate resampling of a stream, on the device (contract in include/gfdm_hip.h, gfdm_hip_resampler): the resampler GNU
    Radio's channels.channel_model drives with epsilon (place -> resample -> ChannelModel.apply), and the conversion of a capture at a
    radio's rate in front of BurstSync.detect.  step_or_ratio: a Python int is the step itself (unsigned Q32.32: input samples per
    output sample times 2^32), a float or fractions.Fraction goes through resampler_step.  taps: a float32 table of shape
    (n_phases + 1, n_taps), row n_phases being row 0 moved by one sample; None: resampler_taps(n_phases, n_taps, cutoff) with cutoff =
    min(1, 1 / rate).  interp: "linear" between neighbouring rows or "nearest" (GNU Radio's mmse rule).  The table and interp are fixed;
    the step has a setter, and a captured graph keeps the step it was captured with.  The table does not follow set_step: the default
    table's cutoff is that of the step given here, so a later, larger step aliases what lies above 1 / rate -- build a new Resampler (or
    pass a table of the smaller cutoff) for a larger rate."""
    _destroy = "gfdm_hip_resampler_destroy"
    INTERP = {"nearest": 0, "linear": 1}

    def __init__(self, step_or_ratio, taps=None, n_phases=128, n_taps=16, interp="linear", device=None):
        if interp not in self.INTERP:
            raise ValueError("interp must be 'nearest' or 'linear', not %r" % (interp,))
        step = self._step_of(step_or_ratio)
        if taps is None:
            taps = resampler_taps(n_phases, n_taps, min(1.0, float(1 << 32) / step))
        t = np.ascontiguousarray(taps, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] < 2:
            raise ValueError("taps must have shape (n_phases + 1, n_taps), not %s" % (tuple(t.shape),))
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        _check(lib().gfdm_hip_resampler_create(ctypes.byref(h), t.ctypes.data, t.shape[1], t.shape[0] - 1, self.INTERP[interp], step, dev))
        self._h = h
        self._dev = dev
        self._T = int(t.shape[1])

    @staticmethod
    def _step_of(step_or_ratio):
        if isinstance(step_or_ratio, (int, np.integer)) and not isinstance(step_or_ratio, bool):
            step = int(step_or_ratio)
            if not (1 << 29) <= step <= (1 << 35):
                raise ValueError("step(%d) must lie in 2^29 .. 2^35 (Q32.32: 1/8 .. 8)" % step)
            return step
        return resampler_step(step_or_ratio)

    def n_taps(self):
        return lib().gfdm_hip_resampler_n_taps(self._h)

    def n_phases(self):
        return lib().gfdm_hip_resampler_n_phases(self._h)

    def interp(self):
        return "linear" if lib().gfdm_hip_resampler_interp(self._h) else "nearest"

    def taps(self):
        """the table as given to the constructor (float32 (n_phases + 1, n_taps), bit for bit)"""
        t = np.empty((self.n_phases() + 1, self.n_taps()), np.float32)
        _check(lib().gfdm_hip_resampler_taps(self._h, t.ctypes.data))
        return t

    def step(self):
        v = ctypes.c_uint64()
        _check(lib().gfdm_hip_resampler_step(self._h, ctypes.byref(v)))
        return v.value

    def set_step(self, step_or_ratio):
        _check(lib().gfdm_hip_resampler_set_step(self._h, self._step_of(step_or_ratio)))

    def plan(self, n_in, pos=0, flush=True):
        """(n_out, advance, next_pos) of a piece of n_in samples read from position pos (Q32.32, relative to its first sample): the outputs
        whose whole window lies inside the piece -- with flush those up to its end, zeros behind it --, how many samples the next piece
        starts further on, and its pos; the next piece passes history = min((n_taps - 1) // 2, samples in front of it).  Host arithmetic."""
        n_out, adv, nxt = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(lib().gfdm_hip_resampler_plan(self.step(), self._T, int(pos), int(n_in), int(bool(flush)), ctypes.byref(n_out), ctypes.byref(adv),
                                             ctypes.byref(nxt)))
        return n_out.value, adv.value, nxt.value

    def resample(self, x, history=0, pos=0, n_out=None, flush=True, out=None, stream=None):
        """x holds history + n_in samples; output i is the interpolated value at input position (pos + i * step) / 2^32, counted from
        x[history]; what lies in front of x and behind it is zeros.  n_out: None takes plan(n_in, pos, flush)'s.  numpy x -> numpy result
        (host path); a torch device tensor -> a tensor on its device (device path, current stream unless given).  complex64 samples, or
        int16 I/Q of shape (n, 2) or (2n,) (sc16, read as it is).  The result is complex64 always."""
        x, size, infix = ops.capture(x, self._dev, "x")
        ops.check_result(out, x, C64, self._dev, as_what="x")
        history, pos = int(history), int(pos)
        if history < 0 or history > size:
            raise ValueError("history(%d) must lie in 0 .. the size of x(%d)" % (history, size))
        n_in = size - history
        if n_out is None:
            n_out = self.plan(n_in, pos, flush)[0]
        n_out = int(n_out)
        if n_out < 0:
            raise ValueError("n_out(%d) must be >= 0" % n_out)
        res = ops.stream_result(x, n_out, False, self._dev, out, "x")
        sb = 4 if infix else 8
        self._run("gfdm_hip_resampler_resample" + infix, x, (ops.ptr(res), ops.ptr(x) + sb * history, n_out, n_in, history, pos), stream)
        return res


class LinkMeter(_Rows):
    """Closing the loop on the device (contract in include/gfdm_hip.h, gfdm_hip_link_meter): match() pairs BurstSync.detect's detections
    with the bursts that were sent, measure() counts bit / symbol / row errors of demodulated rows against the sent payload with the
    decisions SymbolMapper.decode makes and gives every row's error-vector power (data-aided: the EVM; without a payload: the
    decision-directed noise estimate SymbolMapper.soft's scale asks for), and every call adds to twelve counters that stay on the device
    until totals() reads them -- the one read of a curve point.  Constructor arguments as SymbolMapper's.  numpy arrays run the host
    flavour; torch device tensors the device flavour on the current stream unless given.  count is an int or (device path) detect's
    one-element int64 tensor.  out: a dict with any of the result's keys, to write into existing arrays; workspace: a uint8 device
    tensor of match_workspace_bytes() / measure_workspace_bytes() to use instead of a new one."""
    _destroy = "gfdm_hip_link_meter_destroy"
    _kind = "gfdm_hip_link_meter"
    FIELDS = ("rows", "symbols", "bits", "bit_errors", "symbol_errors", "row_errors", "detections", "matched", "missed", "false_alarms")

    @staticmethod
    def match_workspace_bytes(n_sent):
        return _bytes(lib().gfdm_hip_link_meter_match_workspace_bytes(int(n_sent)))

    @staticmethod
    def measure_workspace_bytes(n_sym, n_rows):
        return _bytes(lib().gfdm_hip_link_meter_measure_workspace_bytes(int(n_sym), int(n_rows)))

    def _result(self, out, key, like, n, dtype):
        """the output `key` of n elements: out[key] where given, else a new array of `like`'s kind"""
        return ops.result(like, (n,), dtype, self._dev, None if out is None else out.get(key), "out[%r]" % key, off_device=RuntimeError)

    def _settle(self, lead):
        """the host flavours run on the handle's own stream: what torch's current stream still holds for this handle (a reset) goes first"""
        if ops.on_device(lead):
            return
        try:
            import torch
        except ImportError:
            return
        torch.cuda.current_stream(self._dev).synchronize()

    def reset(self, stream=None):
        """enqueue the zeroing of the totals"""
        _check(lib().gfdm_hip_link_meter_reset(self._h, self._sp(stream)))

    def totals_ptr(self):
        """device pointer of the int64[12] totals (gfdm_hip_link_meter_totals_device)"""
        return lib().gfdm_hip_link_meter_totals_device(self._h)

    def totals(self, stream=None):
        """dict of Python ints: synchronises the stream and reads the 96 bytes"""
        t = np.zeros(12, np.int64)
        _check(lib().gfdm_hip_link_meter_totals(self._h, t.ctypes.data, self._sp(stream)))
        return {name: int(t[i]) for i, name in enumerate(self.FIELDS)}

    def ber(self, stream=None):
        """bit_errors / bits of totals(); nan where no bit was counted"""
        t = self.totals(stream)
        return t["bit_errors"] / t["bits"] if t["bits"] else float("nan")

    def fer(self, stream=None):
        """(row_errors + missed) / (rows + missed) of totals(): a burst that was not found is a frame in error; nan where both are 0"""
        t = self.totals(stream)
        den = t["rows"] + t["missed"]
        return (t["row_errors"] + t["missed"]) / den if den else float("nan")

    def match(self, frame_start, sent_pos, tol, offset=0, count=None, out=None, stream=None, workspace=None):
        """{"ref_row": int64 (n_rows,), "sent_row": int64 (n_sent,)}: ref_row[d] is the sent burst detection d is (or -1), sent_row[j] the
        detection that is sent burst j (or -1); sent_pos ascending, a detection matches within |frame_start - (sent_pos + offset)| <= tol"""
        fs = ops.vector(frame_start, I64, "frame_start", self._dev, None)
        sent = ops.vector(sent_pos, I64, "sent_pos", self._dev, fs, as_what="frame_start")
        n_rows, n_sent = ops.size(fs), ops.size(sent)
        tol, offset = int(tol), int(offset)
        res = {"ref_row": self._result(out, "ref_row", fs, n_rows, I64), "sent_row": self._result(out, "sent_row", fs, n_sent, I64)}
        cnt = ops.count_arg(count, fs, self._dev)
        self._settle(fs)
        self._run("gfdm_hip_link_meter_match", fs, (ops.ptr(res["ref_row"]), ops.ptr(res["sent_row"]), ops.ptr(fs), ops.ptr(cnt), n_rows, ops.ptr(sent),
                                                    n_sent, offset, tol), stream,
                  scratch=lambda: ops.workspace(workspace, fs, self.match_workspace_bytes(n_sent), self._dev))
        return res

    def measure(self, symbols, payload=None, ref_row=None, count=None, out=None, stream=None, workspace=None):
        """symbols (n_rows, n_sym) complex64 against payload (n_ref, row_bytes(n_sym)) uint8 -> {"bit_errors": int32, "err_power": float32,
        "ref_power": float32}, each (n_rows,); row r is compared with payload row ref_row[r] (None: r), a row whose ref_row is negative or
        beyond the payload gives -1 / 0 / 0 and is not read.  payload None: decision-directed, err_power against the decided points, no
        bit_errors."""
        symbols, n_rows, n_sym, _ = ops.rows(symbols, C64, "symbols", self._dev)
        n_ref = 0
        if payload is not None:
            payload, n_ref, _, _ = ops.rows(payload, U8, "payload", self._dev, self.row_bytes(n_sym), symbols, "symbols")
        if ref_row is not None:
            ref_row = ops.vector(ref_row, I64, "ref_row", self._dev, symbols, n_rows, "symbols")
        res = {}
        if payload is not None:
            res["bit_errors"] = self._result(out, "bit_errors", symbols, n_rows, I32)
        elif out is not None and out.get("bit_errors") is not None:
            raise ValueError("bit_errors needs a payload: a decision-directed call counts no errors")
        res["err_power"] = self._result(out, "err_power", symbols, n_rows, F32)
        res["ref_power"] = self._result(out, "ref_power", symbols, n_rows, F32)
        cnt = ops.count_arg(count, symbols, self._dev)
        if ops.on_device(symbols) and payload is not None and n_ref == 0:          # an empty tensor has no pointer, and NULL would mean decision-directed
            import torch
            payload = torch.empty(16, dtype=torch.uint8, device=symbols.device)
        self._settle(symbols)
        self._run("gfdm_hip_link_meter_measure", symbols, (ops.ptr(res.get("bit_errors")), ops.ptr(res["err_power"]), ops.ptr(res["ref_power"]),
                                                           ops.ptr(symbols), ops.ptr(payload), n_ref, ops.ptr(ref_row), ops.ptr(cnt), n_sym, n_rows), stream,
                  scratch=lambda: ops.workspace(workspace, symbols, self.measure_workspace_bytes(n_sym, n_rows), self._dev))
        return res


SPECTRUM_WINDOWS = {
    # cosine-sum windows, periodic form (the period is nfft, as scipy.signal.get_window(name, nfft) has it): sum_i (-1)^i a_i cos(2 pi i n / nfft)
    "rect": (1.0,),
    "hann": (0.5, 0.5),
    "blackmanharris": (0.35875, 0.48829, 0.14128, 0.01168),
    "flattop": (0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368),
}


def spectrum_window(name, nfft):
    """A window of SpectrumMeter: float32 (nfft,), 'rect' | 'hann' | 'blackmanharris' | 'flattop', the periodic cosine sums of
    SPECTRUM_WINDOWS computed in float64 and rounded once."""
    if name not in SPECTRUM_WINDOWS:
        raise ValueError("window must be one of %s, not %r" % (", ".join(sorted(SPECTRUM_WINDOWS)), name))
    nfft = int(nfft)
    if nfft < 1:
        raise ValueError("nfft(%d) must be >= 1" % nfft)
    n = np.arange(nfft, dtype=np.float64)
    w = np.zeros(nfft, np.float64)
    for i, a in enumerate(SPECTRUM_WINDOWS[name]):
        w += (-1.0) ** i * a * np.cos(2.0 * np.pi * i * n / nfft)
    return w.astype(np.float32)


def subcarrier_power(P, K):
    """The power of each of K subcarriers in a PSD P (FFT order, DC at 0, len(P) a multiple of K): the bins of subcarrier k are
    [(k - 1/2) nfft / K, (k + 1/2) nfft / K), cyclic; where nfft / K is odd the half bin is rounded down (the range starts at
    ceil((k - 1/2) nfft / K)).  float64 (K,), adding up to sum(P)."""
    P = np.asarray(P, dtype=np.float64).ravel()
    K = int(K)
    if K < 1 or P.size % K:
        raise ValueError("the PSD's size(%d) must be a multiple of K(%d)" % (P.size, K))
    per = P.size // K
    return np.roll(P, per // 2).reshape(K, per).sum(axis=1)


def oob_ratio_db(P, K, subcarrier_map):
    """10 log10(power of the subcarriers outside subcarrier_map / power of those in it) of a PSD P, by subcarrier_power: the out-of-band
    emission as a ratio to the occupied band.  -inf where nothing lies outside, nan where the map is empty."""
    sc = subcarrier_power(P, K)
    inside = np.zeros(int(K), bool)
    inside[np.asarray(subcarrier_map, dtype=np.int64).ravel() % int(K)] = True
    if not inside.any():
        return float("nan")
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(sc[~inside].sum() / sc[inside].sum()))


class SpectrumMeter(_Kernel):
    """What the waveform looks like on the air, on the device (contract in include/gfdm_hip.h, gfdm_hip_spectrum_meter): update() adds the
    Welch periodograms of a stream's segments of nfft samples every hop to psd_sum, update_at() those of the bursts BurstSync.detect
    found in a capture, power() adds every sample's power to a histogram, a sum and a peak; all of it stays on the device until read().
    window: a name of spectrum_window or a real float32 array (nfft,); hop defaults to nfft // 2; both are fixed.  numpy arrays run the
    host flavour; torch device tensors the device flavour on the current stream unless given.  complex64 samples, or int16 I/Q of
    shape (n, 2) or (2n,) (sc16, read as it is, unscaled)."""
    _destroy = "gfdm_hip_spectrum_meter_destroy"
    HEAD = ("segments", "bad_segments", "samples", "bad_samples", "peak_bits")
    HIST_BINS = 512

    def __init__(self, nfft, window="hann", hop=None, device=None):
        nfft = int(nfft)
        hop = nfft // 2 if hop is None else int(hop)
        if isinstance(window, str):
            if nfft < 1:
                raise ValueError("nfft must be a power of two in 16 .. 4096")
            window = spectrum_window(window, nfft)
        w = np.ascontiguousarray(window, dtype=np.float32).ravel()
        if w.size != nfft:
            raise ValueError("the window has %d values, expected nfft(%d)" % (w.size, nfft))
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        _check(lib().gfdm_hip_spectrum_meter_create(ctypes.byref(h), w.ctypes.data, nfft, hop, dev))
        self._h = h
        self._dev = dev
        self._nfft, self._hop = nfft, hop
        self._w = w.copy()

    def nfft(self):
        return lib().gfdm_hip_spectrum_meter_nfft(self._h)

    def hop(self):
        return lib().gfdm_hip_spectrum_meter_hop(self._h)

    def window(self):
        """the window as given at create (float32 (nfft,), bit for bit)"""
        w = np.empty(self._nfft, np.float32)
        _check(lib().gfdm_hip_spectrum_meter_window(self._h, w.ctypes.data))
        return w

    @staticmethod
    def plan_for(nfft, hop, n):
        """(n_seg, advance) of n samples: gfdm_hip_spectrum_meter_plan, host arithmetic"""
        n_seg, adv = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().gfdm_hip_spectrum_meter_plan(int(nfft), int(hop), int(n), ctypes.byref(n_seg), ctypes.byref(adv)))
        return n_seg.value, adv.value

    def plan(self, n):
        """(n_seg, advance) of a piece of n samples: the segments that lie inside it, and how many samples further on the next piece of
        a cut stream starts"""
        return self.plan_for(self._nfft, self._hop, n)

    def _settle(self, lead):
        """the host flavours run on the handle's own stream: what torch's current stream still holds for this handle (a reset) goes first"""
        if ops.on_device(lead):
            return
        try:
            import torch
        except ImportError:
            return
        if torch.cuda.is_available():
            torch.cuda.current_stream(self._dev).synchronize()

    def update(self, x, stream=None):
        """add the periodograms of x's segments to psd_sum; returns plan(len(x))'s advance"""
        x, n, infix = ops.capture(x, self._dev, "x")
        self._settle(x)
        self._run("gfdm_hip_spectrum_meter_accumulate" + infix, x, (ops.ptr(x), n), stream)
        return self.plan(n)[1]

    def update_at(self, x, starts, seg_per_burst, first=0, count=None, stream=None):
        """add the periodograms of seg_per_burst segments of every burst of the capture x: segment (b, j) starts at starts[b] + first +
        j hop; starts int64 (n_bursts,) and count as BurstSync.detect gives them (negative starts, bursts from count on and segments that
        do not lie inside x are skipped)"""
        x, n, infix = ops.capture(x, self._dev, "x")
        starts = ops.vector(starts, I64, "starts", self._dev, x, as_what="x")
        cnt = ops.count_arg(count, x, self._dev)
        self._settle(x)
        self._run("gfdm_hip_spectrum_meter_accumulate_at" + infix, x, (ops.ptr(x), n, ops.ptr(starts), ops.ptr(cnt), int(first), int(seg_per_burst),
                                                                       ops.size(starts)), stream)

    def power(self, x, stream=None):
        """add every sample's power to the histogram, power_sum, the peak and the sample counters"""
        x, n, infix = ops.capture(x, self._dev, "x")
        self._settle(x)
        self._run("gfdm_hip_spectrum_meter_power" + infix, x, (ops.ptr(x), n), stream)

    def reset(self, stream=None):
        """enqueue the zeroing of the totals"""
        _check(lib().gfdm_hip_spectrum_meter_reset(self._h, self._sp(stream)))

    def totals_ptr(self):
        """device pointer of the totals (gfdm_hip_spectrum_meter_totals_device): int64[8] | float64 | float64[nfft] | int64[512]"""
        return lib().gfdm_hip_spectrum_meter_totals_device(self._h)

    def totals_bytes(self):
        return _bytes(lib().gfdm_hip_spectrum_meter_totals_bytes(self._h))

    def read(self, stream=None):
        """synchronises the stream and reads the totals: dict(segments, bad_segments, samples, bad_samples, peak_bits: ints; power_sum: a
        float; psd_sum: float64 (nfft,), FFT order; hist: int64 (512,))"""
        head, ps = np.zeros(8, np.int64), np.zeros(1, np.float64)
        psd, hist = np.zeros(self._nfft, np.float64), np.zeros(self.HIST_BINS, np.int64)
        _check(lib().gfdm_hip_spectrum_meter_read(self._h, head.ctypes.data, ps.ctypes.data, psd.ctypes.data, hist.ctypes.data, self._sp(stream)))
        t = {name: int(head[i]) for i, name in enumerate(self.HEAD)}
        t.update(power_sum=float(ps[0]), psd_sum=psd, hist=hist)
        return t

    def psd(self, shift=False, stream=None):
        """psd_sum / (segments nfft sum(w^2)): for a stationary input its bins add up to the mean |x|^2.  shift: DC in the middle
        (numpy.fft.fftshift).  nan where no segment was counted."""
        t = self.read(stream)
        den = t["segments"] * self._nfft * float(np.sum(self._w.astype(np.float64) ** 2))
        P = t["psd_sum"] / den if den else np.full(self._nfft, np.nan)
        return np.fft.fftshift(P) if shift else P

    def band_power(self, lo, hi, stream=None):
        """the sum of psd() over the bins lo .. hi - 1, cyclic (lo may be negative: band_power(-4, 5) is nine bins around DC)"""
        P = self.psd(stream=stream)
        return float(P[np.arange(int(lo), int(hi)) % self._nfft].sum())

    def mean_power(self, stream=None):
        """power_sum / samples of power(); nan where no sample was counted"""
        t = self.read(stream)
        return t["power_sum"] / t["samples"] if t["samples"] else float("nan")

    def peak_power(self, stream=None):
        """the largest finite sample power power() has seen (peak_bits as the float32 it is)"""
        return float(np.array([self.read(stream)["peak_bits"]], np.uint32).view(np.float32)[0])

    def papr_db(self, stream=None):
        """10 log10(peak power / mean power) of power(); nan where no sample was counted or the mean is 0"""
        t = self.read(stream)
        if not t["samples"] or not t["power_sum"] > 0.0:
            return float("nan")
        peak = float(np.array([t["peak_bits"]], np.uint32).view(np.float32)[0])
        return float(10.0 * np.log10(peak / (t["power_sum"] / t["samples"])))

    @staticmethod
    def hist_edges():
        """the lower edges of the 512 histogram bins, float64: (1 + (i mod 8) / 8) 2^(i // 8 - 32); bin 0 also holds everything below"""
        i = np.arange(SpectrumMeter.HIST_BINS)
        return (1.0 + (i % 8) / 8.0) * np.exp2(i // 8 - 32.0)

    def ccdf(self, stream=None):
        """(edges, tail): the lower edge of every histogram bin relative to the mean power, and the number of counted samples whose power
        lies in that bin or above -- tail / samples is the CCDF of the instantaneous power at the edges, exact at every edge but bin 0's"""
        t = self.read(stream)
        mean = t["power_sum"] / t["samples"] if t["samples"] else float("nan")
        return self.hist_edges() / mean, np.cumsum(t["hist"][::-1])[::-1]


CC_MODES = {"terminated": 0, "truncated": 1}
CC_TERMINATED, CC_TRUNCATED = "terminated", "truncated"                   # the keys of CC_MODES, as mode() reports them


class ConvolutionalCode(_Kernel):
    """The constraint-length-7, rate-1/2 convolutional code (contract in include/gfdm_hip.h, gfdm_hip_conv_code): encode() in front of
    SymbolMapper.map, decode() -- a soft-input Viterbi decoder -- behind SymbolMapper.soft, decode_hard() behind SymbolMapper.decode.
    polys: the two generators, 1 <= |g| <= 127, a negative one complements its output; the default is 171 / 133 octal, GNU Radio's
    [109, 79] (the code is defined by the header's formulas; parity with GNU Radio's blocks is unpinned).  mode: "terminated" (six zero
    tail bits, steps = n_info + 6) or "truncated".  Rows are frames or bursts: information bytes (n_rows, info_bytes(n_info)), coded bytes
    (n_rows, >= coded_bytes(n_info)), LLRs (n_rows, >= coded_bits(n_info)) float32, positive for bit 0; a 1-D input is one row and gives a
    1-D result.  numpy arrays run the host flavour; torch device tensors the device flavour on the current stream unless given.  count (an
    int, or on the device path a one-element int64 tensor such as detect's) limits the call to the first count rows, the rest is written
    as zeros; it is clamped to [0, n_rows].  path_metric: an int32 array / tensor (n_rows,) that receives every row's final metric.
    workspace: a uint8 device tensor of workspace_bytes() to use instead of a new one (long rows only)."""
    _destroy = "gfdm_hip_conv_code_destroy"

    def __init__(self, polys=(109, 79), mode=CC_TERMINATED, device=0):
        g0, g1 = (int(g) for g in polys)
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_conv_code_create(ctypes.byref(h), g0, g1, CC_MODES.get(mode, mode), device))
        self._h = h
        self._dev = int(device)

    def polys(self):
        return tuple(lib().gfdm_hip_conv_code_poly(self._h, i) for i in (0, 1))

    def mode(self):
        """'terminated' | 'truncated'"""
        return {v: k for k, v in CC_MODES.items()}[lib().gfdm_hip_conv_code_mode(self._h)]

    def steps(self, n_info):
        """trellis steps of a row: n_info + 6 (terminated) or n_info"""
        return _bytes(lib().gfdm_hip_conv_code_steps(self._h, int(n_info)))

    def coded_bits(self, n_info):
        return _bytes(lib().gfdm_hip_conv_code_coded_bits(self._h, int(n_info)))

    def coded_bytes(self, n_info):
        return _bytes(lib().gfdm_hip_conv_code_coded_bytes(self._h, int(n_info)))

    def info_bytes(self, n_info):
        return _bytes(lib().gfdm_hip_conv_code_info_bytes(self._h, int(n_info)))

    def workspace_bytes(self, n_info, n_rows):
        """bytes of device scratch a device decode of n_rows rows needs: 0 while a row's survivor decisions fit in LDS"""
        return _bytes(lib().gfdm_hip_conv_code_decode_workspace_bytes(self._h, int(n_info), int(n_rows)))

    def _table(self, n_info, n_rows):
        g0, g1 = self.polys()
        _check(lib().gfdm_hip_conv_code_check(g0, g1, lib().gfdm_hip_conv_code_mode(self._h), n_info, n_rows))

    def encode(self, data, n_info, out_row_bytes=None, count=None, out=None, stream=None):
        """information bytes (n_rows, info_bytes(n_info)) uint8 -> coded bytes (n_rows, out_row_bytes) uint8; out_row_bytes (default
        coded_bytes(n_info)) may be wider, e.g. SymbolMapper.row_bytes(n_sym): what lies behind the coded bits is written as 0"""
        n_info = int(n_info)
        data, n_rows, _, flat = ops.rows(data, U8, "data", self._dev, self.info_bytes(n_info))
        self._table(n_info, n_rows)
        width = self.coded_bytes(n_info) if out_row_bytes is None else int(out_row_bytes)
        res = ops.result(data, (width,) if flat else (n_rows, width), U8, self._dev, out, off_device=RuntimeError)
        cnt = ops.count_arg(count, data, self._dev)
        self._run("gfdm_hip_conv_code_encode", data, (ops.ptr(res), ops.ptr(data), ops.ptr(cnt), n_info, width, n_rows), stream)
        return res

    def _decode(self, stem, x, dtype, what, n_info, extra, count, out, path_metric, workspace, stream):
        n_info = int(n_info)
        x, n_rows, width, flat = ops.rows(x, dtype, what, self._dev)
        self._table(n_info, n_rows)
        nb = self.info_bytes(n_info)
        res = ops.result(x, (nb,) if flat else (n_rows, nb), U8, self._dev, out, as_what=what, off_device=RuntimeError)
        ops.check_result(path_metric, x, I32, self._dev, "path_metric", what, n_rows, off_device=RuntimeError)
        cnt = ops.count_arg(count, x, self._dev)
        need = self.workspace_bytes(n_info, n_rows)
        self._run(stem, x, (ops.ptr(res), ops.ptr(path_metric), ops.ptr(x), ops.ptr(cnt), n_info, width, *extra, n_rows), stream,
                  scratch=lambda: ops.workspace(workspace, x, need, self._dev) if need else None)
        return res

    def decode(self, llr, n_info, gain, count=None, out=None, path_metric=None, workspace=None, stream=None):
        """LLRs (n_rows, llr_stride >= coded_bits(n_info)) float32 -- SymbolMapper.soft's output as it is -> information bytes
        (n_rows, info_bytes(n_info)) uint8.  A value enters the trellis as clamp(rint(llr * gain), -127, 127); gain is finite and > 0."""
        return self._decode("gfdm_hip_conv_code_decode", llr, F32, "llr", n_info, (float(gain),), count, out, path_metric, workspace, stream)

    def decode_hard(self, coded, n_info, count=None, out=None, path_metric=None, workspace=None, stream=None):
        """coded bytes (n_rows, in_row_bytes >= coded_bytes(n_info)) uint8 -- encode's output, SymbolMapper.decode's bytes -> information
        bytes (n_rows, info_bytes(n_info)) uint8: the same decoder on +1 / -1"""
        return self._decode("gfdm_hip_conv_code_decode_hard", coded, U8, "coded", n_info, (), count, out, path_metric, workspace, stream)


PUNCTURE_PATTERNS = {"1/2": (1, 1), "2/3": (1, 1, 1, 0), "3/4": (1, 1, 1, 0, 0, 1), "5/6": (1, 1, 1, 0, 0, 1, 1, 0, 0, 1)}


def puncture_pattern(rate):
    """The keep pattern (uint8) of a code rate over the coded row c_{0,0} c_{0,1} c_{1,0} c_{1,1} ...: "1/2", "2/3", "3/4" or "5/6" -- IEEE
    802.11a's patterns for the 171 / 133 code (include/gfdm_hip.h, gfdm_hip_rate_matcher: bit-compatibility with that standard is
    unpinned).  Pure host code."""
    if rate not in PUNCTURE_PATTERNS:
        raise ValueError("no puncturing pattern for rate %r: one of %s" % (rate, ", ".join(sorted(PUNCTURE_PATTERNS))))
    return np.array(PUNCTURE_PATTERNS[rate], np.uint8)


def block_interleaver(n, columns):
    """The permutation (int32, n entries) of a block interleaver: 0 .. rows * columns - 1 written row-wise into rows = ceil(n / columns)
    rows, read column-wise, the indices >= n dropped.  Pure host code."""
    n, columns = int(n), int(columns)
    if n < 1 or columns < 1:
        raise ValueError("a block interleaver needs n >= 1 and columns >= 1")
    rows = -(-n // columns)
    a = np.arange(rows * columns, dtype=np.int64).reshape(rows, columns).T.ravel()
    return a[a < n].astype(np.int32)


class RateMatcher(_Kernel):
    """Puncturing and interleaving of coded bits (contract in include/gfdm_hip.h, gfdm_hip_rate_matcher): match() between
    ConvolutionalCode.encode and SymbolMapper.map, unmatch() between SymbolMapper.soft and ConvolutionalCode.decode, unmatch_hard()
    between SymbolMapper.decode and ConvolutionalCode.decode(gain=1).  n_coded: the bits of a mother-code row (coded_bits(n_info) of the
    code).  keep: the puncturing pattern, bit i is transmitted iff keep[i % len(keep)] != 0 (None: every bit; puncture_pattern(rate) has
    the usual ones).  perm: a permutation of range(tx_bits()), transmitted bit j is punctured bit perm[j] (None: identity;
    block_interleaver(n, columns) makes one; RateMatcher.tx_bits_of(n_coded, keep) sizes it).  Rows are frames or bursts: coded bytes
    (n_rows, >= ceil(n_coded / 8)), transmitted bytes (n_rows, >= tx_bytes()), LLRs in (n_rows, >= tx_bits()) and out
    (n_rows, >= coded_bits()) float32; a 1-D input is one row and gives a 1-D result.  numpy arrays run the host flavour; torch device
    tensors the device flavour on the current stream unless given.  count (an int, or on the device path a one-element int64 tensor such
    as detect's) limits the call to the first count rows, the rest is written as zeros; it is clamped to [0, n_rows]."""
    _destroy = "gfdm_hip_rate_matcher_destroy"

    @staticmethod
    def _pattern(keep):
        return np.ones(1, U8) if keep is None else np.ascontiguousarray(np.asarray(keep).ravel() != 0, dtype=U8)

    @staticmethod
    def _perm(perm):
        if perm is None:
            return None
        p = np.asarray(perm).ravel()
        if p.size and not np.issubdtype(p.dtype, np.integer):
            raise TypeError("perm must hold integers, not %s" % p.dtype)
        if p.size and (p.min() < 0 or p.max() >= 2 ** 31):
            raise ValueError("perm is not a permutation of 0 .. n_tx - 1")
        return np.ascontiguousarray(p, dtype=I32)

    @classmethod
    def tx_bits_of(cls, n_coded, keep=None):
        """transmitted bits of a row of n_coded coded bits under the pattern: no handle, no device"""
        keep = cls._pattern(keep)
        return _bytes(lib().gfdm_hip_rate_matcher_tx_bits_of(int(n_coded), keep.ctypes.data, keep.size))

    def __init__(self, n_coded, keep=None, perm=None, device=0):
        keep, perm = self._pattern(keep), self._perm(perm)
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_rate_matcher_create(ctypes.byref(h), int(n_coded), keep.ctypes.data, keep.size, ops.ptr(perm),
                                                  0 if perm is None else perm.size, device))
        self._h = h
        self._dev = int(device)
        self._n_coded, self._n_tx = (_bytes(getattr(lib(), "gfdm_hip_rate_matcher_" + name)(h)) for name in ("coded_bits", "tx_bits"))

    def coded_bits(self):
        return self._n_coded

    def tx_bits(self):
        return self._n_tx

    def tx_bytes(self):
        """bytes of a packed transmitted row: ceil(tx_bits() / 8)"""
        return _bytes(lib().gfdm_hip_rate_matcher_tx_bytes(self._h))

    def source_index(self):
        """src (int32, tx_bits() entries): transmitted bit j is coded bit src[j] -- the pattern and the permutation composed"""
        src = np.empty(self._n_tx, I32)
        _check(lib().gfdm_hip_rate_matcher_source_index(self._h, src.ctypes.data))
        return src

    def _call(self, name, x, dtype, what, least_in, out_dtype, least_out, out_width, out_what, count, out, stream):
        x, n_rows, width, flat = ops.rows(x, dtype, what, self._dev)
        out_width = least_out if out_width is None else int(out_width)
        if width < least_in or out_width < least_out:
            raise ValueError("%s has rows of %d, below the minimum %d" % ((what, width, least_in) if width < least_in else (out_what, out_width, least_out)))
        res = ops.result(x, (out_width,) if flat else (n_rows, out_width), out_dtype, self._dev, out, as_what=what, off_device=RuntimeError)
        cnt = ops.count_arg(count, x, self._dev)
        self._run("gfdm_hip_rate_matcher_" + name, x, (ops.ptr(res), ops.ptr(x), ops.ptr(cnt), width, out_width, n_rows), stream)
        return res

    def match(self, coded, out_row_bytes=None, count=None, out=None, stream=None):
        """coded bytes (n_rows, in_row_bytes >= ceil(coded_bits() / 8)) uint8 -- encode's output at any width -> transmitted bytes
        (n_rows, out_row_bytes) uint8; out_row_bytes (default tx_bytes()) may be wider, e.g. SymbolMapper.row_bytes(n_sym): what lies
        behind the transmitted bits is written as 0"""
        return self._call("match", coded, U8, "coded", (self._n_coded + 7) // 8, U8, self.tx_bytes(), out_row_bytes, "out_row_bytes", count, out, stream)

    def unmatch(self, llr, out_stride=None, count=None, out=None, stream=None):
        """LLRs (n_rows, in_stride >= tx_bits()) float32 -- SymbolMapper.soft's output as it is -> LLRs of the coded row
        (n_rows, out_stride) float32, out_stride >= coded_bits() (the default): a bit copy of every transmitted value at its coded
        position, +0.0 at the punctured positions and behind coded_bits().  What ConvolutionalCode.decode takes."""
        return self._call("unmatch", llr, F32, "llr", self._n_tx, F32, self._n_coded, out_stride, "out_stride", count, out, stream)

    def unmatch_hard(self, tx, out_stride=None, count=None, out=None, stream=None):
        """transmitted bytes (n_rows, in_row_bytes >= tx_bytes()) uint8 -- SymbolMapper.decode's output -> float32 rows laid out as
        unmatch's: +1.0 for a 0 bit, -1.0 for a 1 bit, +0.0 at the punctured positions.  ConvolutionalCode.decode with gain 1 on them is
        hard-decision decoding with erasures."""
        return self._call("unmatch_hard", tx, U8, "tx", self.tx_bytes(), F32, self._n_coded, out_stride, "out_stride", count, out, stream)


class FrameCheck(_Kernel):
    """Frame check sequence and whitening of payload rows (contract in include/gfdm_hip.h, gfdm_hip_frame_check): attach() in front of
    ConvolutionalCode.encode, verify() behind ConvolutionalCode.decode at n_info = frame_bits -- the receiver's keep-or-drop verdict on a
    row.  n_payload: the bytes of a payload row; a frame row is frame_bytes = n_payload + 4: the payload, its CRC-32 (zlib.crc32) least
    significant byte first, and over both the whitening sequence of the Fibonacci LFSR (mask, seed, degree), MSB first; degree=0
    switches whitening off (mask and seed are then ignored).  The default is x^7 + x^4 + 1 from the all-ones state.  Rows are frames or
    bursts: payload bytes (n_rows, >= payload_bytes), frame bytes (n_rows, >= frame_bytes); a 1-D input is one row and gives a 1-D
    result.  numpy arrays run the host flavour; torch device tensors the device flavour on the current stream unless given.  count (an
    int, or on the device path a one-element int64 tensor such as detect's) limits the call to the first count rows, the rest is written
    as zeros (ok 0); it is clamped to [0, n_rows]."""
    _destroy = "gfdm_hip_frame_check_destroy"

    @staticmethod
    def _lfsr(mask, seed, degree):
        mask, seed, degree = int(mask), int(seed), int(degree)
        if degree == 0:
            return 0, 0, 0
        if not (0 <= mask < 2 ** 64 and 0 <= seed < 2 ** 64):
            raise ValueError("mask and seed must satisfy 1 <= value < 2^degree")
        return mask, seed, degree

    @classmethod
    def check(cls, n_payload, mask=0x11, seed=0x7F, degree=7, n_rows=0):
        """the argument table of the constructor and the calls (ValueError): no handle, no device"""
        _check(lib().gfdm_hip_frame_check_check(int(n_payload), *cls._lfsr(mask, seed, degree), int(n_rows)))

    def __init__(self, n_payload, mask=0x11, seed=0x7F, degree=7, device=0):
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_frame_check_create(ctypes.byref(h), int(n_payload), *self._lfsr(mask, seed, degree), device))
        self._h = h
        self._dev = int(device)
        self._n_payload, self._n_frame = (_bytes(getattr(lib(), "gfdm_hip_frame_check_" + name)(h)) for name in ("payload_bytes", "frame_bytes"))

    @property
    def payload_bytes(self):
        return self._n_payload

    @property
    def frame_bytes(self):
        """payload_bytes + 4"""
        return self._n_frame

    @property
    def frame_bits(self):
        """8 * frame_bytes: the n_info of ConvolutionalCode.encode / decode"""
        return _bytes(lib().gfdm_hip_frame_check_frame_bits(self._h))

    @property
    def whitening(self):
        """the packed whitening sequence of a frame row (uint8, frame_bytes entries; zeros with degree=0)"""
        seq = np.empty(self._n_frame, U8)
        _check(lib().gfdm_hip_frame_check_whitening(self._h, seq.ctypes.data))
        return seq

    @staticmethod
    def _width(width, least, what):
        width = least if width is None else int(width)
        if width < least:
            raise ValueError("%s is %d, below the minimum %d" % (what, width, least))
        return width

    def attach(self, payload, count=None, out=None, stream=None, out_row_bytes=None):
        """payload bytes (n_rows, in_row_bytes >= payload_bytes) uint8 -> frame bytes (n_rows, out_row_bytes) uint8; out_row_bytes
        (default frame_bytes) may be wider: what lies behind the frame is written as 0.  What ConvolutionalCode.encode takes at
        n_info = frame_bits."""
        x, n_rows, width, flat = ops.rows(payload, U8, "payload", self._dev)
        self._width(width, self._n_payload, "the width of payload")
        out_width = self._width(out_row_bytes, self._n_frame, "out_row_bytes")
        res = ops.result(x, (out_width,) if flat else (n_rows, out_width), U8, self._dev, out, as_what="payload", off_device=RuntimeError)
        cnt = ops.count_arg(count, x, self._dev)
        self._run("gfdm_hip_frame_check_attach", x, (ops.ptr(res), ops.ptr(x), ops.ptr(cnt), width, out_width, n_rows), stream)
        return res

    def verify(self, frames, count=None, good_rows=False, out=None, stream=None, out_row_bytes=None, payload=True):
        """frame bytes (n_rows, in_row_bytes >= frame_bytes) uint8 -- ConvolutionalCode.decode's output as it is -> (payload, ok), or with
        good_rows (payload, ok, good_row, n_good): payload (n_rows, out_row_bytes >= payload_bytes, the default) uint8, the dewhitened
        payload of every live row, good or not; ok (n_rows,) uint8, 1 where the row's CRC holds; good_row (n_rows,) int64, the indices
        of the good rows in ascending order, then -1; n_good (1,) int64.  payload=False checks only (the first result is None).  out: a
        dict with any of "payload", "ok", "good_row", "n_good" to write into."""
        x, n_rows, width, flat = ops.rows(frames, U8, "frames", self._dev)
        self._width(width, self._n_frame, "the width of frames")
        out = out or {}

        def result(key, shape, dtype):
            return ops.result(x, shape, dtype, self._dev, out.get(key), "out[%r]" % key, "frames", off_device=RuntimeError)

        res_p, out_width = None, 0
        if payload:
            out_width = self._width(out_row_bytes, self._n_payload, "out_row_bytes")
            res_p = result("payload", (out_width,) if flat else (n_rows, out_width), U8)
        elif out.get("payload") is not None:
            raise ValueError("payload=False writes no payload")
        ok = result("ok", (n_rows,), U8)
        good = n_good = None
        if good_rows:
            good, n_good = result("good_row", (n_rows,), I64), result("n_good", (1,), I64)
            if n_rows == 0:                                    # a call without rows launches nothing
                n_good[...] = 0
        elif out.get("good_row") is not None or out.get("n_good") is not None:
            raise ValueError("good_row and n_good need good_rows=True")
        cnt = ops.count_arg(count, x, self._dev)
        if n_rows:                                             # (an empty tensor has no address: its good_row would read as "not asked for")
            self._run("gfdm_hip_frame_check_verify", x, (ops.ptr(res_p), ops.ptr(ok), ops.ptr(good), ops.ptr(n_good), ops.ptr(x), ops.ptr(cnt), width,
                                                          out_width, n_rows), stream)
        return (res_p, ok, good, n_good) if good_rows else (res_p, ok)
