"""The operand layer of the Python wrapper (gfdm_amd/_operands.py) on its own: no handle, no library, no device.  Every rule it keeps for
the classes of gfdm_amd.capi, for numpy operands and -- where the rule is "a tensor off the device is refused" -- for torch CPU tensors."""
import numpy as np
import pytest

from gfdm_amd import _operands as ops

C64, F32, I64, I32, I16, U8 = np.complex64, np.float32, np.int64, np.int32, np.int16, np.uint8


def test_kind_is_told_by_the_duck_test():
    import torch
    assert ops.is_tensor(torch.zeros(1)) and not ops.is_tensor(np.zeros(1)) and not ops.is_tensor([1, 2]) and not ops.is_tensor(None)
    assert ops.size(torch.zeros(3, 2)) == 6 and ops.size(np.zeros((3, 2))) == 6 and ops.size([1, 2, 3]) == 3
    with pytest.raises(TypeError, match="starts must be a host array, as frames is"):
        ops.operand(torch.zeros(2, dtype=torch.int64), I64, "starts", 0, np.zeros(2, C64), "frames")
    with pytest.raises(TypeError, match="scale must be a CUDA/HIP tensor, as the input is"):
        ops.operand(np.zeros(2, F32), F32, "scale", 0, torch.zeros(2))


def test_host_arrays_are_converted_only_where_they_must_be():
    for dtype in (C64, I64, F32, I32, U8, I16):
        a = np.zeros((3, 4), dtype)
        got = ops.operand(a, dtype, "a", 0)
        assert got is a and ops.ptr(got) == a.ctypes.data                  # as it is: its own pointer, no copy
    got = ops.operand([[1, 2], [3, 4]], C64, "a", 0)                        # anything np.asarray takes, integers included
    assert got.dtype == C64 and got.flags.c_contiguous and got.shape == (2, 2)
    strided = np.arange(12, dtype=np.complex128).reshape(3, 4)[:, ::2]
    got = ops.operand(strided, C64, "a", 0)
    assert got.dtype == C64 and got.flags.c_contiguous and np.array_equal(got, strided)
    for dtype, src in ((I64, [1, 2]), (F32, [1.5]), (I32, (3,))):
        assert ops.operand(src, dtype, "v", 0).dtype == dtype
    assert ops.ptr(None) is None


def test_bound_gives_operand_address_and_count_in_one_call():
    a = np.zeros((3, 4), C64)
    got, address, n = ops.bound(a, C64, "a", 0)
    assert got is a and address == a.ctypes.data and n == 12
    got, address, n = ops.bound([1, 2, 3], C64, "a", 0, address=False)
    assert got.dtype == C64 and address is None and n == 3
    import torch
    with pytest.raises(TypeError, match="out must be a contiguous complex64 CUDA/HIP tensor"):
        ops.bound(torch.zeros(4, dtype=torch.complex64), C64, "out", 0, torch.zeros(4))
    with pytest.raises(TypeError, match="out must be a CUDA/HIP tensor, as the input is"):
        ops.bound(np.zeros(4, C64), C64, "out", 0, torch.zeros(4))


def test_packed_bytes_and_complex_samples_are_not_made_from_other_integers():
    for dt in (np.int8, I16, I32, np.float32, bool):
        with pytest.raises(TypeError, match=r"data must be uint8 \(packed bytes\), not"):
            ops.operand(np.zeros(4, dt), U8, "data", 0)
    for dt in (I16, I32, U8, bool):
        with pytest.raises(TypeError, match="x must be complex samples, not"):
            ops.operand(np.zeros(4, dt), C64, "x", 0, floating=True)
        with pytest.raises(TypeError, match="symbols must be complex samples"):
            ops.rows(np.zeros((2, 2), dt), C64, "symbols", 0)
    assert ops.operand(np.zeros(4, np.float64), C64, "x", 0, floating=True).dtype == C64


def test_a_tensor_off_the_device_or_of_another_type_is_refused():
    import torch
    for t, dtype in ((torch.zeros(4, dtype=torch.complex64), C64), (torch.zeros(4, dtype=torch.float32), C64), (torch.zeros(4, dtype=torch.int64), I64),
                     (torch.zeros(4, dtype=torch.uint8), U8), (torch.zeros(4, 2, dtype=torch.int16), I16)):
        with pytest.raises(TypeError, match="t must be a contiguous %s CUDA/HIP tensor" % np.dtype(dtype).name):
            ops.operand(t, dtype, "t", 0)
    with pytest.raises(TypeError, match="contiguous complex64"):
        ops.rows(torch.zeros(2, 2, dtype=torch.complex64), C64, "symbols", 0)
    with pytest.raises(TypeError, match="contiguous int64"):
        ops.vector(torch.zeros(2, dtype=torch.int64), I64, "offsets", 0, None)


def test_element_counts():
    a = np.zeros((2, 6), C64)
    assert ops.sized(a, 12, "a") is a and ops.at_least(a, 12, "a") is a and ops.at_least(a, 0, "a") is a
    with pytest.raises(RuntimeError, match="a has 12 elements, expected 13"):
        ops.sized(a, 13, "a")
    with pytest.raises(RuntimeError, match=r"rx_preamble size\(12\) MUST be at least 13!"):
        ops.at_least(a, 13, "rx_preamble")
    assert ops.batches(a, 4, "size(%d) MUST be a multiple of %d!") == 3 and ops.batches(np.zeros(0), 4, "%d %d") == 0
    for n in (5, 0, -1):
        with pytest.raises(RuntimeError, match=r"frames size\(12\) MUST be a multiple of frame_len\(%d\)!" % n):
            ops.batches(a, n, "frames size(%d) MUST be a multiple of frame_len(%d)!")
    v = ops.vector([[1, 2], [3, 4]], I64, "starts", 0, a, 4)
    assert v.shape == (4,) and v.dtype == I64
    with pytest.raises(RuntimeError, match="scale has 1 elements, expected 2"):
        ops.vector([1.0], F32, "scale", 0, a, 2)


def test_rows():
    x, n_rows, w, flat = ops.rows(np.zeros((3, 5), C64), C64, "symbols", 0)
    assert (n_rows, w, flat) == (3, 5, False)
    x, n_rows, w, flat = ops.rows(np.zeros(5, U8), U8, "data", 0, width=5)
    assert (n_rows, w, flat) == (1, 5, True)
    assert ops.rows(np.zeros((0, 5), C64), C64, "symbols", 0)[1:] == (0, 5, False)
    with pytest.raises(RuntimeError, match="data has rows of 5 elements, expected 4"):
        ops.rows(np.zeros((3, 5), U8), U8, "data", 0, width=4)
    with pytest.raises(ValueError, match=r"symbols must be \(n_rows, n\) or one row \(n,\), not \(2, 3, 4\)"):
        ops.rows(np.zeros((2, 3, 4), C64), C64, "symbols", 0)
    with pytest.raises(TypeError, match="payload must be a host array, as symbols is"):
        import torch
        ops.rows(torch.zeros(2, 2, dtype=torch.uint8), U8, "payload", 0, None, np.zeros((2, 2), C64), "symbols")


def test_sc16_shapes():
    assert ops.sc16_pairs((7, 2), "iq") == 7 and ops.sc16_pairs((14,), "iq") == 7 and ops.sc16_pairs((0,), "iq") == 0
    assert ops.sc16_pairs((14,), "iq", np.zeros(14, I16).reshape).shape == (7, 2)
    with pytest.raises(ValueError, match=r"iq: a flat sc16 array holds I, Q pairs, its length\(13\) is odd"):
        ops.sc16_pairs((13,), "iq")
    for shape in ((7, 3), (2, 7, 2), ()):
        with pytest.raises(ValueError, match=r"iq: an sc16 array has shape \(n, 2\) or \(2n,\)"):
            ops.sc16_pairs(shape, "iq")


def test_a_new_result_is_of_the_leading_operands_kind():
    x = np.zeros(4, C64)
    for shape, dtype in (((3, 5), C64), ((7,), F32), ((0, 4), U8), ((2, 2), I16), ((1,), I64), ((3,), I32)):
        r = ops.result(x, shape, dtype, 0)
        assert isinstance(r, np.ndarray) and r.shape == shape and r.dtype == dtype and r.flags.c_contiguous
    assert ops.stream_result(x, 5, False, 0).shape == (5,) and ops.stream_result(x, 5, False, 0).dtype == C64
    assert ops.stream_result(x, 5, True, 0).shape == (5, 2) and ops.stream_result(x, 5, True, 0).dtype == I16


def test_a_callers_out_is_checked_and_written_in_place():
    import torch
    x = np.zeros(4, C64)
    out = np.zeros((3, 5), C64)
    assert ops.result(x, (3, 5), C64, 0, out) is out and ops.result(x, (15,), C64, 0, out) is out          # the element count decides, not the shape
    for flat in (np.zeros((5, 2), I16), np.zeros(10, I16)):
        assert ops.stream_result(x, 5, True, 0, flat) is flat                                               # sc16: (n, 2) or flat (2n,)
    with pytest.raises(TypeError, match="out must be a numpy array, as x is"):
        ops.result(x, (4,), C64, 0, torch.zeros(4, dtype=torch.complex64), as_what="x")
    with pytest.raises(TypeError, match="out must be a numpy array"):
        ops.result(x, (4,), C64, 0, [0j] * 4)
    with pytest.raises(TypeError, match="out must be a CUDA/HIP tensor, as the input is"):
        ops.result(torch.zeros(4), (4,), C64, 0, np.zeros(4, C64))
    with pytest.raises(TypeError, match=r"out must be int16 I/Q \(sc16\), not complex64"):
        ops.stream_result(x, 4, True, 0, np.zeros(4, C64))
    with pytest.raises(TypeError, match="out must be complex64, not int16"):
        ops.stream_result(x, 4, False, 0, np.zeros((4, 2), I16))
    with pytest.raises(TypeError, match=r"out\['bit_errors'\] must be int32, not int64"):
        ops.result(x, (4,), I32, 0, np.zeros(4, I64), "out['bit_errors']")
    with pytest.raises(TypeError, match="out must be contiguous"):
        ops.result(x, (4,), C64, 0, np.zeros(8, C64)[::2])
    with pytest.raises(TypeError, match="out must be contiguous"):
        ops.stream_result(x, 4, True, 0, np.zeros((4, 4), I16)[:, :2])
    with pytest.raises(ValueError, match="odd"):
        ops.stream_result(x, 4, True, 0, np.zeros(9, I16))
    with pytest.raises(ValueError, match="shape"):
        ops.stream_result(x, 4, True, 0, np.zeros((4, 3), I16))
    with pytest.raises(RuntimeError, match="out holds 10 samples, expected 7"):
        ops.stream_result(x, 7, False, 0, np.zeros(10, C64))
    with pytest.raises(RuntimeError, match="out holds 5 samples, expected 7"):
        ops.stream_result(x, 7, True, 0, np.zeros((5, 2), I16))
    with pytest.raises(RuntimeError, match="out holds 15 elements, expected 16"):
        ops.result(x, (4, 4), C64, 0, out)
    with pytest.raises(TypeError, match="out must be a contiguous complex64 CUDA/HIP tensor"):
        ops.result(torch.zeros(4), (4,), C64, 0, torch.zeros(4, dtype=torch.complex64))                      # a tensor off the device
    with pytest.raises(RuntimeError, match="out must live on GPU 0, as the handle does"):                     # SymbolMapper's and LinkMeter's answer to the same
        ops.result(torch.zeros(4), (4,), C64, 0, torch.zeros(4, dtype=torch.complex64), off_device=RuntimeError)
    ops.check_result(None, x, C64, 0)
    ops.check_result(np.zeros(3, C64), x, C64, 0)                                                           # the early half: no size yet
    with pytest.raises(TypeError, match="int16"):
        ops.check_result(np.zeros(3, C64), x, I16, 0)


def test_count_on_the_host_path_is_an_int():
    import torch
    x = np.zeros(4, C64)
    assert ops.count_arg(None, x, 0) is None and ops.count_arg(None, torch.zeros(1), 0) is None
    for count in (3, np.int64(3), np.array([3])):
        c = ops.count_arg(count, x, 0)
        assert c.dtype == I64 and c.shape == (1,) and c[0] == 3 and ops.ptr(c) == c.ctypes.data
    with pytest.raises(TypeError, match="count must be an int on the host path"):
        ops.count_arg(torch.zeros(1, dtype=torch.int64), x, 0)
    with pytest.raises(RuntimeError, match="count has 2 elements, expected 1"):
        ops.count_arg([1, 2], x, 0)
    with pytest.raises(TypeError, match="count must be a contiguous int64 CUDA/HIP tensor"):
        ops.count_arg(torch.zeros(1, dtype=torch.int64), torch.zeros(4), 0)                                   # a count tensor off the device


def test_workspace_must_be_a_device_byte_tensor():
    import torch
    like = torch.zeros(4)
    for ws in (np.zeros(64, U8), torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.float32), [0] * 64):
        with pytest.raises(TypeError, match="workspace must be a contiguous uint8 CUDA/HIP tensor of at least 64 bytes on GPU 0"):
            ops.workspace(ws, like, 64, 0)
    ws = ops.workspace(None, like, 64, 0)                                                                    # a new one beside `like` (here: the CPU)
    assert ws.dtype == torch.uint8 and ws.numel() == 64


def test_capture():
    import torch
    a = np.zeros(9, C64)
    got, n, infix = ops.capture(a, 0)
    assert ops.ptr(got) == a.ctypes.data and (n, infix) == (9, "")                                          # its own memory, no copy
    got, n, infix = ops.capture(np.zeros((3, 3), np.float64), 0)
    assert got.dtype == C64 and got.shape == (9,) and (n, infix) == (9, "")
    for iq in (np.zeros((7, 2), I16), np.zeros(14, I16)):
        got, n, infix = ops.capture(iq, 0)
        assert got is iq and (n, infix) == (7, "_sc16")                                                      # passed on as it is, never widened
    for dt in (np.int8, U8, np.uint16, I32, I64):
        with pytest.raises(TypeError, match=r"samples: integer captures must be int16 \(sc16\), not"):
            ops.capture(np.zeros((8, 2), dt), 0)
    with pytest.raises(TypeError, match="integer captures must be int16"):
        ops.capture(torch.zeros(8, 2, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="odd"):
        ops.capture(np.zeros(13, I16), 0)
    with pytest.raises(ValueError, match="shape"):
        ops.capture(np.zeros((4, 2, 2), I16), 0)
    with pytest.raises(TypeError, match="samples must be a C-contiguous int16 array"):
        ops.capture(np.zeros((8, 4), I16)[:, :2], 0)
    for t in (torch.zeros(8, 2, dtype=torch.int16), torch.zeros(8, dtype=torch.complex64)):                 # tensors off the device
        with pytest.raises(TypeError, match="samples must be a contiguous"):
            ops.capture(t, 0)


def test_the_wrapper_needs_no_torch_on_the_host_path():
    """importing the package and the operand layer, and every host-path rule above, import no torch: a subprocess that forbids it"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; sys.modules['torch'] = None\n"
            "import numpy as np\n"
            "from gfdm_amd import _operands as ops\n"
            "x = ops.operand([1, 2], np.complex64, 'x', 0)\n"
            "ops.result(x, (2,), np.complex64, 0); ops.count_arg(1, x, 0); ops.capture(np.zeros((2, 2), np.int16), 0)\n"
            "ops.stream_result(x, 2, True, 0, np.zeros(4, np.int16)); ops.rows(np.zeros(3, np.uint8), np.uint8, 'd', 0)\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gr-gfdm_amd", "python"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
