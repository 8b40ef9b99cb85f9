"""Loader and ctypes signature table of the C-ABI in include/gfdm_hip.h (gr-gfdm_amd/lib/libgfdm_hip.so).

tests/test_boundary.py holds the expanded table to the header: same names, same arity, same class of every parameter and return type.
"""
import atexit
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.normpath(os.path.join(_PKG, "..", "..", "lib"))
LIB_PATH = os.environ.get("GFDM_HIP_LIB") or os.path.join(LIB_DIR, "libgfdm_hip.so")   # override: A/B builds of the kernels

OK, EINVAL_TAPS, EINVAL_OVERLAP, EINVAL, ENODEV, EHIP, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7

_lib = None


class GfdmHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("gfdm_hip error %d: %s" % (status, message))
        self.status = status


def _signatures():
    """{name: (restype, argtypes)} of every function of the header"""
    vp, i32, i64, cp, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_float, ctypes.c_double
    u32, u64, out = ctypes.c_uint, ctypes.c_uint64, ctypes.POINTER
    sig = {}

    def fn(name, res, *args):
        sig["gfdm_hip_" + name] = (res, list(args))

    def getters(prefix, names, res=i32):
        """<prefix>_<name>(handle) for every name"""
        for name in names.split():
            fn(prefix + "_" + name, res, vp)

    def call(stem, *args, device=(vp,), sc16=None):
        """The <stem>_host / <stem>_device pair of one batched call: (handle, *args), and what the device flavour appends -- the stream, or
        (workspace, stream).  sc16: also the <stem>_sc16_* twins, their sibling's arguments plus these."""
        for infix, more in (("", ()),) if sc16 is None else (("", ()), ("_sc16", tuple(sc16))):
            fn(stem + infix + "_host", i32, vp, *args, *more)
            fn(stem + infix + "_device", i32, vp, *args, *more, *device)

    ws_stream = (vp, vp)

    # ---- the library ----
    fn("strerror", cp, i32)
    for name in ("last_error", "version", "build_id"):
        fn(name, cp)
    fn("device_count", i32)
    fn("quiesce", None)
    for name in ("force_generic_family_for_testing", "set_jit", "set_ic_matrix_cores", "set_wide_access", "set_dft_matrix_cores",
                 "set_host_streaming_copies_for_testing"):
        fn(name, i32, i32)
    fn("precompile", i32, i32, i32, i32, u32)
    fn("jit_build_for_testing", i32, i32, i32, i32, i32)
    fn("register_host", i32, vp, ctypes.c_size_t)
    fn("unregister_host", i32, vp)
    fn("set_host_pipeline", i32, i32, i64, i32, i32, i32)
    fn("get_host_pipeline", i32, vp, vp, vp, vp, vp)
    fn("host_call_stats", i32, vp, vp, vp, vp, vp, vp)
    fn("host_call_times", i32, vp)

    # ---- modulator, receiver, advanced receiver ----
    fn("modulator_create", i32, out(vp), i32, i32, i32, vp, i32, i32)
    getters("modulator", "destroy block_size")
    fn("modulator_filter_taps", i32, vp, vp)
    call("modulator_work", vp, vp, i64)
    fn("receiver_create", i32, out(vp), i32, i32, i32, vp, i32, i32)
    getters("receiver", "destroy block_size timeslots subcarriers overlap")
    fn("receiver_filter_taps", i32, vp, vp)
    fn("receiver_ic_filter_taps", i32, vp, vp)
    call("receiver_demodulate", vp, vp, vp, i64)
    call("receiver_fft_filter_downsample", vp, vp, vp, i64)
    call("receiver_transform_subcarriers_to_td", vp, vp, i64)
    call("receiver_cancel_sc_interference", vp, vp, vp, i64)
    fn("advanced_receiver_create", i32, out(vp), i32, i32, i32, vp, i32, vp, i32, i32, vp, i32, i32, i32, i32)
    getters("advanced_receiver", "destroy block_size get_ic get_phase_compensation decision")
    fn("advanced_receiver_set_ic", i32, vp, i32)
    fn("advanced_receiver_set_phase_compensation", i32, vp, i32)
    call("advanced_receiver_work", vp, vp, vp, i64)
    for rx, verb in (("receiver", "demodulate"), ("advanced_receiver", "work")):      # what _Receiver drives on either kind of handle
        fn(rx + "_configure_frames", i32, vp, i32, i32, vp, i32, i32)
        fn(rx + "_set_channel_estimator", i32, vp, vp)
        fn(rx + "_io_layout", i32, vp, i32, i32, vp, vp, vp)
        call("%s_%s_frames" % (rx, verb), vp, vp, vp, i32, i64)
        call("%s_%s_estimated" % (rx, verb), vp, vp, vp, i32, i32, i64)
        call("%s_%s_bursts" % (rx, verb), vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, sc16=())

    # ---- transmitter and its stand-alone stages ----
    fn("transmitter_create", i32, out(vp), i32, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32)
    getters("transmitter", "destroy input_vector_size output_vector_size block_size n_cyclic_shifts")
    fn("transmitter_cyclic_shift", i32, vp, i32)
    call("transmitter_work", vp, i32, vp, i32, i64)
    call("transmitter_modulate", vp, vp, i32, i64)
    call("transmitter_add_frame", vp, vp, i32, i64)
    fn("resource_mapper_create", i32, out(vp), i32, i32, i32, vp, i32, i32, i32)
    getters("resource_mapper", "destroy block_size frame_size")
    call("resource_mapper_map", vp, vp, i32, i64)
    call("resource_mapper_demap", vp, vp, i32, i64)
    fn("cyclic_prefixer_create", i32, out(vp), i32, i32, i32, i32, vp, i32, i32, i32)
    getters("cyclic_prefixer", "destroy block_size frame_size cyclic_shift")
    call("cyclic_prefixer_add", vp, vp, i32, i64)
    call("cyclic_prefixer_remove", vp, vp, i64)

    # ---- channel estimator ----
    fn("channel_estimator_create", i32, out(vp), i32, i32, i32, i32, i32, vp, i32, i32)
    getters("channel_estimator", "destroy timeslots fft_len active_subcarriers frame_len is_dc_free filtered_len")
    fn("channel_estimator_preamble_filter_taps", i32, vp, vp)
    for name in ("estimate_frame", "estimate_preamble_channel", "filter_preamble_estimate", "interpolate_frame", "prepare_for_zf"):
        call("channel_estimator_" + name, vp, vp, i64)
    call("channel_estimator_estimate_snr", vp, vp, vp, i64)
    for kind in ("modulator", "receiver", "advanced_receiver", "transmitter", "channel_estimator"):
        getters(kind, "kernel_name", cp)

    # ---- burst sync and extractor: every call on a capture has an sc16 twin with the same signature ----
    fn("burst_sync_create", i32, out(vp), i32, i32, vp, i32, i64, i32)
    getters("burst_sync", "destroy fft_len cp_len")
    getters("burst_sync", "window_len corr_len", i64)
    call("burst_sync_find_frame_start", vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, sc16=())
    call("burst_sync_auto_correlate", vp, vp, vp, i64, i64, i64, i64, sc16=())
    call("burst_sync_find_frame_start_at", vp, vp, vp, vp, vp, vp, i64, vp, i64, sc16=())
    fn("burst_sync_detect_check", i32, i32, i32, i64, i64, f32, i64, i64, i64)
    fn("burst_sync_detect_workspace_bytes", i64, vp, i64)
    call("burst_sync_detect", vp, vp, vp, vp, vp, vp, vp, i64, f32, i64, i64, i64, device=ws_stream, sc16=())
    fn("burst_extractor_create", i32, out(vp), i32, i32, i32, i32)
    getters("burst_extractor", "destroy burst_len tag_backoff get_cfo_correction")
    fn("burst_extractor_set_cfo_correction", i32, vp, i32)
    call("burst_extractor_extract", vp, vp, i64, vp, vp, vp, i64, sc16=())

    # ---- burst shaper and channel model: the sc16 twins take the peak / the gain behind their sibling's arguments ----
    fn("burst_shaper_create", i32, out(vp), i32, i32, i32, f32, f32, i32)
    getters("burst_shaper", "destroy frame_len pre_padding post_padding")
    fn("burst_shaper_scale", i32, vp, vp)
    fn("burst_shaper_check", i32, i32, i32, i32, f64, i64, i64)
    fn("burst_shaper_workspace_bytes", i64, vp, i64, i64)
    call("burst_shaper_shape", vp, vp, i64, device=ws_stream, sc16=(f64,))
    call("burst_shaper_place", vp, i64, vp, vp, vp, i64, device=ws_stream, sc16=(f64,))
    fn("channel_model_create", i32, out(vp), vp, i32, f64, f64, u64, i32)
    getters("channel_model", "destroy n_taps")
    fn("channel_model_taps", i32, vp, vp)
    fn("channel_model_frequency_offset", i32, vp, out(f64))
    fn("channel_model_noise_voltage", i32, vp, out(f64))
    fn("channel_model_seed", i32, vp, out(u64))
    fn("channel_model_set_frequency_offset", i32, vp, f64)
    fn("channel_model_set_noise_voltage", i32, vp, f64)
    fn("channel_model_set_seed", i32, vp, u64)
    fn("channel_model_check", i32, i32, f64, f64, i64, i64, i64, f64)
    call("channel_model_apply", vp, vp, i64, i64, i64, sc16=(f64,))

    # ---- resampler: the sc16 twins read int16 I/Q and take their sibling's arguments ----
    fn("resampler_create", i32, out(vp), vp, i32, i32, i32, u64, i32)
    getters("resampler", "destroy n_taps n_phases interp")
    fn("resampler_taps", i32, vp, vp)
    fn("resampler_step", i32, vp, out(u64))
    fn("resampler_set_step", i32, vp, u64)
    fn("resampler_check", i32, i32, i32, i32, u64, i64, i64, i64, i64)
    fn("resampler_plan", i32, u64, i32, i64, i64, i32, out(i64), out(i64), out(i64))
    call("resampler_resample", vp, vp, i64, i64, i64, i64, sc16=())

    # ---- fading model: four tables at create, the channel model's call ----
    fn("fading_model_create", i32, out(vp), vp, vp, vp, vp, i32, i32, i32, i32)
    getters("fading_model", "destroy n_paths n_sinusoids n_taps")
    for name in ("taps", "amplitudes", "frequencies", "phases"):
        fn("fading_model_" + name, i32, vp, vp)
    fn("fading_model_check", i32, i32, i32, i32, i64, i64, i64, f64)
    call("fading_model_apply", vp, vp, i64, i64, i64, sc16=(f64,))

    # ---- amplifier model: the kind's parameters or a coefficient table at create, the channel model's call without an offset ----
    fn("amplifier_model_create", i32, out(vp), i32, vp, i32, vp, i32, i32, f64, i32)
    getters("amplifier_model", "destroy kind n_params n_delays n_orders")
    fn("amplifier_model_params", i32, vp, vp)
    fn("amplifier_model_coefficients", i32, vp, vp)
    fn("amplifier_model_drive", i32, vp, out(f64))
    fn("amplifier_model_set_drive", i32, vp, f64)
    fn("amplifier_model_check", i32, i32, vp, i32, i32, i32, f64, i64, i64, f64)
    call("amplifier_model_apply", vp, vp, i64, i64, sc16=(f64,))

    # ---- symbol mapper and link meter ----
    for kind in ("symbol_mapper", "link_meter"):
        fn(kind + "_create", i32, out(vp), vp, i32, i32, i32)
        getters(kind, "destroy bits_per_symbol n_points decision")
        fn(kind + "_row_bytes", i64, vp, i64)
    fn("symbol_mapper_points", i32, vp, vp)
    fn("symbol_mapper_check", i32, i32, i64, i64)
    call("symbol_mapper_map", vp, vp, vp, i64, i64)
    call("symbol_mapper_decode", vp, vp, vp, i64, i64)
    call("symbol_mapper_soft", vp, vp, vp, vp, i64, i64)
    fn("link_meter_totals_device", vp, vp)
    fn("link_meter_reset", i32, vp, vp)
    fn("link_meter_totals", i32, vp, vp, vp)
    fn("link_meter_match_workspace_bytes", i64, i64)
    fn("link_meter_measure_workspace_bytes", i64, i64, i64)
    call("link_meter_match", vp, vp, vp, vp, i64, vp, i64, i64, i64, device=ws_stream)
    call("link_meter_measure", vp, vp, vp, vp, vp, i64, vp, vp, i64, i64, device=ws_stream)

    # ---- convolutional code ----
    fn("conv_code_create", i32, out(vp), i32, i32, i32, i32)
    getters("conv_code", "destroy mode")
    fn("conv_code_poly", i32, vp, i32)
    for name in ("steps", "coded_bits", "coded_bytes", "info_bytes"):
        fn("conv_code_" + name, i64, vp, i64)
    fn("conv_code_decode_workspace_bytes", i64, vp, i64, i64)
    fn("conv_code_check", i32, i32, i32, i32, i64, i64)
    call("conv_code_encode", vp, vp, vp, i64, i64, i64)
    call("conv_code_decode", vp, vp, vp, vp, i64, i64, f32, i64, device=ws_stream)
    call("conv_code_decode_hard", vp, vp, vp, vp, i64, i64, i64, device=ws_stream)

    # ---- rate matcher ----
    fn("rate_matcher_create", i32, out(vp), i64, vp, i32, vp, i64, i32)
    getters("rate_matcher", "destroy")
    getters("rate_matcher", "coded_bits tx_bits tx_bytes", i64)
    fn("rate_matcher_source_index", i32, vp, vp)
    fn("rate_matcher_tx_bits_of", i64, i64, vp, i32)
    fn("rate_matcher_check", i32, i64, vp, i32, vp, i64, i64)
    for name in ("match", "unmatch", "unmatch_hard"):
        call("rate_matcher_" + name, vp, vp, vp, i64, i64, i64)

    # ---- frame check ----
    fn("frame_check_create", i32, out(vp), i64, u64, u64, i32, i32)
    getters("frame_check", "destroy")
    getters("frame_check", "payload_bytes frame_bytes frame_bits", i64)
    fn("frame_check_whitening", i32, vp, vp)
    fn("frame_check_check", i32, i64, u64, u64, i32, i64)
    call("frame_check_attach", vp, vp, vp, i64, i64, i64)
    call("frame_check_verify", vp, vp, vp, vp, vp, vp, i64, i64, i64)

    # ---- spectrum meter: every call on samples has an sc16 twin with the same signature ----
    fn("spectrum_meter_create", i32, out(vp), vp, i32, i64, i32)
    getters("spectrum_meter", "destroy nfft")
    getters("spectrum_meter", "hop totals_bytes", i64)
    fn("spectrum_meter_window", i32, vp, vp)
    fn("spectrum_meter_plan", i32, i32, i64, i64, out(i64), out(i64))
    fn("spectrum_meter_totals_device", vp, vp)
    fn("spectrum_meter_reset", i32, vp, vp)
    fn("spectrum_meter_read", i32, vp, vp, vp, vp, vp, vp)
    call("spectrum_meter_accumulate", vp, i64, sc16=())
    call("spectrum_meter_accumulate_at", vp, i64, vp, vp, i64, i64, i64, sc16=())
    call("spectrum_meter_power", vp, i64, sc16=())
    return sig


def lib():
    """Load libgfdm_hip.so (built by `make -C gr-gfdm_amd` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `make -C gr-gfdm_amd` (no CPU fallback exists)" % LIB_PATH)
    # PyTorch-ROCm ships its own copy of the HIP runtime (torch/lib/libamdhip64.so).  A process can only work with ONE runtime:
    # if /opt/rocm's gets initialised first (through this library), torch later reports "No HIP GPUs are available".  The device
    # path of this package hands torch tensors to the library, so when torch is installed its runtime is loaded first and
    # libgfdm_hip.so binds to it (same SONAME); without torch the library uses /opt/rocm's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    sig = _signatures()
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    L._gfdm_symbols = sorted(sig)
    # background builds must not outlive the interpreter's tear-down of the HIP runtime (gfdm_hip_quiesce: include/gfdm_hip.h)
    atexit.register(L.gfdm_hip_quiesce)
    _lib = L
    return L


def loaded():
    """the library if lib() has loaded it, else None (a handle's __del__ must not load it)"""
    return _lib


def exported_symbols():
    return list(lib()._gfdm_symbols)


def _check(status):
    if status == OK:
        return
    L = lib()
    msg = (L.gfdm_hip_last_error() or b"").decode() or L.gfdm_hip_strerror(status).decode()
    if status in (EINVAL_TAPS, EINVAL_OVERLAP, EINVAL):
        raise ValueError(msg)            # std::invalid_argument in the reference (pybind11 maps it to ValueError)
    raise GfdmHipError(status, msg)
