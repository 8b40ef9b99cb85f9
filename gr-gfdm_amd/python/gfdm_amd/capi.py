"""ctypes binding of the C-ABI in include/gfdm_hip.h (gr-gfdm_amd/lib/libgfdm_hip.so).

Host-side mirror of the reference's kernel-class surface for Python callers that
work on whole batches and on device-resident torch tensors (bench.py, the
multi-GPU sharding helper).  The pybind11 module `gfdm_python` is the drop-in for
the reference's own binding; this module adds nothing numerically, it only
forwards pointers.  There is no CPU fallback: a missing library or GPU raises.
"""
import ctypes
import mmap
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.normpath(os.path.join(_PKG, "..", "..", "lib"))
LIB_PATH = os.environ.get("GFDM_HIP_LIB") or os.path.join(LIB_DIR, "libgfdm_hip.so")   # override: A/B builds of the kernels

OK, EINVAL_TAPS, EINVAL_OVERLAP, EINVAL, ENODEV, EHIP, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7
DECIDE = {"auto": -1, "nearest": 0, "qpsk": 1, "bpsk": 2}
DECIDE_AUTO, DECIDE_NEAREST, DECIDE_QPSK, DECIDE_BPSK = "auto", "nearest", "qpsk", "bpsk"      # the keys of DECIDE, as decision_rule() reports them

_lib = None


class GfdmHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("gfdm_hip error %d: %s" % (status, message))
        self.status = status


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
    vp, i32, i64, cp, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_char_p, ctypes.c_float, ctypes.c_double
    u64 = ctypes.c_uint64
    sig = {
        "gfdm_hip_strerror": (cp, [i32]),
        "gfdm_hip_last_error": (cp, []),
        "gfdm_hip_device_count": (i32, []),
        "gfdm_hip_force_generic_family_for_testing": (i32, [i32]),
        "gfdm_hip_set_jit": (i32, [i32]),
        "gfdm_hip_precompile": (i32, [i32, i32, i32, ctypes.c_uint]),
        "gfdm_hip_set_ic_matrix_cores": (i32, [i32]),
        "gfdm_hip_set_wide_access": (i32, [i32]),
        "gfdm_hip_quiesce": (None, []),
        "gfdm_hip_set_dft_matrix_cores": (i32, [i32]),
        "gfdm_hip_jit_build_for_testing": (i32, [i32, i32, i32, i32]),
        "gfdm_hip_version": (cp, []),
        "gfdm_hip_build_id": (cp, []),
        "gfdm_hip_register_host": (i32, [vp, ctypes.c_size_t]),
        "gfdm_hip_unregister_host": (i32, [vp]),
        "gfdm_hip_set_host_pipeline": (i32, [i32, i64, i32, i32, i32]),
        "gfdm_hip_get_host_pipeline": (i32, [vp, vp, vp, vp, vp]),
        "gfdm_hip_host_call_stats": (i32, [vp, vp, vp, vp, vp, vp]),
        "gfdm_hip_host_call_times": (i32, [vp]),
        "gfdm_hip_set_host_streaming_copies_for_testing": (i32, [i32]),
        "gfdm_hip_modulator_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, i32, i32]),
        "gfdm_hip_modulator_destroy": (i32, [vp]),
        "gfdm_hip_modulator_block_size": (i32, [vp]),
        "gfdm_hip_modulator_filter_taps": (i32, [vp, vp]),
        "gfdm_hip_modulator_kernel_name": (cp, [vp]),
        "gfdm_hip_modulator_work_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_modulator_work_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, i32, i32]),
        "gfdm_hip_receiver_destroy": (i32, [vp]),
        "gfdm_hip_receiver_block_size": (i32, [vp]),
        "gfdm_hip_receiver_timeslots": (i32, [vp]),
        "gfdm_hip_receiver_subcarriers": (i32, [vp]),
        "gfdm_hip_receiver_overlap": (i32, [vp]),
        "gfdm_hip_receiver_filter_taps": (i32, [vp, vp]),
        "gfdm_hip_receiver_ic_filter_taps": (i32, [vp, vp]),
        "gfdm_hip_receiver_kernel_name": (cp, [vp]),
        "gfdm_hip_receiver_demodulate_host": (i32, [vp, vp, vp, vp, i64]),
        "gfdm_hip_receiver_demodulate_device": (i32, [vp, vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_fft_filter_downsample_host": (i32, [vp, vp, vp, vp, i64]),
        "gfdm_hip_receiver_fft_filter_downsample_device": (i32, [vp, vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_transform_subcarriers_to_td_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_receiver_transform_subcarriers_to_td_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_cancel_sc_interference_host": (i32, [vp, vp, vp, vp, i64]),
        "gfdm_hip_receiver_cancel_sc_interference_device": (i32, [vp, vp, vp, vp, i64, vp]),
        "gfdm_hip_advanced_receiver_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, i32, vp, i32, i32, vp, i32, i32, i32, i32]),
        "gfdm_hip_advanced_receiver_destroy": (i32, [vp]),
        "gfdm_hip_advanced_receiver_block_size": (i32, [vp]),
        "gfdm_hip_advanced_receiver_set_ic": (i32, [vp, i32]),
        "gfdm_hip_advanced_receiver_get_ic": (i32, [vp]),
        "gfdm_hip_advanced_receiver_set_phase_compensation": (i32, [vp, i32]),
        "gfdm_hip_advanced_receiver_get_phase_compensation": (i32, [vp]),
        "gfdm_hip_advanced_receiver_decision": (i32, [vp]),
        "gfdm_hip_advanced_receiver_kernel_name": (cp, [vp]),
        "gfdm_hip_advanced_receiver_work_host": (i32, [vp, vp, vp, vp, i64]),
        "gfdm_hip_advanced_receiver_work_device": (i32, [vp, vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_configure_frames": (i32, [vp, i32, i32, vp, i32, i32]),
        "gfdm_hip_receiver_demodulate_frames_host": (i32, [vp, vp, vp, vp, i32, i64]),
        "gfdm_hip_receiver_demodulate_frames_device": (i32, [vp, vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_advanced_receiver_configure_frames": (i32, [vp, i32, i32, vp, i32, i32]),
        "gfdm_hip_advanced_receiver_work_frames_host": (i32, [vp, vp, vp, vp, i32, i64]),
        "gfdm_hip_advanced_receiver_work_frames_device": (i32, [vp, vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_transmitter_create": (i32, [ctypes.POINTER(vp)] + [i32] * 6 + [vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32]),
        "gfdm_hip_transmitter_destroy": (i32, [vp]),
        "gfdm_hip_transmitter_input_vector_size": (i32, [vp]),
        "gfdm_hip_transmitter_output_vector_size": (i32, [vp]),
        "gfdm_hip_transmitter_block_size": (i32, [vp]),
        "gfdm_hip_transmitter_n_cyclic_shifts": (i32, [vp]),
        "gfdm_hip_transmitter_cyclic_shift": (i32, [vp, i32]),
        "gfdm_hip_transmitter_kernel_name": (cp, [vp]),
        "gfdm_hip_transmitter_work_host": (i32, [vp, vp, i32, vp, i32, i64]),
        "gfdm_hip_transmitter_work_device": (i32, [vp, vp, i32, vp, i32, i64, vp]),
        "gfdm_hip_transmitter_modulate_host": (i32, [vp, vp, vp, i32, i64]),
        "gfdm_hip_transmitter_modulate_device": (i32, [vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_transmitter_add_frame_host": (i32, [vp, vp, vp, i32, i64]),
        "gfdm_hip_transmitter_add_frame_device": (i32, [vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_resource_mapper_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, vp, i32, i32, i32]),
        "gfdm_hip_resource_mapper_destroy": (i32, [vp]),
        "gfdm_hip_resource_mapper_block_size": (i32, [vp]),
        "gfdm_hip_resource_mapper_frame_size": (i32, [vp]),
        "gfdm_hip_resource_mapper_map_host": (i32, [vp, vp, vp, i32, i64]),
        "gfdm_hip_resource_mapper_map_device": (i32, [vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_resource_mapper_demap_host": (i32, [vp, vp, vp, i32, i64]),
        "gfdm_hip_resource_mapper_demap_device": (i32, [vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_cyclic_prefixer_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, i32, vp, i32, i32, i32]),
        "gfdm_hip_cyclic_prefixer_destroy": (i32, [vp]),
        "gfdm_hip_cyclic_prefixer_block_size": (i32, [vp]),
        "gfdm_hip_cyclic_prefixer_frame_size": (i32, [vp]),
        "gfdm_hip_cyclic_prefixer_cyclic_shift": (i32, [vp]),
        "gfdm_hip_cyclic_prefixer_add_host": (i32, [vp, vp, vp, i32, i64]),
        "gfdm_hip_cyclic_prefixer_add_device": (i32, [vp, vp, vp, i32, i64, vp]),
        "gfdm_hip_cyclic_prefixer_remove_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_cyclic_prefixer_remove_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, i32, i32, vp, i32, i32]),
        "gfdm_hip_channel_estimator_destroy": (i32, [vp]),
        "gfdm_hip_channel_estimator_timeslots": (i32, [vp]),
        "gfdm_hip_channel_estimator_fft_len": (i32, [vp]),
        "gfdm_hip_channel_estimator_active_subcarriers": (i32, [vp]),
        "gfdm_hip_channel_estimator_frame_len": (i32, [vp]),
        "gfdm_hip_channel_estimator_is_dc_free": (i32, [vp]),
        "gfdm_hip_channel_estimator_filtered_len": (i32, [vp]),
        "gfdm_hip_channel_estimator_kernel_name": (cp, [vp]),
        "gfdm_hip_channel_estimator_preamble_filter_taps": (i32, [vp, vp]),
        "gfdm_hip_channel_estimator_estimate_frame_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_estimate_frame_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_estimate_preamble_channel_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_estimate_preamble_channel_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_filter_preamble_estimate_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_filter_preamble_estimate_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_interpolate_frame_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_interpolate_frame_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_prepare_for_zf_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_prepare_for_zf_device": (i32, [vp, vp, vp, i64, vp]),
        "gfdm_hip_channel_estimator_estimate_snr_host": (i32, [vp, vp, vp, vp, i64]),
        "gfdm_hip_channel_estimator_estimate_snr_device": (i32, [vp, vp, vp, vp, i64, vp]),
        "gfdm_hip_receiver_set_channel_estimator": (i32, [vp, vp]),
        "gfdm_hip_advanced_receiver_set_channel_estimator": (i32, [vp, vp]),
        "gfdm_hip_receiver_io_layout": (i32, [vp, i32, i32, vp, vp, vp]),
        "gfdm_hip_advanced_receiver_io_layout": (i32, [vp, i32, i32, vp, vp, vp]),
        "gfdm_hip_receiver_demodulate_estimated_host": (i32, [vp, vp, vp, vp, i32, i32, i64]),
        "gfdm_hip_receiver_demodulate_estimated_device": (i32, [vp, vp, vp, vp, i32, i32, i64, vp]),
        "gfdm_hip_advanced_receiver_work_estimated_host": (i32, [vp, vp, vp, vp, i32, i32, i64]),
        "gfdm_hip_advanced_receiver_work_estimated_device": (i32, [vp, vp, vp, vp, i32, i32, i64, vp]),
        "gfdm_hip_receiver_demodulate_bursts_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64]),
        "gfdm_hip_receiver_demodulate_bursts_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, vp]),
        "gfdm_hip_advanced_receiver_work_bursts_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64]),
        "gfdm_hip_advanced_receiver_work_bursts_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, vp]),
        "gfdm_hip_burst_sync_create": (i32, [ctypes.POINTER(vp), i32, i32, vp, i32, i64, i32]),
        "gfdm_hip_burst_sync_destroy": (i32, [vp]),
        "gfdm_hip_burst_sync_fft_len": (i32, [vp]),
        "gfdm_hip_burst_sync_cp_len": (i32, [vp]),
        "gfdm_hip_burst_sync_window_len": (i64, [vp]),
        "gfdm_hip_burst_sync_corr_len": (i64, [vp]),
        "gfdm_hip_burst_sync_find_frame_start_host": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64]),
        "gfdm_hip_burst_sync_find_frame_start_device": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp]),
        "gfdm_hip_burst_sync_auto_correlate_host": (i32, [vp, vp, vp, vp, i64, i64, i64, i64]),
        "gfdm_hip_burst_sync_auto_correlate_device": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, vp]),
        "gfdm_hip_burst_sync_find_frame_start_at_host": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64]),
        "gfdm_hip_burst_sync_find_frame_start_at_device": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp]),
        "gfdm_hip_burst_sync_detect_check": (i32, [i32, i32, i64, i64, f32, i64, i64, i64]),
        "gfdm_hip_burst_sync_detect_workspace_bytes": (i64, [vp, i64]),
        "gfdm_hip_burst_sync_detect_host": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, f32, i64, i64, i64]),
        "gfdm_hip_burst_sync_detect_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, f32, i64, i64, i64, vp, vp]),
        "gfdm_hip_burst_extractor_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, i32]),
        "gfdm_hip_burst_extractor_destroy": (i32, [vp]),
        "gfdm_hip_burst_extractor_burst_len": (i32, [vp]),
        "gfdm_hip_burst_extractor_tag_backoff": (i32, [vp]),
        "gfdm_hip_burst_extractor_set_cfo_correction": (i32, [vp, i32]),
        "gfdm_hip_burst_extractor_get_cfo_correction": (i32, [vp]),
        "gfdm_hip_burst_extractor_extract_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i64]),
        "gfdm_hip_burst_extractor_extract_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i64, vp]),
        # the sc16 twins: the same signatures, `samples` interleaved int16 I/Q
        "gfdm_hip_receiver_demodulate_bursts_sc16_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64]),
        "gfdm_hip_receiver_demodulate_bursts_sc16_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, vp]),
        "gfdm_hip_advanced_receiver_work_bursts_sc16_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64]),
        "gfdm_hip_advanced_receiver_work_bursts_sc16_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i64, vp]),
        "gfdm_hip_burst_sync_find_frame_start_sc16_host": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64]),
        "gfdm_hip_burst_sync_find_frame_start_sc16_device": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp]),
        "gfdm_hip_burst_sync_auto_correlate_sc16_host": (i32, [vp, vp, vp, vp, i64, i64, i64, i64]),
        "gfdm_hip_burst_sync_auto_correlate_sc16_device": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, vp]),
        "gfdm_hip_burst_sync_find_frame_start_at_sc16_host": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64]),
        "gfdm_hip_burst_sync_find_frame_start_at_sc16_device": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp]),
        "gfdm_hip_burst_sync_detect_sc16_host": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, f32, i64, i64, i64]),
        "gfdm_hip_burst_sync_detect_sc16_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, f32, i64, i64, i64, vp, vp]),
        "gfdm_hip_burst_extractor_extract_sc16_host": (i32, [vp, vp, vp, i64, vp, vp, vp, i64]),
        "gfdm_hip_burst_extractor_extract_sc16_device": (i32, [vp, vp, vp, i64, vp, vp, vp, i64, vp]),
        "gfdm_hip_burst_shaper_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, f32, f32, i32]),
        "gfdm_hip_burst_shaper_destroy": (i32, [vp]),
        "gfdm_hip_burst_shaper_frame_len": (i32, [vp]),
        "gfdm_hip_burst_shaper_pre_padding": (i32, [vp]),
        "gfdm_hip_burst_shaper_post_padding": (i32, [vp]),
        "gfdm_hip_burst_shaper_scale": (i32, [vp, vp]),
        "gfdm_hip_burst_shaper_check": (i32, [i32, i32, i32, f64, i64, i64]),
        "gfdm_hip_burst_shaper_workspace_bytes": (i64, [vp, i64, i64]),
        "gfdm_hip_burst_shaper_shape_host": (i32, [vp, vp, vp, i64]),
        "gfdm_hip_burst_shaper_shape_device": (i32, [vp, vp, vp, i64, vp, vp]),
        "gfdm_hip_burst_shaper_shape_sc16_host": (i32, [vp, vp, vp, i64, f64]),
        "gfdm_hip_burst_shaper_shape_sc16_device": (i32, [vp, vp, vp, i64, f64, vp, vp]),
        "gfdm_hip_burst_shaper_place_host": (i32, [vp, vp, i64, vp, vp, vp, i64]),
        "gfdm_hip_burst_shaper_place_device": (i32, [vp, vp, i64, vp, vp, vp, i64, vp, vp]),
        "gfdm_hip_burst_shaper_place_sc16_host": (i32, [vp, vp, i64, vp, vp, vp, i64, f64]),
        "gfdm_hip_burst_shaper_place_sc16_device": (i32, [vp, vp, i64, vp, vp, vp, i64, f64, vp, vp]),
        "gfdm_hip_symbol_mapper_create": (i32, [ctypes.POINTER(vp), vp, i32, i32, i32]),
        "gfdm_hip_symbol_mapper_destroy": (i32, [vp]),
        "gfdm_hip_symbol_mapper_bits_per_symbol": (i32, [vp]),
        "gfdm_hip_symbol_mapper_n_points": (i32, [vp]),
        "gfdm_hip_symbol_mapper_decision": (i32, [vp]),
        "gfdm_hip_symbol_mapper_points": (i32, [vp, vp]),
        "gfdm_hip_symbol_mapper_row_bytes": (i64, [vp, i64]),
        "gfdm_hip_symbol_mapper_check": (i32, [i32, i64, i64]),
        "gfdm_hip_symbol_mapper_map_host": (i32, [vp, vp, vp, vp, i64, i64]),
        "gfdm_hip_symbol_mapper_map_device": (i32, [vp, vp, vp, vp, i64, i64, vp]),
        "gfdm_hip_symbol_mapper_decode_host": (i32, [vp, vp, vp, vp, i64, i64]),
        "gfdm_hip_symbol_mapper_decode_device": (i32, [vp, vp, vp, vp, i64, i64, vp]),
        "gfdm_hip_symbol_mapper_soft_host": (i32, [vp, vp, vp, vp, vp, i64, i64]),
        "gfdm_hip_symbol_mapper_soft_device": (i32, [vp, vp, vp, vp, vp, i64, i64, vp]),
        "gfdm_hip_channel_model_create": (i32, [ctypes.POINTER(vp), vp, i32, f64, f64, u64, i32]),
        "gfdm_hip_channel_model_destroy": (i32, [vp]),
        "gfdm_hip_channel_model_n_taps": (i32, [vp]),
        "gfdm_hip_channel_model_taps": (i32, [vp, vp]),
        "gfdm_hip_channel_model_frequency_offset": (i32, [vp, ctypes.POINTER(f64)]),
        "gfdm_hip_channel_model_noise_voltage": (i32, [vp, ctypes.POINTER(f64)]),
        "gfdm_hip_channel_model_seed": (i32, [vp, ctypes.POINTER(u64)]),
        "gfdm_hip_channel_model_set_frequency_offset": (i32, [vp, f64]),
        "gfdm_hip_channel_model_set_noise_voltage": (i32, [vp, f64]),
        "gfdm_hip_channel_model_set_seed": (i32, [vp, u64]),
        "gfdm_hip_channel_model_check": (i32, [i32, f64, f64, i64, i64, i64, f64]),
        "gfdm_hip_channel_model_apply_host": (i32, [vp, vp, vp, i64, i64, i64]),
        "gfdm_hip_channel_model_apply_device": (i32, [vp, vp, vp, i64, i64, i64, vp]),
        "gfdm_hip_channel_model_apply_sc16_host": (i32, [vp, vp, vp, i64, i64, i64, f64]),
        "gfdm_hip_channel_model_apply_sc16_device": (i32, [vp, vp, vp, i64, i64, i64, f64, vp]),
        "gfdm_hip_link_meter_create": (i32, [ctypes.POINTER(vp), vp, i32, i32, i32]),
        "gfdm_hip_link_meter_destroy": (i32, [vp]),
        "gfdm_hip_link_meter_bits_per_symbol": (i32, [vp]),
        "gfdm_hip_link_meter_n_points": (i32, [vp]),
        "gfdm_hip_link_meter_decision": (i32, [vp]),
        "gfdm_hip_link_meter_row_bytes": (i64, [vp, i64]),
        "gfdm_hip_link_meter_totals_device": (vp, [vp]),
        "gfdm_hip_link_meter_reset": (i32, [vp, vp]),
        "gfdm_hip_link_meter_totals": (i32, [vp, vp, vp]),
        "gfdm_hip_link_meter_match_workspace_bytes": (i64, [i64]),
        "gfdm_hip_link_meter_measure_workspace_bytes": (i64, [i64, i64]),
        "gfdm_hip_link_meter_match_host": (i32, [vp, vp, vp, vp, vp, i64, vp, i64, i64, i64]),
        "gfdm_hip_link_meter_match_device": (i32, [vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, vp, vp]),
        "gfdm_hip_link_meter_measure_host": (i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, i64]),
        "gfdm_hip_link_meter_measure_device": (i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, i64, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here == the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    L._gfdm_symbols = sorted(sig)
    # background builds must not outlive the interpreter's tear-down of the HIP runtime (gfdm_hip_quiesce: include/gfdm_hip.h)
    import atexit
    atexit.register(L.gfdm_hip_quiesce)
    _lib = L
    return L


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


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.complex64)


def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _dev_ptr(t, n_elems, what, device=None):
    import torch
    if not t.is_cuda or t.dtype != torch.complex64 or not t.is_contiguous():
        raise TypeError("%s must be a contiguous complex64 CUDA/HIP tensor" % what)
    if device is not None and t.device.index != device:
        raise RuntimeError("%s lives on GPU %d, the kernel handle on GPU %d" % (what, t.device.index, device))
    if t.numel() != n_elems:
        raise RuntimeError("%s has %d elements, expected %d" % (what, t.numel(), n_elems))
    return t.data_ptr()


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
    a = _sc16_pairs(a.shape, "iq", a.reshape)
    out = np.empty(a.shape[0], np.complex64)
    out.real = a[:, 0]
    out.imag = a[:, 1]
    return out


def _sc16_pairs(shape, what, reshape=None):
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


def _capture(samples, device, what="samples"):
    """A capture argument -> (pointer, n_samples, name infix, keep-alive): complex64 (anything _c64 takes on the host path, a contiguous
    complex64 tensor on the device path: infix "") or sc16 (a contiguous int16 array / tensor of shape (n, 2) or (2n,): infix "_sc16",
    passed on as it is, never widened).  Any other integer dtype is a TypeError.  Checks come before anything touches the device."""
    if _is_tensor(samples):
        import torch
        if samples.dtype == torch.int16:
            n = _sc16_pairs(samples.shape, what)
            if not samples.is_cuda or not samples.is_contiguous():
                raise TypeError("%s must be a contiguous int16 CUDA/HIP tensor" % what)
            if samples.device.index != device:
                raise RuntimeError("%s lives on GPU %d, the kernel handle on GPU %d" % (what, samples.device.index, device))
            return samples.data_ptr(), n, "_sc16", samples
        if not (samples.dtype.is_floating_point or samples.dtype.is_complex):
            raise TypeError("%s: integer captures must be int16 (sc16), not %s" % (what, samples.dtype))
        return _dev_ptr(samples, samples.numel(), what, device), samples.numel(), "", samples
    a = np.asarray(samples)
    if a.dtype == np.int16:
        n = _sc16_pairs(a.shape, what)
        if not a.flags.c_contiguous:
            raise TypeError("%s must be a C-contiguous int16 array" % what)
        return a.ctypes.data, n, "_sc16", a
    if np.issubdtype(a.dtype, np.integer):
        raise TypeError("%s: integer captures must be int16 (sc16), not %s" % (what, a.dtype))
    a = _c64(a).ravel()
    return a.ctypes.data, a.size, "", a


def _stream_ptr(stream, device=None):
    if stream is None:
        import torch
        return torch.cuda.current_stream(device).cuda_stream      # the current stream of the HANDLE's GPU, not of torch's current one
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


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


PAGE = mmap.PAGESIZE


def aligned_empty(shape, dtype=np.complex64):
    """An uninitialised C-contiguous array that starts on a page boundary and owns its pages to the end of the last one: what register_host takes
    (gfdm_hip_register_host pins whole pages).  The backing buffer stays alive with the array."""
    import mmap
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


class _Kernel:
    """Shared plumbing: host (numpy) and device (torch) batched calls."""
    _destroy = None
    _dev = 0                       # GPU the handle was created on: every tensor and the stream of a call must belong to it

    def _dp(self, t, n_elems, what):
        return _dev_ptr(t, n_elems, what, self._dev)

    def _sp(self, stream):
        return _stream_ptr(stream, self._dev)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None and self._destroy:
            getattr(_lib, self._destroy)(h)
            self._h = None

    def _nblocks(self, size, what="Input"):
        n = self.block_size()
        if size % n:
            raise RuntimeError("%s vector size(%d) MUST be a multiple of block_size(%d)!" % (what, size, n))
        return size // n

    def _host(self, fn, x, extra=(), extra_ok_none=False, out=None):
        """numpy path: the *_host entry point on the arrays' memory.  `out`: an existing complex64 array to write into (e.g. one registered with
        register_host, so that the call runs in place on it)."""
        x = _c64(x)
        nb = self._nblocks(x.size)
        ptrs = []
        keep = []
        for e in extra:
            if e is None:
                if not extra_ok_none:
                    raise RuntimeError("missing input vector")
                ptrs.append(None)
            else:
                e = _c64(e)
                if e.size != x.size:
                    raise RuntimeError("Channel vector size(%d) MUST be equal to input size(%d)!" % (e.size, x.size))
                keep.append(e)
                ptrs.append(e.ctypes.data)
        if out is None:
            out = np.empty(x.shape, np.complex64)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.flags.c_contiguous and out.size == x.size):
            raise TypeError("out must be a C-contiguous complex64 numpy array of the input's size")
        _check(fn(self._h, out.ctypes.data, x.ctypes.data, *ptrs, nb))
        return out

    def _device(self, fn, out, x, extra=(), stream=None):
        n = x.numel()
        nb = self._nblocks(n)
        ptrs = [None if e is None else self._dp(e, n, "extra input") for e in extra]
        _check(fn(self._h, self._dp(out, n, "out"), self._dp(x, n, "in"), *ptrs, nb, self._sp(stream)))
        return out


class _Receiver(_Kernel):
    """What Demodulator and AdvancedReceiver share: frames in / demapped symbols out, the fused channel estimator, bursts straight from a
    capture.  The C-ABI names are <_stem>_<name> for the settings and <_stem>_<_verb>_<call kind>[_sc16]_{host,device} for the calls."""
    _stem = None                   # "gfdm_hip_receiver" | "gfdm_hip_advanced_receiver"
    _verb = None                   # "demodulate" | "work"

    def _fn(self, name):
        return getattr(lib(), self._stem + "_" + name)

    @property
    def _bursts_prefix(self):
        return "%s_%s_bursts" % (self._stem, self._verb)

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
        if _is_tensor(frames):
            import torch
            if frames.numel() % frame_len:
                raise RuntimeError("frames size(%d) MUST be a multiple of frame_len(%d)!" % (frames.numel(), frame_len))
            nb = frames.numel() // frame_len
            out = torch.empty(nb, nout, dtype=torch.complex64, device=frames.device) if out is None else out
            feq = None if f_eq is None else self._dp(f_eq, nb * N, "f_eq")
            _check(self._fn(self._verb + "_frames_device")(self._h, self._dp(out, nb * nout, "out"), self._dp(frames, nb * frame_len, "frames"),
                                                        feq, nout_arg, nb, self._sp(stream)))
            return out
        x = _c64(frames)
        if x.size % frame_len:
            raise RuntimeError("frames size(%d) MUST be a multiple of frame_len(%d)!" % (x.size, frame_len))
        nb = x.size // frame_len
        e = None if f_eq is None else _c64(f_eq)
        if e is not None and e.size != nb * N:
            raise RuntimeError("Channel vector size(%d) MUST be equal to nframes * block_size(%d)!" % (e.size, nb * N))
        res = np.empty((nb, nout), np.complex64)
        _check(self._fn(self._verb + "_frames_host")(self._h, res.ctypes.data, x.ctypes.data, None if e is None else e.ctypes.data, nout_arg, nb))
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
        if _is_tensor(x):
            import torch
            if x.numel() % n_in:
                raise RuntimeError("Input size(%d) MUST be a multiple of %d!" % (x.numel(), n_in))
            nb = x.numel() // n_in
            out = torch.empty(nb, nout, dtype=torch.complex64, device=x.device) if out is None else out
            need = (nb - 1) * stride + 2 * fft_len if nb else 0
            if rx_preamble.numel() < need:
                raise RuntimeError("rx_preamble has %d elements, at least %d are needed" % (rx_preamble.numel(), need))
            self._dp(rx_preamble, rx_preamble.numel(), "rx_preamble")
            _check(self._fn(self._verb + "_estimated_device")(self._h, self._dp(out, nb * nout, "out"), self._dp(x, nb * n_in, "in"),
                                                              rx_preamble.data_ptr(), int(preamble_stride), nout_arg, nb, self._sp(stream)))
            return out
        a = _c64(x)
        if a.size % n_in:
            raise RuntimeError("Input size(%d) MUST be a multiple of %d!" % (a.size, n_in))
        nb = a.size // n_in
        pre = _c64(rx_preamble)
        need = (nb - 1) * stride + 2 * fft_len if nb else 0
        if pre.size < need:
            raise RuntimeError("rx_preamble size(%d) MUST be at least %d!" % (pre.size, need))
        res = np.empty((nb, nout), np.complex64)
        _check(self._fn(self._verb + "_estimated_host")(self._h, res.ctypes.data, a.ctypes.data, pre.ctypes.data, int(preamble_stride), nout_arg, nb))
        return res

    def demodulate_bursts(self, samples, offsets, sc_rot=None, count=None, backoff=0, preamble_offset=0, cfo_correction=True, noutput_size=None,
                          out=None, stream=None):
        """The bursts at `offsets` of the capture `samples`, demodulated straight from it: BurstExtractor.extract (offset - backoff, zero
        outside the capture, CFO rotation by sc_rot) as the load stage of demodulate_estimated, preamble at preamble_offset of each burst.
        Needs configure_frames and set_channel_estimator.  count (one int64, e.g. detect's): rows from count on are zeros.
        r = sync.detect(...) feeds it as demodulate_bursts(samples, r["frame_start"], r["sc_rot"], r["count"], ...).
        Torch device tensors run the device entry point (no allocation beyond `out`, no synchronisation), numpy arrays the host one.
        An int16 capture, shape (n, 2) or (2n,), is read as sc16 (the *_sc16_* entry points): bit-equal to the call on from_sc16(samples)."""
        sptr, slen, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        if getattr(self, "_estimator", None) is None:
            raise ValueError("set_channel_estimator has not been called on this handle")
        nout_arg = -1 if noutput_size is None else int(noutput_size)
        _, nout, _ = self._layout(True, nout_arg)
        args = (int(backoff), int(preamble_offset), int(bool(cfo_correction)), nout_arg)
        if _is_tensor(samples):
            import torch
            n = offsets.numel()
            out = torch.empty(n, nout, dtype=torch.complex64, device=samples.device) if out is None else out
            rp = None if sc_rot is None else _dev_arg(sc_rot, torch.complex64, n, "sc_rot", self._dev)
            cp = None if count is None else _dev_arg(count, torch.int64, 1, "count", self._dev)
            _check(getattr(L, self._bursts_prefix + fmt + "_device")(self._h, self._dp(out, n * nout, "out"), sptr, slen,
                                                                    _dev_arg(offsets, torch.int64, n, "offsets", self._dev), rp, cp, *args, n,
                                                                    self._sp(stream)))
            return out
        off = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        n = off.size
        rot = None if sc_rot is None else _c64(sc_rot).ravel()
        if rot is not None and rot.size != n:
            raise RuntimeError("sc_rot has %d elements, expected %d" % (rot.size, n))
        cnt = None if count is None else np.ascontiguousarray(count, dtype=np.int64).ravel()
        if cnt is not None and cnt.size != 1:
            raise RuntimeError("count has %d elements, expected 1" % cnt.size)
        res = np.empty((n, nout), np.complex64)
        _check(getattr(L, self._bursts_prefix + fmt + "_host")(self._h, res.ctypes.data, sptr, slen, off.ctypes.data,
                                                              None if rot is None else rot.ctypes.data, None if cnt is None else cnt.ctypes.data, *args, n))
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
        if _is_tensor(x):
            import torch
            out = torch.empty_like(x) if out is None else out
            return self._device(lib().gfdm_hip_modulator_work_device, out, x, stream=stream)
        return self._host(lib().gfdm_hip_modulator_work_host, x, out=out)


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

    def _call(self, name, x, extra, out, stream, extra_ok_none=False):
        L = lib()
        if _is_tensor(x):
            import torch
            out = torch.empty_like(x) if out is None else out
            return self._device(getattr(L, name + "_device"), out, x, extra, stream)
        return self._host(getattr(L, name + "_host"), x, extra, extra_ok_none, out=out)

    def demodulate(self, x, out=None, stream=None):
        return self._call("gfdm_hip_receiver_demodulate", x, (None,), out, stream, True)

    def demodulate_equalize(self, x, f_eq, out=None, stream=None):
        return self._call("gfdm_hip_receiver_demodulate", x, (f_eq,), out, stream)

    def fft_filter_downsample(self, x, out=None, stream=None):
        return self._call("gfdm_hip_receiver_fft_filter_downsample", x, (None,), out, stream, True)

    def fft_equalize_filter_downsample(self, x, f_eq, out=None, stream=None):
        return self._call("gfdm_hip_receiver_fft_filter_downsample", x, (f_eq,), out, stream)

    def transform_subcarriers_to_td(self, x, out=None, stream=None):
        return self._call("gfdm_hip_receiver_transform_subcarriers_to_td", x, (), out, stream)

    def cancel_sc_interference(self, td, fd, out=None, stream=None):
        return self._call("gfdm_hip_receiver_cancel_sc_interference", td, (fd,), out, stream)


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

    def _call(self, x, f_eq, out, stream):
        L = lib()
        if _is_tensor(x):
            import torch
            out = torch.empty_like(x) if out is None else out
            return self._device(L.gfdm_hip_advanced_receiver_work_device, out, x, (f_eq,), stream)
        return self._host(L.gfdm_hip_advanced_receiver_work_host, x, (f_eq,), True, out=out)

    def demodulate(self, x, out=None, stream=None):
        """generic_work: IC receiver without equaliser."""
        return self._call(x, None, out, stream)

    def demodulate_equalize(self, x, f_eq, out=None, stream=None):
        """generic_work_equalize: one f_eq vector per block."""
        return self._call(x, f_eq, out, stream)


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
        size = x.numel() if _is_tensor(x) else np.asarray(x).size
        if n <= 0 or size % n:
            raise RuntimeError("input size(%d) MUST be a multiple of ninput_size(%d)!" % (size, n))
        return n, size // n

    def transmit(self, symbols, ninput_size=None, n_ports=None, stream=None, outs=None):
        """All ports (or the first n_ports): list of (nblocks, output_vector_size) arrays / tensors, one per cyclic shift.
        `outs` (device path only): one tensor of nblocks * output_vector_size elements per port to write into."""
        L = lib()
        n, nb = self._split(symbols, ninput_size)
        ports = len(self._shifts) if n_ports is None else n_ports
        F = self.output_vector_size()
        if _is_tensor(symbols):
            import torch
            if outs is None:
                outs = [torch.empty(nb, F, dtype=torch.complex64, device=symbols.device) for _ in range(ports)]
            elif len(outs) != ports:
                raise RuntimeError("outs has %d tensors, expected one per port (%d)" % (len(outs), ports))
            outs = list(outs)
            arr = (ctypes.c_void_p * ports)(*[self._dp(o, nb * F, "outs[%d]" % i) for i, o in enumerate(outs)])
            _check(L.gfdm_hip_transmitter_work_device(self._h, arr, ports, self._dp(symbols, nb * n, "in"), n, nb, self._sp(stream)))
            return outs
        if outs is not None:
            raise TypeError("outs is for device tensors; the numpy path returns new arrays")
        x = _c64(symbols)
        outs = [np.empty((nb, F), np.complex64) for _ in range(ports)]
        arr = (ctypes.c_void_p * ports)(*[o.ctypes.data for o in outs])
        _check(L.gfdm_hip_transmitter_work_host(self._h, arr, ports, x.ctypes.data, n, nb))
        return outs

    def generic_work(self, symbols, ninput_size=None):
        """transmitter_kernel::generic_work: the frame of cyclic_shifts[0]."""
        return self.transmit(symbols, ninput_size, 1)[0]

    def modulate(self, symbols, ninput_size=None, stream=None, out=None):
        L = lib()
        n, nb = self._split(symbols, ninput_size)
        N = self.block_size()
        if _is_tensor(symbols):
            import torch
            out = torch.empty(nb, N, dtype=torch.complex64, device=symbols.device) if out is None else out
            _check(L.gfdm_hip_transmitter_modulate_device(self._h, self._dp(out, nb * N, "out"), self._dp(symbols, nb * n, "in"), n, nb, self._sp(stream)))
            return out
        if out is not None:
            raise TypeError("out is for device tensors; the numpy path returns a new array")
        x = _c64(symbols)
        out = np.empty((nb, N), np.complex64)
        _check(L.gfdm_hip_transmitter_modulate_host(self._h, out.ctypes.data, x.ctypes.data, n, nb))
        return out

    def add_frame(self, blocks, cyclic_shift, stream=None, out=None):
        L = lib()
        N, F = self.block_size(), self.output_vector_size()
        if _is_tensor(blocks):
            import torch
            nb = blocks.numel() // N
            out = torch.empty(nb, F, dtype=torch.complex64, device=blocks.device) if out is None else out
            _check(L.gfdm_hip_transmitter_add_frame_device(self._h, self._dp(out, nb * F, "out"), self._dp(blocks, nb * N, "in"), int(cyclic_shift), nb, self._sp(stream)))
            return out
        if out is not None:
            raise TypeError("out is for device tensors; the numpy path returns a new array")
        x = _c64(blocks)
        nb = x.size // N
        out = np.empty((nb, F), np.complex64)
        _check(L.gfdm_hip_transmitter_add_frame_host(self._h, out.ctypes.data, x.ctypes.data, int(cyclic_shift), nb))
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

    def _run(self, host, dev, x, n_in, n_out, size_arg, stream, out=None):
        size = x.numel() if _is_tensor(x) else np.asarray(x).size
        if n_in <= 0 or size % n_in:
            raise RuntimeError("input size(%d) MUST be a multiple of %d!" % (size, n_in))
        nb = size // n_in
        if _is_tensor(x):
            import torch
            if out is None:
                out = torch.empty(nb, n_out, dtype=torch.complex64, device=x.device)
            _check(dev(self._h, self._dp(out, nb * n_out, "out"), self._dp(x, size, "in"), size_arg, nb, self._sp(stream)))
            return out
        a = _c64(x)
        out = np.empty((nb, n_out), np.complex64)
        _check(host(self._h, out.ctypes.data, a.ctypes.data, size_arg, nb))
        return out[0] if (np.asarray(x).ndim == 1 and nb == 1) else out

    def map_to_resources(self, symbols, ninput_size=None, stream=None, out=None):
        """ninput_size symbols per block (default block_size) -> frame_size grid values per block, unfilled slots zero."""
        n = self.block_size() if ninput_size is None else int(ninput_size)
        if n == 0:
            raise RuntimeError("ninput_size 0: give the number of blocks through a [nblocks][0] input of the C-ABI instead")
        L = lib()
        return self._run(L.gfdm_hip_resource_mapper_map_host, L.gfdm_hip_resource_mapper_map_device, symbols, n, self.frame_size(), n, stream, out)

    def demap_from_resources(self, grid, noutput_size=None, stream=None, out=None):
        n = self.block_size() if noutput_size is None else int(noutput_size)
        L = lib()
        return self._run(L.gfdm_hip_resource_mapper_demap_host, L.gfdm_hip_resource_mapper_demap_device, grid, self.frame_size(), n, n, stream, out)


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

    def _batch(self, x, n_in):
        size = x.numel() if _is_tensor(x) else np.asarray(x).size
        if size % n_in:
            raise RuntimeError("input size(%d) MUST be a multiple of %d!" % (size, n_in))
        return size, size // n_in

    def add_cyclic_prefix(self, blocks, cyclic_shift=None, stream=None, out=None):
        L = lib()
        s = self.cyclic_shift() if cyclic_shift is None else int(cyclic_shift)
        N, F = self.block_size(), self.frame_size()
        size, nb = self._batch(blocks, N)
        if _is_tensor(blocks):
            import torch
            if out is None:
                out = torch.empty(nb, F, dtype=torch.complex64, device=blocks.device)
            _check(L.gfdm_hip_cyclic_prefixer_add_device(self._h, self._dp(out, nb * F, "out"), self._dp(blocks, size, "in"), s, nb, self._sp(stream)))
            return out
        a = _c64(blocks)
        out = np.empty((nb, F), np.complex64)
        _check(L.gfdm_hip_cyclic_prefixer_add_host(self._h, out.ctypes.data, a.ctypes.data, s, nb))
        return out[0] if (np.asarray(blocks).ndim == 1 and nb == 1) else out

    generic_work = add_cyclic_prefix

    def remove_cyclic_prefix(self, frames, stream=None, out=None):
        L = lib()
        N, F = self.block_size(), self.frame_size()
        size, nb = self._batch(frames, F)
        if _is_tensor(frames):
            import torch
            if out is None:
                out = torch.empty(nb, N, dtype=torch.complex64, device=frames.device)
            _check(L.gfdm_hip_cyclic_prefixer_remove_device(self._h, self._dp(out, nb * N, "out"), self._dp(frames, size, "in"), nb, self._sp(stream)))
            return out
        a = _c64(frames)
        out = np.empty((nb, N), np.complex64)
        _check(L.gfdm_hip_cyclic_prefixer_remove_host(self._h, out.ctypes.data, a.ctypes.data, nb))
        return out[0] if (np.asarray(frames).ndim == 1 and nb == 1) else out


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

    def _run(self, name, x, n_in, n_out, stream):
        L = lib()
        if _is_tensor(x):
            import torch
            if x.numel() % n_in:
                raise RuntimeError("Input size %d is not a multiple of %d" % (x.numel(), n_in))
            nf = x.numel() // n_in
            out = torch.empty((nf, n_out) if x.dim() > 1 or nf != 1 else (n_out,), dtype=torch.complex64, device=x.device)
            _check(getattr(L, name + "_device")(self._h, out.data_ptr(), self._dp(x, nf * n_in, "in"), nf, self._sp(stream)))
            return out
        a = _c64(x)
        if a.size % n_in:
            raise RuntimeError("Input size %d is not a multiple of %d" % (a.size, n_in))
        nf = a.size // n_in
        out = np.empty((nf, n_out) if a.ndim > 1 or nf != 1 else (n_out,), np.complex64)
        _check(getattr(L, name + "_host")(self._h, out.ctypes.data, a.ctypes.data, nf))
        return out

    def estimate_frame(self, rx_preamble, stream=None):
        n = self._lens()
        return self._run("gfdm_hip_channel_estimator_estimate_frame", rx_preamble, n["rx"], n["frame"], stream)

    def estimate_preamble_channel(self, rx_preamble, stream=None):
        n = self._lens()
        return self._run("gfdm_hip_channel_estimator_estimate_preamble_channel", rx_preamble, n["rx"], n["est"], stream)

    def filter_preamble_estimate(self, estimate, stream=None):
        n = self._lens()
        return self._run("gfdm_hip_channel_estimator_filter_preamble_estimate", estimate, n["est"], n["filt"], stream)

    def interpolate_frame(self, filtered, stream=None):
        n = self._lens()
        return self._run("gfdm_hip_channel_estimator_interpolate_frame", filtered, n["filt"], n["frame"], stream)

    def prepare_for_zf(self, frame_estimate, stream=None):
        n = self._lens()
        return self._run("gfdm_hip_channel_estimator_prepare_for_zf", frame_estimate, n["frame"], n["frame"], stream)

    def estimate_snr(self, rx_preamble, stream=None):
        """(snr_lin, cnrs): scalars / [active] for one preamble, [nframes] / [nframes][active] for a batch."""
        L = lib()
        n_in, A = 2 * self.fft_len(), self.active_subcarriers()
        if _is_tensor(rx_preamble):
            import torch
            nf = rx_preamble.numel() // n_in
            snr = torch.empty(nf, dtype=torch.float32, device=rx_preamble.device)
            cnrs = torch.empty(nf, A, dtype=torch.float32, device=rx_preamble.device)
            _check(L.gfdm_hip_channel_estimator_estimate_snr_device(self._h, snr.data_ptr(), cnrs.data_ptr(), self._dp(rx_preamble, nf * n_in, "in"),
                                                                    nf, self._sp(stream)))
            return snr, cnrs
        a = _c64(rx_preamble)
        if a.size % n_in:
            raise RuntimeError("Input size %d is not a multiple of %d" % (a.size, n_in))
        nf = a.size // n_in
        snr = np.empty(nf, np.float32)
        cnrs = np.empty((nf, A), np.float32)
        _check(L.gfdm_hip_channel_estimator_estimate_snr_host(self._h, snr.ctypes.data, cnrs.ctypes.data, a.ctypes.data, nf))
        if a.ndim <= 1 and nf == 1:
            return float(snr[0]), cnrs[0]
        return snr, cnrs


def threshold_factor(false_alarm_prob):
    """pygfdm's calculate_threshold_factor (python/pygfdm/synchronization.py:239-243): sqrt(-(4 / pi) ln p), the detection threshold
    relative to the noise level for a false-alarm probability p < 1."""
    if not false_alarm_prob < 1.0:
        raise ValueError("False alarm probability MUST be smaller 1.0!")
    return float(np.sqrt(-(4 / np.pi) * np.log(false_alarm_prob)))


def _dev_arg(t, dtype, n_elems, what, device):
    """device pointer of a contiguous torch tensor of `dtype` with n_elems elements on `device`"""
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise TypeError("%s must be a contiguous %s CUDA/HIP tensor" % (what, dtype))
    if t.device.index != device:
        raise RuntimeError("%s lives on GPU %d, the handle on GPU %d" % (what, t.device.index, device))
    if t.numel() != n_elems:
        raise RuntimeError("%s has %d elements, expected %d" % (what, t.numel(), n_elems))
    return t.data_ptr()


class BurstSync(_Kernel):
    """Preamble timing / CFO synchronisation: pygfdm's find_frame_start (python/pygfdm/synchronization.py:154-263) on every window
    stream[first + b * stride : ... + window_len] of a capture buffer (contract in include/gfdm_hip.h).  numpy samples -> numpy results
    (host path), a torch complex64 device tensor -> torch results on its device (device path, current stream unless given).  Every call that
    takes `samples` also takes an sc16 capture -- int16 I/Q of shape (n, 2) or (2n,), numpy or torch -- and reads it as it is (the *_sc16_*
    entry points): bit-equal to the call on from_sc16(samples)."""
    _destroy = "gfdm_hip_burst_sync_destroy"

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

    def find_frame_start(self, samples, first=0, stride=None, n_windows=1, stream=None):
        """dict of per-window arrays: frame_start, coarse (stream indices, int64), cfo, metric (float32), sc_rot (complex64).
        stride defaults to window_len (windows back to back)."""
        sptr, n, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        first, stride, nw = self._grid(first, stride, n_windows)
        if _is_tensor(samples):
            r = self._outputs(nw, samples.device)
            _check(getattr(L, "gfdm_hip_burst_sync_find_frame_start%s_device" % fmt)(self._h, *[r[k].data_ptr() for k in self._OUT], sptr, n, first, stride, nw,
                                                                                    self._sp(stream)))
            return r
        r = self._outputs(nw)
        _check(getattr(L, "gfdm_hip_burst_sync_find_frame_start%s_host" % fmt)(self._h, *[r[k].ctypes.data for k in self._OUT], sptr, n, first, stride, nw))
        return r

    _OUT = ("frame_start", "coarse", "cfo", "metric", "sc_rot")

    @staticmethod
    def _outputs(n, device=None):
        """the five per-window result arrays: torch tensors on `device`, numpy arrays without one"""
        if device is None:
            return {"frame_start": np.empty(n, np.int64), "coarse": np.empty(n, np.int64), "cfo": np.empty(n, np.float32),
                    "metric": np.empty(n, np.float32), "sc_rot": np.empty(n, np.complex64)}
        import torch
        return {"frame_start": torch.empty(n, dtype=torch.int64, device=device), "coarse": torch.empty(n, dtype=torch.int64, device=device),
                "cfo": torch.empty(n, dtype=torch.float32, device=device), "metric": torch.empty(n, dtype=torch.float32, device=device),
                "sc_rot": torch.empty(n, dtype=torch.complex64, device=device)}

    def find_frame_start_at(self, samples, starts, stream=None):
        """find_frame_start on the windows samples[st : st + window_len], st = clamp(starts[w], 0, len(samples) - window_len): the same
        dict, bit-equal per window to find_frame_start(first=st).  starts: int64 (a device tensor when samples is one)."""
        sptr, n, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        if _is_tensor(samples):
            import torch
            nw = starts.numel()
            r = self._outputs(nw, samples.device)
            _check(getattr(L, "gfdm_hip_burst_sync_find_frame_start_at%s_device" % fmt)(self._h, *[r[k].data_ptr() for k in self._OUT], sptr, n,
                                                                                       _dev_arg(starts, torch.int64, nw, "starts", self._dev), nw,
                                                                                       self._sp(stream)))
            return r
        st = np.ascontiguousarray(starts, dtype=np.int64).ravel()
        r = self._outputs(st.size)
        _check(getattr(L, "gfdm_hip_burst_sync_find_frame_start_at%s_host" % fmt)(self._h, *[r[k].ctypes.data for k in self._OUT], sptr, n, st.ctypes.data,
                                                                                 st.size))
        return r

    def detect(self, samples, threshold, min_distance, lead=None, max_bursts=None, stream=None):
        """Every burst of a stream (contract in include/gfdm_hip.h): peaks of ic over the whole stream that reach `threshold` and are
        the first maximum within +-min_distance, in ascending position; each one's window starts `lead` before it.  Returns a dict:
        count (total peaks found: int on the host path, a one-element int64 tensor on the device path, which does not synchronise) and
        the five find_frame_start arrays with max_bursts slots, those from min(count, max_bursts) on at frame_start = coarse = -1.
        Defaults: lead = cp_len + fft_len // 2, max_bursts = ceil(P / (min_distance + 1)), the most peaks P positions can hold."""
        sptr, n, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        R = int(min_distance)
        lead = self.cp_len() + self.fft_len() // 2 if lead is None else int(lead)
        if max_bursts is None:
            max_bursts = max(0, -(-(n - 2 * self.fft_len()) // (max(R, 0) + 1)))
        nb = int(max_bursts)
        _check(L.gfdm_hip_burst_sync_detect_check(self.fft_len(), self.cp_len(), self.window_len(), n, threshold, R, lead, nb))
        if _is_tensor(samples):
            import torch
            d = samples.device
            r = self._outputs(nb, d)
            count = torch.empty(1, dtype=torch.int64, device=d)
            ws = torch.empty(L.gfdm_hip_burst_sync_detect_workspace_bytes(self._h, n), dtype=torch.uint8, device=d)
            _check(getattr(L, "gfdm_hip_burst_sync_detect%s_device" % fmt)(self._h, count.data_ptr(), *[r[k].data_ptr() for k in self._OUT], sptr, n,
                                                                          threshold, R, lead, nb, ws.data_ptr(), self._sp(stream)))
            r["count"] = count
            return r
        r = self._outputs(nb)
        count = np.zeros(1, np.int64)
        _check(getattr(L, "gfdm_hip_burst_sync_detect%s_host" % fmt)(self._h, count.ctypes.data, *[r[k].ctypes.data for k in self._OUT], sptr, n, threshold, R,
                                                                    lead, nb))
        r["count"] = int(count[0])
        return r

    def auto_correlate(self, samples, first=0, stride=None, n_windows=1, stream=None):
        """(ac, ic): [n_windows][corr_len] complex64 / float32 (pygfdm's auto_correlate_signal and abs_integrate)."""
        sptr, n, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        first, stride, nw = self._grid(first, stride, n_windows)
        P = self.corr_len()
        if _is_tensor(samples):
            import torch
            ac = torch.empty(nw, P, dtype=torch.complex64, device=samples.device)
            ic = torch.empty(nw, P, dtype=torch.float32, device=samples.device)
            _check(getattr(L, "gfdm_hip_burst_sync_auto_correlate%s_device" % fmt)(self._h, ac.data_ptr(), ic.data_ptr(), sptr, n, first, stride, nw,
                                                                                  self._sp(stream)))
            return ac, ic
        ac = np.empty((nw, P), np.complex64)
        ic = np.empty((nw, P), np.float32)
        _check(getattr(L, "gfdm_hip_burst_sync_auto_correlate%s_host" % fmt)(self._h, ac.ctypes.data, ic.ctypes.data, sptr, n, first, stride, nw))
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
        sptr, slen, fmt, _keep = _capture(samples, self._dev)
        L = lib()
        B = self.burst_len()
        if _is_tensor(samples):
            import torch
            n = offsets.numel()
            out = torch.empty(n, B, dtype=torch.complex64, device=samples.device)
            sp = None if scale is None else _dev_arg(scale, torch.float32, n, "scale", self._dev)
            rp = None if sc_rot is None else _dev_arg(sc_rot, torch.complex64, n, "sc_rot", self._dev)
            _check(getattr(L, "gfdm_hip_burst_extractor_extract%s_device" % fmt)(self._h, out.data_ptr(), sptr, slen,
                                                                                _dev_arg(offsets, torch.int64, n, "offsets", self._dev), sp, rp, n,
                                                                                self._sp(stream)))
            return out
        off = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        n = off.size
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32).ravel()
        rot = None if sc_rot is None else _c64(sc_rot).ravel()
        for v, what in ((sc, "scale"), (rot, "sc_rot")):
            if v is not None and v.size != n:
                raise RuntimeError("%s has %d elements, expected %d" % (what, v.size, n))
        out = np.empty((n, B), np.complex64)
        _check(getattr(L, "gfdm_hip_burst_extractor_extract%s_host" % fmt)(self._h, out.ctypes.data, sptr, slen, off.ctypes.data,
                                                                          None if sc is None else sc.ctypes.data, None if rot is None else rot.ctypes.data, n))
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
    def _peak(sc16, peak):
        if peak is None:
            return 0.0
        if not sc16:
            raise ValueError("peak normalises sc16 output: pass sc16=True (complex64 output is scaled by `scale` alone)")
        if not 0 < peak <= 32767:
            raise ValueError("peak must lie in (0, 32767]")
        return float(peak)

    @staticmethod
    def _kinds(frames, out, sc16, what="frames"):
        """what can be said of frames and out without the handle (kind, dtype, layout): raised before the library is asked"""
        if _is_tensor(frames):
            import torch
            if frames.dtype != torch.complex64 or not frames.is_cuda or not frames.is_contiguous():
                raise TypeError("%s must be a contiguous complex64 CUDA/HIP tensor" % what)
        else:
            a = np.asarray(frames)
            if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.complexfloating)):
                raise TypeError("%s must be complex samples, not %s" % (what, a.dtype))
            frames = _c64(a).ravel()
        if out is not None:
            if _is_tensor(out) != _is_tensor(frames):
                raise TypeError("out must be a %s, as %s is" % ("CUDA/HIP tensor" if _is_tensor(frames) else "numpy array", what))
            if not _is_tensor(out) and not isinstance(out, np.ndarray):
                raise TypeError("out must be a numpy array")
            have = str(out.dtype).replace("torch.", "")
            if have != ("int16" if sc16 else "complex64"):
                raise TypeError("out must be %s, not %s" % ("int16 I/Q (sc16)" if sc16 else "complex64", have))
            contiguous = out.is_contiguous() if _is_tensor(out) else out.flags.c_contiguous
            if not contiguous:
                raise TypeError("out must be contiguous")
            if sc16:
                _sc16_pairs(out.shape, "out")
        return frames

    def _frames(self, frames):
        """n_bursts of the frames of one port: any shape whose size is a multiple of frame_len"""
        F = self.frame_len()
        size = frames.numel() if _is_tensor(frames) else frames.size
        if size % F:
            raise RuntimeError("frames size(%d) MUST be a multiple of frame_len(%d)!" % (size, F))
        return size // F

    def _out(self, out, n, sc16, like):
        """the output array of n samples -- `out` (checked by _kinds), or a new one of `like`'s kind -- and its pointer"""
        if out is None:
            if _is_tensor(like):
                import torch
                out = torch.empty((n, 2) if sc16 else (n,), dtype=torch.int16 if sc16 else torch.complex64, device=like.device)
            else:
                out = np.empty((n, 2) if sc16 else (n,), np.int16 if sc16 else np.complex64)
        have = _sc16_pairs(out.shape, "out") if sc16 else (out.numel() if _is_tensor(out) else out.size)
        if have != n:
            raise RuntimeError("out holds %d samples, expected %d" % (have, n))
        if _is_tensor(out):
            if out.device.index != self._dev:
                raise RuntimeError("out lives on GPU %d, the handle on GPU %d" % (out.device.index, self._dev))
            return out, out.data_ptr()
        return out, out.ctypes.data

    def _workspace(self, ws, like, n, out_len, pk):
        """pointer of the device scratch of a normalised call (`ws`: a uint8 device tensor of workspace_bytes(), or None for a new one)"""
        if not pk:
            return None, None
        import torch
        need = self.workspace_bytes(n, out_len)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=like.device)
        elif not _is_tensor(ws) or ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need or ws.device.index != self._dev:
            raise TypeError("workspace must be a contiguous uint8 CUDA/HIP tensor of at least %d bytes on GPU %d" % (need, self._dev))
        return ws, ws.data_ptr()

    def shape(self, frames, sc16=False, peak=None, out=None, stream=None, workspace=None):
        """n_bursts * slot_len() samples: every frame scaled, behind pre_padding and in front of post_padding zeros.  workspace (device path,
        normalised sc16 only): a uint8 tensor of workspace_bytes() to use instead of a new one; afterwards its first two floats are the gain
        and the largest component found."""
        if isinstance(frames, (list, tuple)):
            if out is not None and len(out) != len(frames):
                raise ValueError("out must hold one array per port")
            return [self.shape(f, sc16, peak, None if out is None else out[p], stream, workspace) for p, f in enumerate(frames)]
        pk = self._peak(sc16, peak)
        frames = self._kinds(frames, out, sc16)
        n = self._frames(frames)
        L = lib()
        _check(L.gfdm_hip_burst_shaper_check(self.frame_len(), self.pre_padding(), self.post_padding(), pk, n, n * self.slot_len()))
        res, optr = self._out(out, n * self.slot_len(), sc16, frames)
        if _is_tensor(frames):
            fptr = self._dp(frames, frames.numel(), "frames")
            ws, wptr = self._workspace(workspace, frames, n, n * self.slot_len(), pk)
            if sc16:
                _check(L.gfdm_hip_burst_shaper_shape_sc16_device(self._h, optr, fptr, n, pk, wptr, self._sp(stream)))
            else:
                _check(L.gfdm_hip_burst_shaper_shape_device(self._h, optr, fptr, n, wptr, self._sp(stream)))
            return res
        if sc16:
            _check(L.gfdm_hip_burst_shaper_shape_sc16_host(self._h, optr, frames.ctypes.data, n, pk))
        else:
            _check(L.gfdm_hip_burst_shaper_shape_host(self._h, optr, frames.ctypes.data, n))
        return res

    def place(self, frames, starts, out_len, count=None, sc16=False, peak=None, out=None, stream=None, workspace=None):
        """out_len samples: frame b from sample starts[b] on (starts ascending, int64; a device tensor when frames is one), zeros
        elsewhere.  count (an int, or on the device path a one-element int64 tensor such as detect's) limits the call to the first
        count frames; it is clamped to [0, n_bursts].  workspace: as in shape()."""
        if isinstance(frames, (list, tuple)):
            if out is not None and len(out) != len(frames):
                raise ValueError("out must hold one array per port")
            return [self.place(f, starts, out_len, count, sc16, peak, None if out is None else out[p], stream, workspace) for p, f in enumerate(frames)]
        pk = self._peak(sc16, peak)
        frames = self._kinds(frames, out, sc16)
        if _is_tensor(frames) != _is_tensor(starts):
            raise TypeError("starts must be %s, as frames is" % ("a torch.int64 CUDA/HIP tensor" if _is_tensor(frames) else "an integer array"))
        n = self._frames(frames)
        out_len = int(out_len)
        L = lib()
        _check(L.gfdm_hip_burst_shaper_check(self.frame_len(), self.pre_padding(), self.post_padding(), pk, n, out_len))
        if _is_tensor(frames):
            import torch
            sptr = _dev_arg(starts, torch.int64, n, "starts", self._dev)
            if count is not None and not _is_tensor(count):
                count = torch.full((1,), int(count), dtype=torch.int64, device=frames.device)
            cptr = None if count is None else _dev_arg(count, torch.int64, 1, "count", self._dev)
            res, optr = self._out(out, out_len, sc16, frames)
            fptr = self._dp(frames, frames.numel(), "frames")
            ws, wptr = self._workspace(workspace, frames, n, out_len, pk)
            if sc16:
                _check(L.gfdm_hip_burst_shaper_place_sc16_device(self._h, optr, out_len, fptr, sptr, cptr, n, pk, wptr, self._sp(stream)))
            else:
                _check(L.gfdm_hip_burst_shaper_place_device(self._h, optr, out_len, fptr, sptr, cptr, n, wptr, self._sp(stream)))
            return res
        st = np.ascontiguousarray(starts, dtype=np.int64).ravel()
        if st.size != n:
            raise RuntimeError("starts has %d elements, expected %d" % (st.size, n))
        cnt = None if count is None else np.array([int(count)], np.int64)
        res, optr = self._out(out, out_len, sc16, frames)
        cptr = None if cnt is None else cnt.ctypes.data
        if sc16:
            _check(L.gfdm_hip_burst_shaper_place_sc16_host(self._h, optr, out_len, frames.ctypes.data, st.ctypes.data, cptr, n, pk))
        else:
            _check(L.gfdm_hip_burst_shaper_place_host(self._h, optr, out_len, frames.ctypes.data, st.ctypes.data, cptr, n))
        return res


class SymbolMapper(_Kernel):
    """Payload bytes <-> constellation symbols, and max-log soft bits (contract in include/gfdm_hip.h, gfdm_hip_symbol_mapper): map() is
    repack_bits_bb(8 -> k, MSB first) + chunks_to_symbols in front of Transmitter.transmit, decode() is constellation_decoder_cb +
    repack_bits_bb(k -> 8) behind demodulate_frames / demodulate_estimated / demodulate_bursts, soft() feeds a decoder instead.  Rows are
    frames or bursts: symbols are (n_rows, n_sym), packed bytes (n_rows, row_bytes(n_sym)), soft bits (n_rows, n_sym * k); a 1-D input is
    one row and gives a 1-D result.  numpy arrays run the host flavour; torch device tensors (uint8 / complex64 / float32) the device
    flavour on the current stream unless given.  count (an int, or on the device path a one-element int64 tensor such as detect's) limits
    the call to the first count rows, the rest is written as zeros; it is clamped to [0, n_rows]."""
    _destroy = "gfdm_hip_symbol_mapper_destroy"

    def __init__(self, points, decision=DECIDE_AUTO, device=0):
        pts = _c64(np.asarray(points).ravel())
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_symbol_mapper_create(ctypes.byref(h), pts.ctypes.data, pts.size, DECIDE.get(decision, decision), device))
        self._h = h
        self._dev = int(device)
        self._k = lib().gfdm_hip_symbol_mapper_bits_per_symbol(h)

    def bits_per_symbol(self):
        return self._k

    def points(self):
        """the points as given to the constructor (complex64, bit for bit)"""
        p = np.empty(lib().gfdm_hip_symbol_mapper_n_points(self._h), np.complex64)
        _check(lib().gfdm_hip_symbol_mapper_points(self._h, p.ctypes.data))
        return p

    def decision_rule(self):
        """'nearest' | 'qpsk' | 'bpsk': the rule decode() runs (gfdm_hip_symbol_mapper_decision)"""
        code = lib().gfdm_hip_symbol_mapper_decision(self._h)
        return {v: k for k, v in DECIDE.items() if k != "auto"}[code]

    def row_bytes(self, n_sym):
        """bytes of a packed row of n_sym symbols: ceil(n_sym * k / 8)"""
        n = lib().gfdm_hip_symbol_mapper_row_bytes(self._h, int(n_sym))
        if n < 0:
            _check(n)
        return n

    def _rows(self, x, dtype, what, width=None):
        """x as rows of `dtype` -> (x, n_rows, width, was 1-D); nothing touches the device"""
        name = np.dtype(dtype).name
        if _is_tensor(x):
            if str(x.dtype).replace("torch.", "") != name or not x.is_cuda or not x.is_contiguous():
                raise TypeError("%s must be a contiguous %s CUDA/HIP tensor" % (what, name))
            if x.device.index != self._dev:
                raise RuntimeError("%s lives on GPU %d, the handle on GPU %d" % (what, x.device.index, self._dev))
        else:
            x = np.asarray(x)
            if dtype == np.uint8 and x.dtype != np.uint8:
                raise TypeError("%s must be uint8 (packed bytes), not %s" % (what, x.dtype))
            if dtype == np.complex64 and not (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.complexfloating)):
                raise TypeError("%s must be complex symbols, not %s" % (what, x.dtype))
            x = np.ascontiguousarray(x, dtype=dtype)
        if x.ndim not in (1, 2):
            raise ValueError("%s must be (n_rows, n) or one row (n,), not %s" % (what, tuple(x.shape)))
        flat = x.ndim == 1
        n_rows, w = (1, x.shape[0]) if flat else (x.shape[0], x.shape[1])
        if width is not None and w != width:
            raise RuntimeError("%s has rows of %d elements, expected %d" % (what, w, width))
        return x, int(n_rows), int(w), flat

    def _result(self, out, like, shape, dtype, flat):
        name = np.dtype(dtype).name
        shape = shape[1:] if flat else shape
        if out is None:
            if _is_tensor(like):
                import torch
                return torch.empty(shape, dtype=getattr(torch, name), device=like.device)
            return np.empty(shape, dtype)
        if _is_tensor(out) != _is_tensor(like) or (not _is_tensor(out) and not isinstance(out, np.ndarray)):
            raise TypeError("out must be a %s, as the input is" % ("CUDA/HIP tensor" if _is_tensor(like) else "numpy array"))
        if str(out.dtype).replace("torch.", "") != name or not (out.is_contiguous() if _is_tensor(out) else out.flags.c_contiguous):
            raise TypeError("out must be contiguous %s" % name)
        if _is_tensor(out) and (not out.is_cuda or out.device.index != self._dev):
            raise RuntimeError("out must live on GPU %d, as the handle does" % self._dev)
        if int(np.prod(out.shape)) != int(np.prod(shape)):
            raise RuntimeError("out holds %d elements, expected %d" % (int(np.prod(out.shape)), int(np.prod(shape))))
        return out

    def _count(self, count, like, keep):
        """pointer of the optional count (None: every row)"""
        if count is None:
            return None
        if _is_tensor(like):
            import torch
            if not _is_tensor(count):
                count = torch.full((1,), int(count), dtype=torch.int64, device=like.device)
            keep.append(count)
            return _dev_arg(count, torch.int64, 1, "count", self._dev)
        if _is_tensor(count):
            raise TypeError("count must be an int on the host path")
        keep.append(np.array([int(count)], np.int64))
        return keep[-1].ctypes.data

    @staticmethod
    def _ptr(a):
        return a.data_ptr() if _is_tensor(a) else a.ctypes.data

    def _run(self, name, res, x, extra, count, n_sym, n_rows, stream):
        keep = []
        cptr = self._count(count, x, keep)
        L = lib()
        _check(L.gfdm_hip_symbol_mapper_check(1 << self._k, n_sym, n_rows))
        if _is_tensor(x):
            _check(getattr(L, name + "_device")(self._h, self._ptr(res), self._ptr(x), *extra, cptr, n_sym, n_rows, self._sp(stream)))
        else:
            _check(getattr(L, name + "_host")(self._h, self._ptr(res), self._ptr(x), *extra, cptr, n_sym, n_rows))
        return res

    def map(self, data, n_sym, count=None, out=None, stream=None):
        """packed bytes (n_rows, row_bytes(n_sym)) uint8 -> symbols (n_rows, n_sym) complex64: points[index], a bit copy"""
        n_sym = int(n_sym)
        data, n_rows, _, flat = self._rows(data, np.uint8, "data", self.row_bytes(n_sym))
        res = self._result(out, data, (n_rows, n_sym), np.complex64, flat)
        return self._run("gfdm_hip_symbol_mapper_map", res, data, (), count, n_sym, n_rows, stream)

    def decode(self, symbols, count=None, out=None, stream=None):
        """symbols (n_rows, n_sym) complex64 -> packed bytes (n_rows, row_bytes(n_sym)) uint8, by the rule of decision_rule()"""
        symbols, n_rows, n_sym, flat = self._rows(symbols, np.complex64, "symbols")
        _check(lib().gfdm_hip_symbol_mapper_check(1 << self._k, n_sym, n_rows))
        res = self._result(out, symbols, (n_rows, self.row_bytes(n_sym)), np.uint8, flat)
        return self._run("gfdm_hip_symbol_mapper_decode", res, symbols, (), count, n_sym, n_rows, stream)

    def soft(self, symbols, scale=None, count=None, out=None, stream=None):
        """symbols (n_rows, n_sym) complex64 -> max-log LLRs (n_rows, n_sym * k) float32, positive for bit 0; scale: float32 (n_rows,), one
        factor per row (typically 1 / sigma^2), a device tensor when symbols is one"""
        symbols, n_rows, n_sym, flat = self._rows(symbols, np.complex64, "symbols")
        _check(lib().gfdm_hip_symbol_mapper_check(1 << self._k, n_sym, n_rows))
        sptr = None
        if scale is not None:
            if _is_tensor(symbols):
                import torch
                if not _is_tensor(scale):
                    raise TypeError("scale must be a float32 CUDA/HIP tensor, as symbols is a tensor")
                sptr = _dev_arg(scale, torch.float32, n_rows, "scale", self._dev)
            else:
                if _is_tensor(scale):
                    raise TypeError("scale must be a host array, as symbols is one")
                scale = np.ascontiguousarray(scale, dtype=np.float32).ravel()
                if scale.size != n_rows:
                    raise RuntimeError("scale has %d elements, expected %d" % (scale.size, n_rows))
                sptr = scale.ctypes.data
        res = self._result(out, symbols, (n_rows, n_sym * self._k), np.float32, flat)
        return self._run("gfdm_hip_symbol_mapper_soft", res, symbols, (sptr,), count, n_sym, n_rows, stream)


def awgn_noise_voltage(signal, snr_db, rate=1.0):
    """ChannelModel's noise_voltage for `snr_db` on `signal`: sqrt(2 * v), v pygfdm's calculate_awgn_noise_variance (python/pygfdm/utils.py:
    106-110, the variance PER COMPONENT: average sample energy / (2 * rate * 10^(snr_db / 10))) -- the noise power of the channel model is
    noise_voltage^2 = 2 v.  `signal` is a numpy array or a torch tensor; the energy of a tensor is summed on its device."""
    if _is_tensor(signal):
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


class ChannelModel(_Kernel):
    """Multipath, frequency offset and noise on a stream, on the device (contract in include/gfdm_hip.h, gfdm_hip_channel_model): GNU
    Radio's channels.channel_model in its argument order, between BurstShaper.place and BurstSync.detect.  y = FIR(taps) of x, times
    exp(j 2 pi frequency_offset n), plus white Gaussian noise of power noise_voltage^2 that is a pure function of (noise_seed, absolute
    sample index).  epsilon (the timing offset) must be 1.0: resampling is not part of this.  The taps are fixed; frequency_offset,
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

    _kinds = staticmethod(BurstShaper._kinds)
    _out = BurstShaper._out

    def apply(self, x, history=0, offset=0, sc16=False, gain=1.0, out=None, stream=None):
        """x holds history + n samples, the result has n: sample i of the result is the channel's output for x[history + i], whose absolute
        index is offset + i; the first `history` samples are the FIR's past (GNU Radio's history; what lies before them is zeros).  A stream
        cut into calls gives the samples of one call when each piece passes history = min(n_taps - 1, samples before it) and its offset.
        numpy x -> numpy result (host path); a torch complex64 device tensor -> a tensor on its device (device path, current stream unless
        given).  sc16=True writes int16 I/Q of shape (n, 2), truncated and saturated, of y * gain."""
        if not sc16 and float(gain) != 1.0:
            raise ValueError("gain scales sc16 output: pass sc16=True (complex64 output is not scaled)")
        x = self._kinds(x, out, sc16, "x")
        history, offset = int(history), int(offset)
        size = x.numel() if _is_tensor(x) else x.size
        if history < 0 or history > size:
            raise ValueError("history(%d) must lie in 0 .. the size of x(%d)" % (history, size))
        n = size - history
        res, optr = self._out(out, n, sc16, x)
        L = lib()
        if _is_tensor(x):
            xptr = self._dp(x, size, "x") + 8 * history
            if sc16:
                _check(L.gfdm_hip_channel_model_apply_sc16_device(self._h, optr, xptr, n, history, offset, float(gain), self._sp(stream)))
            else:
                _check(L.gfdm_hip_channel_model_apply_device(self._h, optr, xptr, n, history, offset, self._sp(stream)))
            return res
        xptr = x.ctypes.data + 8 * history
        if sc16:
            _check(L.gfdm_hip_channel_model_apply_sc16_host(self._h, optr, xptr, n, history, offset, float(gain)))
        else:
            _check(L.gfdm_hip_channel_model_apply_host(self._h, optr, xptr, n, history, offset))
        return res


class LinkMeter(_Kernel):
    """Closing the loop on the device (contract in include/gfdm_hip.h, gfdm_hip_link_meter): match() pairs BurstSync.detect's detections
    with the bursts that were sent, measure() counts bit / symbol / row errors of demodulated rows against the sent payload with the
    decisions SymbolMapper.decode makes and gives every row's error-vector power (data-aided: the EVM; without a payload: the
    decision-directed noise estimate SymbolMapper.soft's scale asks for), and every call adds to twelve counters that stay on the device
    until totals() reads them -- the one read of a curve point.  Constructor arguments as SymbolMapper's.  numpy arrays run the host
    flavour; torch device tensors the device flavour on the current stream unless given.  count is an int or (device path) detect's
    one-element int64 tensor.  out: a dict with any of the result's keys, to write into existing arrays; workspace: a uint8 device
    tensor of match_workspace_bytes() / measure_workspace_bytes() to use instead of a new one."""
    _destroy = "gfdm_hip_link_meter_destroy"
    FIELDS = ("rows", "symbols", "bits", "bit_errors", "symbol_errors", "row_errors", "detections", "matched", "missed", "false_alarms")

    def __init__(self, points, decision=DECIDE_AUTO, device=0):
        pts = _c64(np.asarray(points).ravel())
        h = ctypes.c_void_p()
        _check(lib().gfdm_hip_link_meter_create(ctypes.byref(h), pts.ctypes.data, pts.size, DECIDE.get(decision, decision), device))
        self._h = h
        self._dev = int(device)
        self._k = lib().gfdm_hip_link_meter_bits_per_symbol(h)

    def bits_per_symbol(self):
        return self._k

    def decision_rule(self):
        """'nearest' | 'qpsk' | 'bpsk': the rule measure() decides by (SymbolMapper.decode's for the same points)"""
        code = lib().gfdm_hip_link_meter_decision(self._h)
        return {v: k for k, v in DECIDE.items() if k != "auto"}[code]

    def row_bytes(self, n_sym):
        n = lib().gfdm_hip_link_meter_row_bytes(self._h, int(n_sym))
        if n < 0:
            _check(n)
        return n

    @staticmethod
    def match_workspace_bytes(n_sent):
        n = lib().gfdm_hip_link_meter_match_workspace_bytes(int(n_sent))
        if n < 0:
            _check(n)
        return n

    @staticmethod
    def measure_workspace_bytes(n_sym, n_rows):
        n = lib().gfdm_hip_link_meter_measure_workspace_bytes(int(n_sym), int(n_rows))
        if n < 0:
            _check(n)
        return n

    _rows = SymbolMapper._rows
    _count = SymbolMapper._count
    _ptr = staticmethod(SymbolMapper._ptr)

    def _vector(self, x, dtype, n, what, like):
        """an input of n elements of `dtype`, of `like`'s kind (device tensor or host array)"""
        name = np.dtype(dtype).name
        if _is_tensor(like):
            import torch
            if not _is_tensor(x):
                raise TypeError("%s must be a torch.%s CUDA/HIP tensor, as the other arrays are" % (what, name))
            _dev_arg(x, getattr(torch, name), n, what, self._dev)
            return x
        if _is_tensor(x):
            raise TypeError("%s must be a host array, as the other arrays are" % what)
        x = np.ascontiguousarray(x, dtype=dtype).ravel()
        if x.size != n:
            raise RuntimeError("%s has %d elements, expected %d" % (what, x.size, n))
        return x

    def _result(self, out, key, like, n, dtype):
        """the output `key` of n elements: out[key] where given, else a new array of `like`'s kind"""
        name = np.dtype(dtype).name
        res = None if out is None else out.get(key)
        if res is None:
            if _is_tensor(like):
                import torch
                return torch.empty((n,), dtype=getattr(torch, name), device=like.device)
            return np.empty((n,), dtype)
        if _is_tensor(res) != _is_tensor(like) or (not _is_tensor(res) and not isinstance(res, np.ndarray)):
            raise TypeError("out[%r] must be a %s, as the input is" % (key, "CUDA/HIP tensor" if _is_tensor(like) else "numpy array"))
        if str(res.dtype).replace("torch.", "") != name or not (res.is_contiguous() if _is_tensor(res) else res.flags.c_contiguous):
            raise TypeError("out[%r] must be contiguous %s" % (key, name))
        if _is_tensor(res) and (not res.is_cuda or res.device.index != self._dev):
            raise RuntimeError("out[%r] must live on GPU %d, as the handle does" % (key, self._dev))
        if int(np.prod(res.shape)) != n:
            raise RuntimeError("out[%r] holds %d elements, expected %d" % (key, int(np.prod(res.shape)), n))
        return res

    def _workspace(self, ws, like, need):
        import torch
        if ws is None:
            return torch.empty(need, dtype=torch.uint8, device=like.device)
        if not _is_tensor(ws) or ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous() or ws.numel() < need or ws.device.index != self._dev:
            raise TypeError("workspace must be a contiguous uint8 CUDA/HIP tensor of at least %d bytes on GPU %d" % (need, self._dev))
        return ws

    def _settle(self):
        """the host flavours run on the handle's own stream: what torch's current stream still holds for this handle (a reset) goes first"""
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
        if not _is_tensor(frame_start):
            frame_start = np.ascontiguousarray(frame_start, dtype=np.int64).ravel()
        n_rows = int(frame_start.numel() if _is_tensor(frame_start) else frame_start.size)
        frame_start = self._vector(frame_start, np.int64, n_rows, "frame_start", frame_start)
        n_sent = int(sent_pos.numel() if _is_tensor(sent_pos) else np.asarray(sent_pos).size)
        sent_pos = self._vector(sent_pos, np.int64, n_sent, "sent_pos", frame_start)
        tol, offset = int(tol), int(offset)
        res = {"ref_row": self._result(out, "ref_row", frame_start, n_rows, np.int64), "sent_row": self._result(out, "sent_row", frame_start, n_sent, np.int64)}
        keep = []
        cptr = self._count(count, frame_start, keep)
        L = lib()
        if _is_tensor(frame_start):
            ws = self._workspace(workspace, frame_start, self.match_workspace_bytes(n_sent))
            _check(L.gfdm_hip_link_meter_match_device(self._h, self._ptr(res["ref_row"]), self._ptr(res["sent_row"]), self._ptr(frame_start), cptr, n_rows,
                                                      self._ptr(sent_pos), n_sent, offset, tol, ws.data_ptr(), self._sp(stream)))
        else:
            self._settle()
            _check(L.gfdm_hip_link_meter_match_host(self._h, self._ptr(res["ref_row"]), self._ptr(res["sent_row"]), self._ptr(frame_start), cptr, n_rows,
                                                    self._ptr(sent_pos), n_sent, offset, tol))
        return res

    def measure(self, symbols, payload=None, ref_row=None, count=None, out=None, stream=None, workspace=None):
        """symbols (n_rows, n_sym) complex64 against payload (n_ref, row_bytes(n_sym)) uint8 -> {"bit_errors": int32, "err_power": float32,
        "ref_power": float32}, each (n_rows,); row r is compared with payload row ref_row[r] (None: r), a row whose ref_row is negative or
        beyond the payload gives -1 / 0 / 0 and is not read.  payload None: decision-directed, err_power against the decided points, no
        bit_errors."""
        symbols, n_rows, n_sym, _ = self._rows(symbols, np.complex64, "symbols")
        n_ref = 0
        if payload is not None:
            if _is_tensor(payload) != _is_tensor(symbols):
                raise TypeError("payload must be a %s, as symbols is" % ("CUDA/HIP tensor" if _is_tensor(symbols) else "numpy array"))
            payload, n_ref, _, _ = self._rows(payload, np.uint8, "payload", self.row_bytes(n_sym))
        if ref_row is not None:
            ref_row = self._vector(ref_row, np.int64, n_rows, "ref_row", symbols)
        res = {}
        if payload is not None:
            res["bit_errors"] = self._result(out, "bit_errors", symbols, n_rows, np.int32)
        elif out is not None and out.get("bit_errors") is not None:
            raise ValueError("bit_errors needs a payload: a decision-directed call counts no errors")
        res["err_power"] = self._result(out, "err_power", symbols, n_rows, np.float32)
        res["ref_power"] = self._result(out, "ref_power", symbols, n_rows, np.float32)
        keep = []
        cptr = self._count(count, symbols, keep)
        ptr = lambda a: None if a is None else self._ptr(a)
        L = lib()
        if _is_tensor(symbols):
            if payload is not None and n_ref == 0:                           # an empty tensor has no pointer, and NULL would mean decision-directed
                import torch
                payload = torch.empty(16, dtype=torch.uint8, device=symbols.device)
            ws = self._workspace(workspace, symbols, self.measure_workspace_bytes(n_sym, n_rows))
            _check(L.gfdm_hip_link_meter_measure_device(self._h, ptr(res.get("bit_errors")), ptr(res["err_power"]), ptr(res["ref_power"]), self._ptr(symbols),
                                                        ptr(payload), n_ref, ptr(ref_row), cptr, n_sym, n_rows, ws.data_ptr(), self._sp(stream)))
        else:
            self._settle()
            _check(L.gfdm_hip_link_meter_measure_host(self._h, ptr(res.get("bit_errors")), ptr(res["err_power"]), ptr(res["ref_power"]), self._ptr(symbols),
                                                      ptr(payload), n_ref, ptr(ref_row), cptr, n_sym, n_rows))
        return res
