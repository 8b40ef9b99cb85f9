"""gfdm_amd: MI355X-native GFDM modulator / receiver / IC-receiver kernels (host-side Python mirror).

`Modulator`, `Demodulator`, `AdvancedReceiver`, `AmplifierModel`, `BurstSync`, `BurstExtractor`, `BurstShaper`, `ChannelModel`, `FadingModel`, `Resampler`, `SymbolMapper`, `LinkMeter`, `SpectrumMeter`, `ConvolutionalCode`, `RateMatcher`, `FrameCheck` and the other handles forward to the C-ABI of include/gfdm_hip.h
(libgfdm_hip.so).  `filters` generates prototype-filter taps; `to_sc16` / `from_sc16` convert captures between complex and int16 I/Q on the host
(the burst calls read either format).  No signal processing runs on the CPU.
"""
from . import filters  # noqa: F401
from .capi import (AdvancedReceiver, AmplifierModel, BurstExtractor, BurstShaper, BurstSync, ChannelEstimator, ChannelModel, ConvolutionalCode, CyclicPrefixer, Demodulator, FadingModel, FrameCheck, GfdmHipError, LinkMeter, Modulator, RateMatcher, Resampler, ResourceMapper, SpectrumMeter, SymbolMapper, Transmitter, exported_symbols,  # noqa: F401
                   JIT_AUTO, JIT_BACKGROUND, JIT_IN_CONSTRUCTOR, JIT_OFF, generic_family_for_testing, lib, precompile, quiesce, set_dft_matrix_cores, set_ic_matrix_cores, set_jit, set_wide_access,
                   HOST_COPY_ENGINES, HOST_ZERO_COPY, aligned_copy, aligned_empty, build_id, get_host_pipeline, host_call_stats, register_host, registered_host, set_host_pipeline, threshold_factor, unregister_host,
                   CC_TERMINATED, CC_TRUNCATED, DECIDE_AUTO, DECIDE_BPSK, DECIDE_NEAREST, DECIDE_QPSK, amplifier_curve, amplifier_drive, awgn_noise_voltage, block_interleaver, fading_sinusoids, fading_taps, from_sc16, puncture_pattern, oob_ratio_db, resampler_step, resampler_taps, spectrum_window, subcarrier_power, to_sc16)
