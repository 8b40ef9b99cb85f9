// The burst extractor's sample fetch (extract_burst_cc, contract in include/gfdm_hip.h): ONE definition for k_extract (gfdm_burst.hip)
// and for the receivers that read their bursts straight from the capture (the gather-load stage of k_row_receive and
// k_generic_receive), so that the two cannot drift.  Compiles under hipcc and under hiprtc (gfdm_jit.hip embeds it).
#pragma once
#include "gfdm_dft.h"
#include "gfdm_plan.h"

namespace gfdm {

// Sample format of a capture, uniform over a launch.  SAMPLES_SC16: interleaved int16 I, Q (UHD's sc16); sample i is (float)I_i + j (float)Q_i,
// unscaled.  int16 -> fp32 is exact and nothing behind the load depends on the format, so every result is bit-equal to that of the same
// values given as complex64.  An sc16 sample is 4-byte aligned and no more: it is one 4-byte access, never half of an 8-byte one.
typedef short sc16_io __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf sc16_to_cf(sc16_io v) { return make_float2((float)v.x, (float)v.y); }

// the capture from its sample i on
__device__ __forceinline__ const void* capture_at(const void* s, int64_t i, int fmt)
{
    return fmt == SAMPLES_SC16 ? (const void*)(static_cast<const sc16_io*>(s) + i) : (const void*)(static_cast<const cf*>(s) + i);
}

// sample i of a capture, plain load (the synchroniser's reads: every sample is read by several workgroups)
__device__ __forceinline__ cf capture_load(const void* __restrict__ s, int64_t i, int fmt)
{
    if (fmt == SAMPLES_SC16) return sc16_to_cf(static_cast<const sc16_io*>(s)[i]);
    return static_cast<const cf*>(s)[i];
}

// phase step of conj(r) / |r|, i.e. -angle(r), in fp64.  The caller has set rotate = 0 and phi = 0: they stay so for r == 0, and that burst
// is not rotated.
__device__ __forceinline__ void burst_phase_step(cf r, int& rotate, double& phi)
{
    if (r.x != 0.f || r.y != 0.f) {
        rotate = 1;
        phi = -atan2((double)r.y, (double)r.x);
    }
}

// g * s[base + n] * exp(j phi n): zero outside [0, stream_len), the phase phi * n reduced mod 2 pi in fp64 (within 2e-5 of a float64
// rotation for any n).  n counts from the burst start, base = off_b - backoff.  fmt: SampleFormat of s.
__device__ __forceinline__ cf burst_fetch(const void* __restrict__ s, int fmt, int64_t stream_len, int64_t base, int n, float g, int rotate, double phi)
{
    constexpr double kPi = 3.14159265358979323846;
    const int64_t i = base + n;
    cf x = make_float2(0.f, 0.f);
    if (i >= 0 && i < stream_len) {
        if (fmt == SAMPLES_SC16) x = sc16_to_cf(__builtin_nontemporal_load(static_cast<const sc16_io*>(s) + i));
        else x = dft::ld_stream(static_cast<const cf*>(s) + i);
    }
    x = make_float2(x.x * g, x.y * g);
    if (rotate) {
        double ph = phi * (double)n;
        ph -= 2.0 * kPi * rint(ph * (0.5 / kPi));
        float sn, cs;
        sincosf((float)ph, &sn, &cs);
        x = make_float2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
    }
    return x;
}

}  // namespace gfdm
