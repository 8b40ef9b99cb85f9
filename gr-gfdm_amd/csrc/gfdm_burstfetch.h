// The burst extractor's sample fetch (extract_burst_cc, contract in include/gfdm_hip.h): ONE definition for k_extract (gfdm_burst.hip)
// and for the receivers that read their bursts straight from the capture (the gather-load stage of k_row_receive and
// k_generic_receive), so that the two cannot drift.  Compiles under hipcc and under hiprtc (gfdm_jit.hip embeds it).
#pragma once
#include "gfdm_dft.h"
#include "gfdm_plan.h"

namespace gfdm {

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
// rotation for any n).  n counts from the burst start, base = off_b - backoff.
__device__ __forceinline__ cf burst_fetch(const cf* __restrict__ s, int64_t stream_len, int64_t base, int n, float g, int rotate, double phi)
{
    constexpr double kPi = 3.14159265358979323846;
    const int64_t i = base + n;
    cf x = (i >= 0 && i < stream_len) ? dft::ld_stream(s + i) : make_float2(0.f, 0.f);
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
