// The sc16 output rule (include/gfdm_hip.h: "q truncates toward zero and saturates to [-32768, 32767], NaN gives 0"): ONE definition for
// every kernel that writes interleaved int16 I/Q -- the burst shaper (gfdm_shaper.hip), the channel model (gfdm_channel.hip) and the fading
// model (gfdm_fading.hip), all three through the stores of gfdm_streamtile.h.
#pragma once
#include "gfdm_plan.h"

namespace gfdm {

// truncation toward zero, saturated to int16; NaN gives 0
__device__ __forceinline__ int q16(float v)
{
    if (v != v) return 0;
    return (int)fminf(fmaxf(v, -32768.f), 32767.f);
}

// one sample: q(y.re * g) in the low half, q(y.im * g) in the high half, the products in fp32
__device__ __forceinline__ unsigned pack_sc16(cf y, float g)
{
    return ((unsigned)q16(y.x * g) & 0xFFFFu) | ((unsigned)q16(y.y * g) << 16);
}

}  // namespace gfdm
