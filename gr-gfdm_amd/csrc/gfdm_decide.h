// Internal, device side: the hard decision of one symbol pair and what goes with it, shared by the symbol mapper (gfdm_symbols.hip:
// decode) and the link meter (gfdm_linkmeter.hip: measure) -- one device function, so that an error counted by the meter is an error in
// the bytes decode writes, to the bit.  The contract is written out in include/gfdm_hip.h (gfdm_hip_symbol_mapper, decode).  live_rows is
// the clamp of the optional `count` operand, for those two, the convolutional code and the burst shaper.
#pragma once
#include "../../include/gfdm_hip.h"
#include "gfdm_plan.h"

#include <algorithm>

namespace gfdm {

// the rows (bursts) of a call that are live: all of them, or the optional device-side count clamped to [0, n_rows]
__host__ __device__ __forceinline__ int64_t live_rows(const int64_t* count, int64_t n_rows)
{
    if (!count) return n_rows;
    return std::min(std::max(*count, (int64_t)0), n_rows);
}

// squared distance in the direct form: the contract's d_i
__device__ __forceinline__ float dist2(cf x, cf p)
{
    const float dr = x.x - p.x, di = x.y - p.y;
    return dr * dr + di * di;
}

// RULE: a gfdm_hip_decision (never AUTO).  NEAREST: the first strict minimum starting from +inf (decide_point of gfdm_rowlane_impl.h), so
// NaN and infinite inputs give index 0; the sign tests are '> 0', so NaN gives 0 and an infinite component decides by its sign.
template <int K, int RULE>
__device__ __forceinline__ void decide2(cf x0, cf x1, const cf* pts, int& i0, int& i1)
{
    if constexpr (RULE == GFDM_HIP_DECIDE_QPSK) {
        i0 = 2 * (x0.y > 0.f) + (x0.x > 0.f);
        i1 = 2 * (x1.y > 0.f) + (x1.x > 0.f);
    } else if constexpr (RULE == GFDM_HIP_DECIDE_BPSK) {
        i0 = (x0.x > 0.f);
        i1 = (x1.x > 0.f);
    } else {
        float b0 = __builtin_huge_valf(), b1 = __builtin_huge_valf();
        i0 = i1 = 0;
#pragma unroll 16
        for (int i = 0; i < (1 << K); ++i) {
            const cf p = pts[i];                    // the same LDS address in every lane: a broadcast
            const float d0 = dist2(x0, p), d1 = dist2(x1, p);
            if (d0 < b0) { b0 = d0; i0 = i; }
            if (d1 < b1) { b1 = d1; i1 = i; }
        }
    }
}

}  // namespace gfdm
