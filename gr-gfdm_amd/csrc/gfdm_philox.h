// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator behind the
// channel model's noise (gfdm_channel.hip; the contract in include/gfdm_hip.h names the constants).  Plain integer code that compiles
// for the device and for the host alike, so that the known answers of the paper's reference implementation can be checked without a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFDM_PHILOX_FN __host__ __device__ __forceinline__
#else
#define GFDM_PHILOX_FN inline
#endif

namespace gfdm {

struct Philox4 {
    uint32_t v[4];
};

// ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1); the key is bumped by the Weyl constants between rounds
GFDM_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kW0;
        k1 += kW1;
    }
    return Philox4{ { c0, c1, c2, c3 } };
}

}  // namespace gfdm
