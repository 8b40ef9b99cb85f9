// Internal: the tile skeleton of the stream stages -- k_shaper_place, k_channel, k_resample, k_fade, k_amplify -- ONE definition of what they
// share, so that the five cannot drift ("Stream stages").  Never seen by hiprtc (not in JIT_HDRS).
//
// A stage tiles its OUTPUT: the stream is cut into 16-byte vectors aligned in memory (VPS = 2 complex64 or 4 sc16 samples), a workgroup takes
// tile_vec of them and strides over the tiles beyond the grid.  Per tile
//   1. (stage_in) the complex64 input samples [first, end) that the tile needs -- the tile and its halo -- go to LDS once, in 16-byte loads
//      aligned in memory, sample by sample where history, n or the alignment of `in` cuts a vector, zeros outside [-history, n);
//   2. the stage's own work;
//   3. (store_tile, store_vector) the tile leaves in 16-byte stores aligned in memory; the first and last samples of an unaligned stream go
//      out one by one.
// The first half is plain C++ for the host and the device alike: the geometry (the kernels and the enqueue functions use the same
// StreamTiles, so the grid is the kernel's own tile count) and the bounds that size the LDS arrays and the lanes' shares, which the stages
// state as static_asserts.  tests/sanitize/streamtile_check.cc brute-forces both.  The second half is device code.
#pragma once
#include "gfdm_plan.h"

#include <stdint.h>
#include <algorithm>
#include <type_traits>

namespace gfdm {

// one tile: the vectors [v0, v1), the samples [i_lo, i_hi) of the stream that lie in them; s0 is the sample at the first lane of vector v0
// (below 0 in the first tile of an unaligned stream)
struct TileSpan {
    int64_t v0, v1, s0, i_lo, i_hi;
};

// the tiles of a stream of n samples at `out`: vps samples per 16-byte vector (vec_bytes: the row stages of gfdm_rowtile.h have one of 4
// bytes), tile_vec vectors per tile (a constant folds).  For n >= 1 every tile holds a sample; the enqueue functions return before a
// launch with n = 0 (an unaligned `out` would give one empty tile)
struct StreamTiles {
    int vps, tile_vec;
    int mis;                 // samples between the vector boundary in front of `out` and `out`
    int64_t n, nvec, ntiles;

    __host__ __device__ __forceinline__ StreamTiles(const void* out, int vps_, int64_t n_, int tile_vec_, int vec_bytes = 16)
        : vps(vps_), tile_vec(tile_vec_), mis((int)(((uintptr_t)out / (vec_bytes / vps_)) % vps_)), n(n_), nvec((n_ + mis + vps_ - 1) / vps_),
          ntiles((nvec + tile_vec_ - 1) / tile_vec_)
    {
    }
    __host__ __device__ __forceinline__ TileSpan tile(int64_t t) const
    {
        TileSpan s;
        s.v0 = t * tile_vec;
        s.v1 = std::min(s.v0 + tile_vec, nvec);
        s.s0 = s.v0 * vps - mis;
        s.i_lo = std::max(s.s0, (int64_t)0);
        s.i_hi = std::min(s.v1 * vps - mis, n);
        return s;
    }
    // the sample at the first lane of vector v
    __host__ __device__ __forceinline__ int64_t first(int64_t v) const { return v * vps - mis; }
    // the vector whose first sample is i lies in the stream as a whole: one 16-byte store, aligned by construction
    __host__ __device__ __forceinline__ bool whole(int64_t i) const { return i >= 0 && i + vps <= n; }
};

// Step 1 starts at the sample at or one in front of g0 that sits on a 16-byte boundary of the complex64 input
__host__ __device__ __forceinline__ int64_t stage_first(const void* in, int64_t g0)
{
    return g0 - ((g0 + (int64_t)(((uintptr_t)in / 8) & 1)) & 1);
}

// the largest end - stage_first(in, i_lo - lower) for end = i_hi + upper: a tile of `tile` samples, `lower` samples in front of it, `upper`
// behind it, and in_align - 1 more for the alignment of the first load.  stage_in stores pairs: the LDS array has an even size >= this.
constexpr int max_stage(int tile, int lower, int upper, int in_align) { return tile + lower + upper + in_align - 1; }

// the largest number of aligned groups of g absolute indices that `tile` consecutive ones can meet, wherever they begin (offset and the
// alignment of `out` move the beginning): the first index may be the last of its group
constexpr int max_groups(int tile, int g) { return tile < 2 ? tile : (tile - 2) / g + 2; }

}  // namespace gfdm

#ifdef __HIPCC__
#include "gfdm_sc16out.h"

namespace gfdm {

// what a sample is in the output: complex64, or the packed int16 pair of pack_sc16
template <int SC16> using stored_t = typename std::conditional<SC16 != 0, unsigned, cf>::type;

template <int SC16>
__device__ __forceinline__ stored_t<SC16> to_stored(cf y, float gain)
{
    if constexpr (SC16) return pack_sc16(y, gain);
    else return y;
}

// where sample k of the staged span lies in LDS: PAD = 0 plain, else one padding sample per 2^PAD (k and k + 1 of an even k are neighbours)
template <int PAD>
__device__ __forceinline__ int staged_at(int k)
{
    return PAD ? k + (k >> PAD) : k;
}

// Step 1: xs[staged_at<PAD>(k)] = x[j0 + k] for k < nstage (and the one behind an odd nstage), zero outside [-history, n); j0 =
// stage_first(in, ...).  The plain layout is written with one 16-byte LDS store per pair, the padded one with two of 8 bytes.
template <int PAD>
__device__ __forceinline__ void stage_in(cf* xs, const cf* in, int64_t j0, int nstage, int64_t history, int64_t n, int lanes)
{
    for (int k = 2 * threadIdx.x; k < nstage; k += 2 * lanes) {
        const int64_t j = j0 + k;
        float4 x2;
        if (j >= -history && j + 1 < n) {
            x2 = *reinterpret_cast<const float4*>(in + j);
        } else {
            const cf xa = (j >= -history && j < n) ? in[j] : make_float2(0.f, 0.f);
            const cf xb = (j + 1 >= -history && j + 1 < n) ? in[j + 1] : make_float2(0.f, 0.f);
            x2 = make_float4(xa.x, xa.y, xb.x, xb.y);
        }
        if constexpr (PAD == 0) {
            *reinterpret_cast<float4*>(xs + k) = x2;
        } else {
            const int at = staged_at<PAD>(k);
            xs[at] = make_float2(x2.x, x2.y);
            xs[at + 1] = make_float2(x2.z, x2.w);
        }
    }
}

// Step 3 from registers: the VPS samples y of the vector whose first sample is i0, times g in sc16
template <int SC16>
__device__ __forceinline__ void store_vector(unsigned char* base, const StreamTiles& tl, int64_t i0, const cf* y, float g)
{
    constexpr int VPS = SC16 ? 4 : 2, SB = 16 / VPS;
    if (tl.whole(i0)) {
        if constexpr (SC16) *reinterpret_cast<uint4*>(base + i0 * SB) = make_uint4(pack_sc16(y[0], g), pack_sc16(y[1], g), pack_sc16(y[2], g), pack_sc16(y[3], g));
        else *reinterpret_cast<float4*>(base + i0 * SB) = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
        return;
    }
#pragma unroll
    for (int j = 0; j < VPS; ++j) {                  // head or tail of the stream
        const int64_t i = i0 + j;
        if (i >= 0 && i < tl.n) *reinterpret_cast<stored_t<SC16>*>(base + i * SB) = to_stored<SC16>(y[j], g);
    }
}

// Step 3 from LDS: ys[k] is sample t.s0 + k of the stream, in output format
template <int SC16>
__device__ __forceinline__ void store_tile(unsigned char* base, const StreamTiles& tl, const TileSpan& t, const stored_t<SC16>* ys, int lanes)
{
    constexpr int VPS = SC16 ? 4 : 2, SB = 16 / VPS;
    for (int64_t v = t.v0 + threadIdx.x; v < t.v1; v += lanes) {
        const int64_t i = tl.first(v);
        const int k = (int)(i - t.s0);
        if (tl.whole(i)) {
            *reinterpret_cast<uint4*>(base + i * SB) = *reinterpret_cast<const uint4*>(ys + k);
        } else {
            for (int e = 0; e < VPS; ++e)
                if (i + e >= 0 && i + e < tl.n) *reinterpret_cast<stored_t<SC16>*>(base + (i + e) * SB) = ys[k + e];
        }
    }
}

}  // namespace gfdm
#endif
