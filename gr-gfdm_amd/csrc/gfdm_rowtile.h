// Internal: the output-tile skeleton of the row stages -- k_symbols_map, k_symbols_soft, k_cc_encode, k_rm_match, k_rm_unmatch -- ONE
// definition of what they share ("Row stages").  Never seen by hiprtc (not in JIT_HDRS).
// A row stage writes rows of `width` elements that lie back to back, so it tiles the flat OUTPUT with the StreamTiles of gfdm_streamtile.h:
// aligned vectors of 16 bytes (4 for k_rm_match), tile_vec of them per workgroup, the tiles beyond the grid strided over.  Per tile ONE
// 64-bit division gives the (row, index) of the first element (RowCursor); a lane reaches its own with at(d), steps on with next(), and its
// vector leaves in one aligned store, element by element at the two ends of an unaligned output (store_elems).  The kernels and the enqueue
// functions build the same StreamTiles (row_grid): the grid is the kernel's own tile count.  tests/sanitize/rowtile_check.cc brute-forces
// the host half -- geometry, grid and cursor.
#pragma once
#include "gfdm_streamtile.h"

namespace gfdm {

// (row, index in the row) of the flat element d behind the one at (r0, i0); rows of n elements, i0 < n.  No 64-bit division: past the
// first row what is left of d is below 2^32, and so is n where a quotient is needed at all.
struct RowPos { int64_t r, i; };
__host__ __device__ __forceinline__ RowPos advance(int64_t r0, int64_t i0, uint32_t d, int64_t n)
{
    RowPos p = { r0, i0 + (int64_t)d };
    if (p.i >= n) {
        p.i -= n;
        ++p.r;
        if (p.i >= n) {
            const uint32_t q = (uint32_t)p.i / (uint32_t)n;
            p.r += q;
            p.i -= (int64_t)q * n;
        }
    }
    return p;
}

// the largest d a stage hands to at(): each states its own as a static_assert against this, which is as far as rowtile_check.cc walks
constexpr int kMaxRowReach = 4095;

// where the flat element i_lo (a tile's first) lies in rows of `width` elements, and the way on from there: at(d) is the element d behind
struct RowCursor : RowPos {
    int64_t width;
    __host__ __device__ __forceinline__ RowCursor(RowPos p, int64_t width_) : RowPos(p), width(width_) {}
    __host__ __device__ __forceinline__ RowCursor(int64_t i_lo, int64_t width_) : RowPos{ i_lo / width_, i_lo }, width(width_) { i -= r * width_; }
    __host__ __device__ __forceinline__ RowCursor at(uint32_t d) const { return RowCursor(advance(r, i, d, width), width); }
    __host__ __device__ __forceinline__ void next()
    {
        if (++i == width) {
            i = 0;
            ++r;
        }
    }
};

// the workgroups of a launch: the kernel's own tile count, at least one, at most cap
inline unsigned row_grid(const void* out, int vps, int64_t total, int tile_vec, int cap, int vec_bytes = 16)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(StreamTiles(out, vps, total, tile_vec, vec_bytes).ntiles, cap));
}

#ifdef __HIPCC__
// Step 3: the V elements of the vector whose first element is i0, packed in 32-bit words as they lie in memory (V sizeof(T) = 16 or 4 bytes)
template <typename T, int V>
__device__ __forceinline__ void store_elems(T* out, const StreamTiles& tl, int64_t i0, const uint32_t (&w)[V * sizeof(T) / 4])
{
    constexpr int W = V * sizeof(T) / 4;
    static_assert((W == 4 || W == 1) && (sizeof(T) == 1 || sizeof(T) == 4 || sizeof(T) == 8), "a vector of 16 or 4 bytes");
    if (tl.whole(i0)) {                              // aligned by construction
        if constexpr (W == 4) *reinterpret_cast<uint4*>(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        else *reinterpret_cast<uint32_t*>(out + i0) = w[0];
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {                // head or tail of the output
            const int64_t i = i0 + e;
            if (i < 0 || i >= tl.n) continue;
            if constexpr (sizeof(T) == 1) *reinterpret_cast<unsigned char*>(out + i) = (unsigned char)(w[e >> 2] >> (8 * (e & 3)));
            else if constexpr (sizeof(T) == 4) *reinterpret_cast<uint32_t*>(out + i) = w[e];
            else *reinterpret_cast<uint2*>(out + i) = make_uint2(w[2 * e], w[2 * e + 1]);
        }
    }
}

// Steps 2 and 3 of a stage whose elements do not depend on each other, for the vector v of tile t: element(r, i) is element i of the live
// row r as its bits; the rows from n_live on and the words' spare bits are 0
template <typename T, int V, typename F>
__device__ __forceinline__ void write_elems(T* out, const StreamTiles& tl, const TileSpan& t, const RowCursor& first, int64_t v, int64_t n_live, F element)
{
    const int64_t i0 = tl.first(v);
    RowCursor pos = first.at((uint32_t)(std::max(i0, (int64_t)0) - t.i_lo));
    uint32_t w[V * sizeof(T) / 4] = {};
#pragma unroll
    for (int e = 0; e < V; ++e) {
        if (i0 + e < 0 || i0 + e >= tl.n) continue;
        if (sizeof(T) == 4 && pos.r < n_live) w[e] = element(pos.r, pos.i);        // (not |=: a load's value is not needed before the store)
        if (sizeof(T) == 1 && pos.r < n_live) w[e / 4] |= (uint32_t)element(pos.r, pos.i) << (8 * (e % 4));
        pos.next();
    }
    store_elems<T, V>(out, tl, i0, w);
}
#endif

}  // namespace gfdm
