// Per-lane tables of the row-lane kernels in the pair-packed form (host side only, plain C++: no HIP header, so that it is compiled and
// tested without a GPU -- tests/test_packed_tables.py).
//
// A per-lane table holds n entries for each of the K lanes of a block.  As planes [n][K] a lane fetches its entries with n 8-byte loads.
// Pair-packed, entries 2 j and 2 j + 1 of a lane lie side by side -- [n / 2][K][2], then one plane [K] for the last entry of an odd n --
// and the lane fetches them with n / 2 16-byte loads (+ one 8-byte load): the same values, the same bits, and a wave instruction still
// reads one contiguous segment (16 K bytes instead of 8 K).  Every plane starts on a 16-byte boundary when the table does: a pair plane
// is 16 K bytes long, and the tables are padded to an even number of elements.
//   twiddles  entry i of lane q = twT[(i + 1) K + q] = W_N^{q (i + 1)}, i < M - 1 (plane 0 of [m][K] is all ones and never read)
//   roots     entry i of lane q = wK[rowgeom::root_index(K, q, i)], i < rowgeom::root_count(K): the subcarrier-FFT roots in the order the
//             kernel consumes them
#pragma once
#include "gfdm_rowgeom.h"

#include <cstddef>
#include <vector>

namespace gfdm {
namespace packed {

// element offset of entry i of lane q inside a pair-packed table of n entries per lane
constexpr size_t entry_offset(int n, int K, int q, int i)
{
    return (n % 2 && i == n - 1) ? (size_t)(n / 2) * 2 * K + q : ((size_t)(i / 2) * K + q) * 2 + i % 2;
}

// appends the pair-packed form of planes[n][K] to dst, padded with `fill` to `elems` elements (>= rowgeom::packed_elems(n, K), even);
// dst.size() must be even (16-byte alignment of the table inside the blob)
template <class C>
void append_pairs(std::vector<C>& dst, const C* planes, int n, int K, size_t elems, C fill)
{
    const size_t at = dst.size();
    dst.resize(at + elems, fill);
    for (int i = 0; i < n; ++i)
        for (int q = 0; q < K; ++q) dst[at + entry_offset(n, K, q, i)] = planes[(size_t)i * K + q];
}

// the twiddles: twT = [M][K]; the region keeps the M K (+ 1) elements of the plain table, the tail is filled with plane 0 (ones)
template <class C>
void append_twiddles(std::vector<C>& dst, const C* twT, int M, int K)
{
    append_pairs(dst, twT + K, M - 1, K, rowgeom::packed_roots_offset(K, M), twT[0]);
}

// the subcarrier-FFT roots: wK = [K]
template <class C>
void append_roots(std::vector<C>& dst, const C* wK, int K)
{
    const int n = rowgeom::root_count(K);
    std::vector<C> planes((size_t)n * K);
    for (int i = 0; i < n; ++i)
        for (int q = 0; q < K; ++q) planes[(size_t)i * K + q] = wK[rowgeom::root_index(K, q, i)];
    append_pairs(dst, planes.data(), n, K, rowgeom::packed_elems(n, K), wK[0]);
}

}  // namespace packed
}  // namespace gfdm
