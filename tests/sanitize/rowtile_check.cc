// TEST-ONLY brute force of the host half of gr-gfdm_amd/csrc/gfdm_rowtile.h -- the geometry the five row stages and their enqueue functions
// share -- as plain C++ under AddressSanitizer + UBSan: no GPU, no Python.  What it covers is what a row stage's kernel trusts without a
// check of its own:
//   partition:  for the four shapes of the stages (2 complex64, 4 floats, 16 bytes in a 16-byte vector; 4 bytes in a 4-byte word), every
//               misalignment of `out`, tile_vec in {1, 2, 3, 255, 256, 1024} and every n in 0 .. 3 tile + 5 the tiles' [i_lo, i_hi) are in
//               order and cover [0, n) exactly, none is larger than a tile or, for n >= 1, empty;
//   whole:      the whole-vector predicate of store_elems holds exactly for the vectors whose elements all lie in [0, n);
//   grid:       row_grid is the number of aligned tiles of memory that the n elements touch, counted from their byte addresses, never
//               below 1 and never above the cap;
//   cursor:     RowCursor's one division, at(d) and repeated next() agree with plain / and % for every width in 1 .. 40 and every start
//               in the row, for widths {255, 256, 257, 4095, 4097, 2^21} at both ends and the middle, in rows 0, 3 and beyond 2^32
//               elements, for every d in 0 .. kMaxRowReach -- the bound the stages' static_asserts hold their tiles to.
#include <hip/hip_runtime.h>

#include "gfdm_rowtile.h"

#include <cstdio>

namespace {

int g_failed = 0;

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++g_failed <= 20) {                                         \
                fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                               \
                fprintf(stderr, "\n");                                      \
            }                                                               \
        }                                                                   \
    } while (0)

struct Shape {
    const char* stage;
    int vps, vec_bytes;
};
const Shape kShapes[] = { { "map", 2, 16 }, { "soft, unmatch", 4, 16 }, { "encode", 16, 16 }, { "match", 4, 4 } };

// an address `mis` elements behind a vector boundary (never dereferenced)
uintptr_t address(const Shape& s, int mis) { return (uintptr_t)4096 + (uintptr_t)(mis * (s.vec_bytes / s.vps)); }

void check_tiles(const Shape& s, int mis, int tile_vec)
{
    const int tile = tile_vec * s.vps, elem = s.vec_bytes / s.vps;
    const uintptr_t a = address(s, mis);
    for (int64_t n = 0; n <= 3 * tile + 5; ++n) {
        const gfdm::StreamTiles tl(reinterpret_cast<const void*>(a), s.vps, n, tile_vec, s.vec_bytes);
        CHECK(tl.mis == mis, "%s mis %d: %d", s.stage, mis, tl.mis);
        int64_t next = 0;
        for (int64_t k = 0; k < tl.ntiles; ++k) {
            const gfdm::TileSpan t = tl.tile(k);
            CHECK(t.i_lo == next && (n > 0 ? t.i_lo < t.i_hi : t.i_hi == 0) && t.i_hi - t.i_lo <= tile, "%s mis %d tile_vec %d n %lld tile %lld: [%lld, %lld) behind %lld",
                  s.stage, mis, tile_vec, (long long)n, (long long)k, (long long)t.i_lo, (long long)t.i_hi, (long long)next);
            CHECK(t.s0 == tl.first(t.v0) && t.s0 <= t.i_lo && t.i_hi <= tl.first(t.v1), "%s tile %lld: s0 %lld", s.stage, (long long)k, (long long)t.s0);
            next = t.i_hi;
        }
        CHECK(next == n, "%s mis %d tile_vec %d n %lld: the tiles end at %lld", s.stage, mis, tile_vec, (long long)n, (long long)next);
        // (a vector away from both ends of the output differs from its neighbours in nothing the predicate reads: the four at either end)
        for (int64_t v = 0; v < tl.nvec; ++v) {
            if (v == 4) v = std::max(v, tl.nvec - 4);
            const int64_t i = tl.first(v);
            int inside = 0;
            for (int e = 0; e < s.vps; ++e) inside += (i + e >= 0 && i + e < n);
            CHECK((inside > 0 || n == 0) && tl.whole(i) == (inside == s.vps) && (!tl.whole(i) || (a + (uintptr_t)(i * elem)) % (uintptr_t)s.vec_bytes == 0),
                  "%s mis %d n %lld vector %lld", s.stage, mis, (long long)n, (long long)v);
        }
        // the grid of the enqueue functions: the aligned vectors of memory between the first and the last byte of the output, tile_vec a tile
        const int64_t vectors = n ? (int64_t)((a + (uintptr_t)(n * elem) - 1) / (uintptr_t)s.vec_bytes - a / (uintptr_t)s.vec_bytes) + 1 : 0;
        const int64_t touched = std::max<int64_t>((vectors + tile_vec - 1) / tile_vec, 1);
        for (const int cap : { 1, 2, 8192 }) {
            const unsigned grid = gfdm::row_grid(reinterpret_cast<const void*>(a), s.vps, n, tile_vec, cap, s.vec_bytes);
            CHECK((int64_t)grid == std::min<int64_t>(touched, cap) && (n == 0 || tl.ntiles == touched), "%s mis %d tile_vec %d n %lld cap %d: grid %u, %lld tiles touched, ntiles %lld",
                  s.stage, mis, tile_vec, (long long)n, cap, grid, (long long)touched, (long long)tl.ntiles);
        }
    }
}

void check_cursor(int64_t width, int64_t i0, int64_t r0)
{
    const int64_t i_lo = r0 * width + i0;
    const gfdm::RowCursor first(i_lo, width);
    CHECK(first.r == r0 && first.i == i0, "width %lld: element %lld at (%lld, %lld)", (long long)width, (long long)i_lo, (long long)first.r, (long long)first.i);
    gfdm::RowCursor walk = first;
    for (uint32_t d = 0; d <= (uint32_t)gfdm::kMaxRowReach; ++d) {
        const int64_t r = (i_lo + d) / width, i = (i_lo + d) % width;
        const gfdm::RowCursor c = first.at(d);
        CHECK(c.r == r && c.i == i && c.width == width && walk.r == r && walk.i == i, "width %lld start (%lld, %lld) d %u: at (%lld, %lld), next (%lld, %lld)", (long long)width,
              (long long)r0, (long long)i0, d, (long long)c.r, (long long)c.i, (long long)walk.r, (long long)walk.i);
        walk.next();
    }
}

}  // namespace

int main()
{
    for (const Shape& s : kShapes)
        for (const int tile_vec : { 1, 2, 3, 255, 256, 1024 })
            for (int mis = 0; mis < s.vps; ++mis) check_tiles(s, mis, tile_vec);
    for (int64_t width = 1; width <= 40; ++width)
        for (int64_t i0 = 0; i0 < width; ++i0)
            for (const int64_t r0 : { (int64_t)0, (int64_t)3, ((int64_t)1 << 33) / width + 1 }) check_cursor(width, i0, r0);
    for (const int64_t width : { (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)4095, (int64_t)4097, (int64_t)1 << 21 })
        for (const int64_t i0 : { (int64_t)0, (int64_t)1, width / 2, width - 2, width - 1 })
            for (const int64_t r0 : { (int64_t)0, (int64_t)3, ((int64_t)1 << 33) / width + 1 }) check_cursor(width, i0, r0);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("rowtile check OK\n");
    return 0;
}
