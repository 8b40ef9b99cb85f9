// TEST-ONLY brute force of the tile geometry and the bounds of gr-gfdm_amd/csrc/gfdm_streamtile.h, the host half of the header as plain C++
// under AddressSanitizer + UBSan: no GPU, no Python.  What it covers is what a stream stage's kernel trusts without a check of its own:
//   partition:  for VPS 2 and 4, every misalignment of `out`, tile_vec in {1, 2, 3, 255, 510, 511, 1024} and every n in 0 .. 3 tile_vec VPS + 5
//               the tiles' [i_lo, i_hi) are in order and cover [0, n) exactly, none has more than tile_vec * VPS samples, ntiles (the grid of
//               the enqueue functions) counts them, and for n >= 1 -- no stage launches with n = 0 -- none is empty (the kernels form i_hi - 1);
//   whole:      the whole-vector predicate holds exactly for the vectors whose VPS samples all lie in [0, n);
//   groups:     for every offset in 0 .. 15 the aligned groups of 2 and of 8 absolute indices that a tile meets never exceed max_groups,
//               and reach it for some input;
//   stage:      with the tiles of the channel model (2044 samples, T in front, 1 behind) and of the fading model (2040 samples, T + 7 in
//               front, 7 behind), every T in 1 .. 64 and both alignments of `in`, the staged span never exceeds max_stage (and reaches it),
//               and max_stage(.., 64, ..) fits the LDS arrays the two kernels declare.
#include <hip/hip_runtime.h>

#include "gfdm_streamtile.h"

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

// an address `mis` samples of 16 / vps bytes behind a 16-byte boundary (never dereferenced)
const void* address(int vps, int mis) { return reinterpret_cast<const void*>((uintptr_t)4096 + (uintptr_t)(mis * (16 / vps))); }

int64_t groups_met(int64_t lo, int64_t hi, int64_t offset, int g) { return (offset + hi - 1) / g - (offset + lo) / g + 1; }

void check_partition_and_groups(int vps, int mis, int tile_vec, int64_t reached[2])
{
    const int tile = tile_vec * vps, bound[2] = { gfdm::max_groups(tile, 2), gfdm::max_groups(tile, 8) };
    for (int64_t n = 0; n <= 3 * tile + 5; ++n) {
        const gfdm::StreamTiles tl(address(vps, mis), vps, n, tile_vec);
        CHECK(tl.mis == mis, "vps %d mis %d: %d", vps, mis, tl.mis);
        CHECK(n > 0 ? tl.ntiles >= 1 : tl.ntiles <= 1, "n %lld ntiles %lld", (long long)n, (long long)tl.ntiles);
        int64_t next = 0;
        for (int64_t k = 0; k < tl.ntiles; ++k) {
            const gfdm::TileSpan t = tl.tile(k);
            CHECK(t.i_lo == next && (n > 0 ? t.i_lo < t.i_hi : t.i_hi == 0) && t.i_hi - t.i_lo <= tile,"vps %d mis %d tile_vec %d n %lld tile %lld: [%lld, %lld) behind %lld", vps, mis,
                  tile_vec, (long long)n, (long long)k, (long long)t.i_lo, (long long)t.i_hi, (long long)next);
            CHECK(t.s0 == tl.first(t.v0) && t.s0 <= t.i_lo && t.i_hi <= tl.first(t.v1), "tile %lld: s0 %lld", (long long)k, (long long)t.s0);
            next = t.i_hi;
            for (int64_t offset = 0; offset < 16; ++offset)
                for (int w = 0; w < 2; ++w) {
                    const int64_t met = groups_met(t.i_lo, t.i_hi, offset, w ? 8 : 2);
                    CHECK(met <= bound[w], "vps %d mis %d tile_vec %d n %lld offset %lld: %lld groups of %d, bound %d", vps, mis, tile_vec, (long long)n,
                          (long long)offset, (long long)met, w ? 8 : 2, bound[w]);
                    if (met > reached[w]) reached[w] = met;
                }
        }
        CHECK(next == n, "vps %d mis %d tile_vec %d n %lld: the tiles end at %lld", vps, mis, tile_vec, (long long)n, (long long)next);
    }
}

// (the predicate does not depend on tile_vec.  Every vector of every n below 256; beyond, where a vector away from both ends of the stream
// differs from its neighbours in nothing the predicate reads, the eight at either end)
void check_whole(int vps, int mis, int64_t n_max)
{
    for (int64_t n = 0; n <= n_max; ++n) {
        const gfdm::StreamTiles tl(address(vps, mis), vps, n, 1);
        CHECK(tl.first(0) <= 0 && tl.first(tl.nvec) >= n && (n == 0 || tl.first(tl.nvec - 1) < n), "vps %d mis %d n %lld: %lld vectors", vps, mis, (long long)n,
              (long long)tl.nvec);
        for (int64_t v = 0; v < tl.nvec; ++v) {
            if (n >= 256 && v == 8) v = std::max(v, tl.nvec - 8);
            const int64_t i = tl.first(v);
            int inside = 0;
            for (int e = 0; e < vps; ++e) inside += (i + e >= 0 && i + e < n);
            CHECK((inside > 0 || n == 0) && tl.whole(i) == (inside == vps), "vps %d mis %d n %lld vector %lld", vps, mis, (long long)n, (long long)v);
        }
    }
}

// a stage whose step 1 takes [i_lo - lower, i_hi + upper): lower = T + extra
void check_stage(int tile, int extra, int upper, int lds)
{
    CHECK(lds % 2 == 0 && lds >= gfdm::max_stage(tile, 64 + extra, upper, 2), "tile %d: %d staged samples", tile, lds);
    for (int T = 1; T <= 64; ++T) {
        const int bound = gfdm::max_stage(tile, T + extra, upper, 2);
        int64_t reached = 0;
        for (int vps = 2; vps <= 4; vps += 2)
            for (int mis = 0; mis < vps; ++mis)
                for (int in_mis = 0; in_mis < 2; ++in_mis)
                    for (const int64_t n : { (int64_t)1, (int64_t)2, (int64_t)tile - 1, (int64_t)tile, (int64_t)tile + 1, (int64_t)2 * tile + 3, (int64_t)3 * tile + 5 }) {
                        const gfdm::StreamTiles tl(address(vps, mis), vps, n, tile / vps);
                        const void* const in = reinterpret_cast<const void*>((uintptr_t)8192 + (uintptr_t)(8 * in_mis));
                        for (int64_t k = 0; k < tl.ntiles; ++k) {
                            const gfdm::TileSpan t = tl.tile(k);
                            const int64_t g0 = t.i_lo - T - extra, j0 = gfdm::stage_first(in, g0), nstage = t.i_hi + upper - j0;
                            CHECK(j0 <= g0 && g0 - j0 <= 1 && (j0 + in_mis) % 2 == 0, "first staged sample %lld for %lld", (long long)j0, (long long)g0);
                            CHECK(nstage <= bound, "tile %d T %d vps %d mis %d in_mis %d n %lld: %lld staged, bound %d", tile, T, vps, mis, in_mis, (long long)n,
                                  (long long)nstage, bound);
                            if (nstage > reached) reached = nstage;
                        }
                    }
        CHECK(reached == bound, "tile %d T %d: the largest staged span is %lld, the bound %d", tile, T, (long long)reached, bound);
    }
}

}  // namespace

int main()
{
    const int tile_vecs[] = { 1, 2, 3, 255, 510, 511, 1024 };
    for (int vps = 2; vps <= 4; vps += 2) {
        for (const int tile_vec : tile_vecs) {
            int64_t reached[2] = { 0, 0 };
            for (int mis = 0; mis < vps; ++mis) check_partition_and_groups(vps, mis, tile_vec, reached);
            CHECK(reached[0] == gfdm::max_groups(tile_vec * vps, 2) && reached[1] == gfdm::max_groups(tile_vec * vps, 8), "vps %d tile_vec %d: %lld pairs, %lld runs",
                  vps, tile_vec, (long long)reached[0], (long long)reached[1]);
        }
        for (int mis = 0; mis < vps; ++mis) check_whole(vps, mis, 3 * 1024 * vps + 5);
    }
    check_stage(2044, 0, 1, 2044 + 64 + 4);         // k_channel: kTile, kStage
    check_stage(2040, 7, 7, 2040 + 64 + 16);        // k_fade
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("streamtile check OK\n");
    return 0;
}
