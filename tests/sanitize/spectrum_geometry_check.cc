// TEST-ONLY brute force of the host geometry of the spectrum meter, gr-gfdm_amd/csrc/gfdm_spectrum.h, as plain C++ under AddressSanitizer +
// UBSan: no GPU, no Python.  What it covers is what the kernels trust without a check of their own:
//   runs:    for every nfft and every total in 0 .. 3 slots + 7, around every multiple of slots * kMaxGroups up to 3, and at 2^40: the runs
//            [lo(g), hi(g)) are in order, none is empty, they cover [0, total) exactly, a run is a whole number of trips, groups <=
//            kMaxGroups (the partial rows the handle owns) and groups = min(kMaxGroups, trips) where the trips divide evenly;
//   power:   the same for the tiles of the power pass, and tiles_per_group + groups <= tiles + 1 (the depth of power_sum's error bound);
//   plan:    segments_of against a count by hand for every nfft, hop in {1, 3, nfft / 2, nfft - 1, nfft} and n in 0 .. 3 nfft + 5: the last
//            segment ends inside n, one more would not;
//   origins: burst_origin against the live rule written out, on every edge of start, first, j and stream_len, with no signed overflow at
//            the limits the argument table admits (UBSan would report it);
//   tables:  check_shape, check_stream, check_bursts at their edges.
#include "gfdm_spectrum.h"

#include <cstdio>
#include <initializer_list>

namespace sp = gfdm::spectrum;

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

void check_runs(int nfft, int64_t total)
{
    const sp::Runs r(total, nfft);
    CHECK(r.slots == sp::kSlotSamples / nfft && r.slots >= 1, "nfft %d: slots %d", nfft, r.slots);
    if (total == 0) {
        CHECK(r.groups == 0, "nfft %d total 0: groups %d", nfft, r.groups);
        return;
    }
    CHECK(r.groups >= 1 && r.groups <= sp::kMaxGroups, "nfft %d total %lld: groups %d", nfft, (long long)total, r.groups);
    CHECK(r.per > 0 && r.per % r.slots == 0, "nfft %d total %lld: per %lld", nfft, (long long)total, (long long)r.per);
    const int64_t trips = (total + r.slots - 1) / r.slots;
    if (trips <= sp::kMaxGroups) CHECK(r.groups == trips && r.per == r.slots, "nfft %d total %lld: %d groups for %lld trips", nfft, (long long)total, r.groups, (long long)trips);
    if (trips % sp::kMaxGroups == 0) CHECK(r.groups == sp::kMaxGroups, "nfft %d total %lld: groups %d", nfft, (long long)total, r.groups);
    int64_t next = 0;
    for (int g = 0; g < r.groups; ++g) {
        CHECK(r.lo(g) == next && r.lo(g) < r.hi(g) && r.hi(g) - r.lo(g) <= r.per, "nfft %d total %lld run %d: [%lld, %lld)", nfft, (long long)total, g,
              (long long)r.lo(g), (long long)r.hi(g));
        next = r.hi(g);
    }
    CHECK(next == total, "nfft %d total %lld: the runs end at %lld", nfft, (long long)total, (long long)next);
}

void check_power(int64_t n)
{
    const sp::PowerRuns r(n);
    if (n == 0) {
        CHECK(r.groups == 0 && r.tiles == 0, "n 0");
        return;
    }
    CHECK(r.tiles == (n + sp::kPowerTile - 1) / sp::kPowerTile, "n %lld: tiles %lld", (long long)n, (long long)r.tiles);
    CHECK(r.groups >= 1 && r.groups <= sp::kPowerGroups && r.per >= 1, "n %lld: groups %d per %lld", (long long)n, r.groups, (long long)r.per);
    CHECK((int64_t)(r.groups - 1) * r.per < r.tiles && (int64_t)r.groups * r.per >= r.tiles, "n %lld: groups %d of %lld tiles do not cover %lld", (long long)n, r.groups,
          (long long)r.per, (long long)r.tiles);
    CHECK(r.per + r.groups <= r.tiles + 1, "n %lld: per %lld + groups %d above tiles %lld + 1", (long long)n, (long long)r.per, r.groups, (long long)r.tiles);
}

void check_plan(int nfft)
{
    for (int64_t hop : { (int64_t)1, (int64_t)3, (int64_t)nfft / 2, (int64_t)nfft - 1, (int64_t)nfft })
        for (int64_t n = 0; n <= 3 * nfft + 5; ++n) {
            const int64_t s = sp::segments_of(nfft, hop, n);
            int64_t by_hand = 0;
            while (by_hand * hop + nfft <= n) ++by_hand;
            CHECK(s == by_hand, "nfft %d hop %lld n %lld: %lld segments, by hand %lld", nfft, (long long)hop, (long long)n, (long long)s, (long long)by_hand);
        }
}

void check_origins()
{
    const int64_t big = sp::kMaxLen, far = sp::kMaxFirst;
    const int64_t starts[] = { -1, 0, 1, 100, big - 4096, big, big + 1, INT64_MAX, INT64_MIN };
    const int64_t firsts[] = { -far, -101, -100, -1, 0, 1, 4096, far };
    const int64_t lens[] = { 0, 15, 16, 17, 4096, 100000, big };
    const int64_t js[] = { 0, 1, 7, ((int64_t)1 << 40) - 1 };
    for (int nfft : { 16, 4096 })
        for (int64_t hop : { (int64_t)1, (int64_t)nfft })
            for (int64_t start : starts)
                for (int64_t first : firsts)
                    for (int64_t len : lens)
                        for (int64_t j : js) {
                            const int64_t o = sp::burst_origin(start, first, j, hop, nfft, len);
                            bool live = start >= 0 && start <= big;
                            __int128 wide = 0;
                            if (live) {
                                wide = (__int128)start + first + (__int128)j * hop;
                                live = wide >= 0 && wide + nfft <= len;
                            }
                            CHECK(live ? (__int128)o == wide : o == -1, "start %lld first %lld j %lld hop %lld nfft %d len %lld: %lld", (long long)start,
                                  (long long)first, (long long)j, (long long)hop, nfft, (long long)len, (long long)o);
                        }
}

void check_tables()
{
    for (int64_t nfft = -1; nfft <= 8200; ++nfft) {
        const int a = sp::log2_of(nfft);
        bool pow2 = false;
        for (int b = 4; b <= 12; ++b) pow2 |= nfft == ((int64_t)1 << b);
        CHECK((a >= 0) == pow2 && (a < 0 || ((int64_t)1 << a) == nfft), "log2_of(%lld) = %d", (long long)nfft, a);
        CHECK((sp::check_shape(nfft, 1) == nullptr) == pow2, "check_shape(%lld, 1)", (long long)nfft);
    }
    CHECK(sp::check_shape(64, 0) && sp::check_shape(64, 65) && sp::check_shape(64, -1) && !sp::check_shape(64, 64) && !sp::check_shape(64, 1), "hop edges");
    CHECK(sp::check_stream(-1) && !sp::check_stream(0) && !sp::check_stream(sp::kMaxLen) && sp::check_stream(sp::kMaxLen + 1), "n edges");
    CHECK(!sp::check_bursts(0, 0, 0, 0) && sp::check_bursts(-1, 0, 1, 1) && sp::check_bursts(sp::kMaxLen + 1, 0, 1, 1), "stream_len edges");
    CHECK(sp::check_bursts(1, sp::kMaxFirst + 1, 1, 1) && sp::check_bursts(1, -sp::kMaxFirst - 1, 1, 1) && !sp::check_bursts(1, -sp::kMaxFirst, 1, 1), "first edges");
    CHECK(sp::check_bursts(1, 0, -1, 1) && sp::check_bursts(1, 0, 1, -1), "negative counts");
    CHECK(!sp::check_bursts(1, 0, (int64_t)1 << 20, (int64_t)1 << 20) && sp::check_bursts(1, 0, ((int64_t)1 << 20) + 1, (int64_t)1 << 20) &&
              sp::check_bursts(1, 0, INT64_MAX, INT64_MAX),
          "segment count edges");
}

}  // namespace

int main()
{
    for (int a = sp::kMinLog; a <= sp::kMaxLog; ++a) {
        const int nfft = 1 << a;
        const int64_t slots = sp::kSlotSamples / nfft;
        for (int64_t total = 0; total <= 3 * slots + 7; ++total) check_runs(nfft, total);
        for (int64_t m = 1; m <= 3; ++m)
            for (int64_t d = -slots - 2; d <= slots + 2; ++d) check_runs(nfft, m * slots * sp::kMaxGroups + d);
        check_runs(nfft, (int64_t)1 << 40);
        check_runs(nfft, sp::kMaxLen);
        check_plan(nfft);
    }
    for (int64_t n = 0; n <= 3 * sp::kPowerTile + 5; ++n) check_power(n);
    for (int64_t m = 1; m <= 3; ++m)
        for (int64_t d = -2; d <= 2; ++d) check_power(m * sp::kPowerTile * sp::kPowerGroups + d);
    for (int64_t tiles = 1; tiles <= 5000; ++tiles) check_power(tiles * sp::kPowerTile);
    check_power(sp::kMaxLen);
    check_origins();
    check_tables();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("spectrum geometry check OK\n");
    return 0;
}
