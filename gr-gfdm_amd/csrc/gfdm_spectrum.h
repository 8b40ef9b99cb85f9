// Internal: the host geometry of the spectrum meter (gfdm_spectrum.hip) -- which segments a workgroup owns, how many partial rows a call
// writes, the tiles of the power pass, plan and the argument tables -- as plain C++ for the host and the device alike, so that the
// kernels and the enqueue functions cannot disagree.  tests/sanitize/spectrum_geometry_check.cc brute-forces all of it.  Never seen by
// hiprtc (not in JIT_HDRS).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GFDM_SPECTRUM_FN __host__ __device__ __forceinline__
#else
#define GFDM_SPECTRUM_FN inline
#endif

namespace gfdm {
namespace spectrum {

constexpr int kLanes = 256;
constexpr int kPerLane = 16;                              // samples of a segment a lane holds in a pass: one radix-16 codelet
constexpr int kSlotSamples = kLanes * kPerLane;           // 4096 samples in flight per workgroup: 4096 / nfft segments side by side
constexpr int kMinLog = 4;
constexpr int kMaxLog = 12;
constexpr int kMaxGroups = 1024;                          // workgroups of a PSD launch = partial rows the handle owns
constexpr int kPowerPer = 8;                              // samples a lane takes of a tile of the power pass
constexpr int kPowerTile = kLanes * kPowerPer;            // 2048 samples
constexpr int kPowerGroups = 1024;                        // workgroups of a power launch = power partials the handle owns
constexpr int kHistBins = 512;
constexpr int kHistBias = 760;                            // bits(2^-32) >> 20
constexpr int kHeadFields = 8;
constexpr int64_t kMaxLen = (int64_t)1 << 61;             // samples of a stream
constexpr int64_t kMaxFirst = (int64_t)1 << 60;
constexpr int64_t kMaxSegments = (int64_t)1 << 40;        // segments of an accumulate_at call

// a with nfft = 2^a, or -1 where nfft is no power of two in 2^kMinLog .. 2^kMaxLog
GFDM_SPECTRUM_FN int log2_of(int64_t nfft)
{
    for (int a = kMinLog; a <= kMaxLog; ++a)
        if (nfft == ((int64_t)1 << a)) return a;
    return -1;
}

// segments of nfft samples every hop samples that lie inside n samples
GFDM_SPECTRUM_FN int64_t segments_of(int64_t nfft, int64_t hop, int64_t n) { return n < nfft ? 0 : (n - nfft) / hop + 1; }

// The runs of a PSD launch over `total` segments: `slots` segments go through a workgroup side by side (one trip), a workgroup owns `per`
// consecutive segments -- a whole number of trips -- and `groups` workgroups cover them: workgroup g owns [g per, min((g + 1) per, total)).
// A function of (total, nfft) alone: so is the order of every sum.
struct Runs {
    int64_t total, per;
    int slots, groups;
    GFDM_SPECTRUM_FN Runs(int64_t total_, int nfft) : total(total_), per(0), slots(kSlotSamples / nfft), groups(0)
    {
        if (total <= 0) return;
        const int64_t trips = (total + slots - 1) / slots;
        const int64_t trips_per = (trips + kMaxGroups - 1) / kMaxGroups;
        per = trips_per * slots;
        groups = (int)((total + per - 1) / per);
    }
    GFDM_SPECTRUM_FN int64_t lo(int g) const { return (int64_t)g * per; }
    GFDM_SPECTRUM_FN int64_t hi(int g) const { return lo(g) + per < total ? lo(g) + per : total; }
};

// The tiles of the power pass over n samples: tile t is the samples [t kPowerTile, min((t + 1) kPowerTile, n)), workgroup g owns the tiles
// [g per, min((g + 1) per, tiles))
struct PowerRuns {
    int64_t tiles, per;
    int groups;
    GFDM_SPECTRUM_FN explicit PowerRuns(int64_t n) : tiles(0), per(0), groups(0)
    {
        if (n <= 0) return;
        tiles = (n + kPowerTile - 1) / kPowerTile;
        per = (tiles + kPowerGroups - 1) / kPowerGroups;
        groups = (int)((tiles + per - 1) / per);
    }
};

// the origin of segment j of burst b, or -1 where the segment is not live (include/gfdm_hip.h, accumulate_at); b < n_live is the caller's
GFDM_SPECTRUM_FN int64_t burst_origin(int64_t start, int64_t first, int64_t j, int64_t hop, int64_t nfft, int64_t stream_len)
{
    if (start < 0 || start > kMaxLen) return -1;
    const int64_t o = start + first + j * hop;            // |first| <= 2^60, j hop < 2^52: no overflow
    return (o < 0 || o > stream_len - nfft) ? -1 : o;
}

// the argument tables, as messages (NULL: fine)
inline const char* check_shape(int64_t nfft, int64_t hop)
{
    if (log2_of(nfft) < 0) return "nfft must be a power of two in 16 .. 4096";
    if (hop < 1 || hop > nfft) return "hop must lie in 1 .. nfft";
    return nullptr;
}

inline const char* check_stream(int64_t n)
{
    if (n < 0) return "n must be >= 0";
    if (n > kMaxLen) return "n must not exceed 2^61";
    return nullptr;
}

inline const char* check_bursts(int64_t stream_len, int64_t first, int64_t seg_per_burst, int64_t n_bursts)
{
    if (stream_len < 0 || stream_len > kMaxLen) return "stream_len must lie in 0 .. 2^61";
    if (first < -kMaxFirst || first > kMaxFirst) return "first must lie in -2^60 .. 2^60";
    if (seg_per_burst < 0 || n_bursts < 0) return "seg_per_burst and n_bursts must be >= 0";
    if (seg_per_burst > 0 && n_bursts > kMaxSegments / seg_per_burst) return "seg_per_burst * n_bursts must not exceed 2^40";
    return nullptr;
}

}  // namespace spectrum
}  // namespace gfdm
