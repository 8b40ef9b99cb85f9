// Channel model between the burst shaper and the synchroniser: a fixed FIR (multipath), a frequency offset and white Gaussian noise on a
// continuous stream, complex64 or interleaved int16 I/Q out (GNU Radio's channels.channel_model with epsilon = 1, as the reference's
// end-to-end flowgraph uses it: examples/gfdm_simulation_demo.grc).  The contract is written out in include/gfdm_hip.h.
//
// One kernel, k_channel<SC16>, a stream stage (gfdm_streamtile.h: the output tiles, step 1 and step 3) with tiles of kTile samples.
//   1. the halo: the input samples [i_lo - T, i_hi + 1) -- the tile, its T - 1 past samples and one more at either end for the pairs of step 2;
//   2. a lane owns aligned PAIRS of absolute sample indices (2p, 2p + 1): one Philox call serves both.  Whatever the parity of `offset`
//      and the alignment of `out` are, a tile meets at most max_groups(kTile, 2) pairs, which is why kTile is 2044 and not 2048: four
//      pairs a lane.  FIR (LDS reads shared by the two samples), mixer, noise, and the results go to a second LDS array in output format.
// T, the all-real-taps case, f == 0 and s == 0 are launch-uniform branches; the taps are kernel arguments.
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
#include "gfdm_philox.h"
#include "gfdm_streamtile.h"

#include <algorithm>
#include <cmath>

using gfdm::cf;
using gfdm::api_fail;

namespace {

constexpr int kLanes = 256;
constexpr int kMaxTaps = 64;
constexpr int kTile = 2044;               // samples per tile: a multiple of 4 whose pairs fit kPairsPerLane * kLanes
constexpr int kPairsPerLane = 4;
constexpr int kStage = kTile + kMaxTaps + 4;      // input samples in LDS
constexpr int kMaxTiles = 8192;           // workgroups per launch; the tiles beyond are strided over
static_assert(kTile % 4 == 0 && gfdm::max_groups(kTile, 2) <= kPairsPerLane * kLanes, "tile geometry");
static_assert(kStage % 2 == 0 && kStage >= gfdm::max_stage(kTile, kMaxTaps, 1, 2), "the stage holds a tile's halo");

struct ChannelArgs {
    const cf* in;            // sample 0; `history` samples in front of it are readable
    int64_t n, history, offset;
    double f;                // cycles per sample
    float sigma;             // (float)(noise_voltage / sqrt 2)
    float gain;              // sc16
    uint32_t key0, key1;     // seed, low and high word
    int T;
    int real_taps;           // every tap has imaginary part 0: the products with it are left out
    int mix, noisy;          // f != 0, noise_voltage != 0
    cf taps[kMaxTaps];
};

// v for the samples i and i + 1, whose x[i + 1 - t] lie at xs[k1 - t]: one LDS read per tap serves both.  The first term is a product,
// the others follow by fma with t ascending: the same chain for every sample.
template <bool REAL>
__device__ __forceinline__ void fir_pair(const ChannelArgs& a, const cf* xs, int k1, cf& v0, cf& v1)
{
    cf hi = xs[k1], lo = xs[k1 - 1];
    const cf h0 = a.taps[0];
    if (REAL) {
        v1 = make_float2(h0.x * hi.x, h0.x * hi.y);
        v0 = make_float2(h0.x * lo.x, h0.x * lo.y);
    } else {
        v1 = make_float2(fmaf(-h0.y, hi.y, h0.x * hi.x), fmaf(h0.y, hi.x, h0.x * hi.y));
        v0 = make_float2(fmaf(-h0.y, lo.y, h0.x * lo.x), fmaf(h0.y, lo.x, h0.x * lo.y));
    }
    for (int t = 1; t < a.T; ++t) {
        const cf h = a.taps[t];
        hi = lo;
        lo = xs[k1 - 1 - t];
        v1.x = fmaf(h.x, hi.x, v1.x);
        v1.y = fmaf(h.x, hi.y, v1.y);
        v0.x = fmaf(h.x, lo.x, v0.x);
        v0.y = fmaf(h.x, lo.y, v0.y);
        if (!REAL) {
            v1.x = fmaf(-h.y, hi.y, v1.x);
            v1.y = fmaf(h.y, hi.x, v1.y);
            v0.x = fmaf(-h.y, lo.y, v0.x);
            v0.y = fmaf(h.y, lo.x, v0.y);
        }
    }
}

// v * exp(j 2 pi frac(f * idx)): the product f * idx rounded to fp64 ONCE (no fused multiply-subtract: the restatement rounds it too),
// its distance to the nearest integer exact, then fp32
__device__ __forceinline__ cf mixed(cf v, double f, int64_t idx)
{
    double p, frac;
    {
#pragma clang fp contract(off)
        p = f * (double)idx;
        frac = p - rint(p);
    }
    const float turns2 = (float)(2.0 * frac);                   // in [-1, 1]: the phase in units of pi
    float sn, cs;
    sincospif(turns2, &sn, &cs);
    return make_float2(fmaf(-v.y, sn, v.x * cs), fmaf(v.y, cs, v.x * sn));
}

// w of the contract from the two Philox words of a sample.  u = (m + 0.5) 2^-24 has 25 significant bits for m >= 2^23: uf is its fp32
// rounding, d = u - uf (0 or +-2^-25, formed exactly) and ln u = ln uf + d / uf to second order (d / uf <= 2^-24).  Without the second
// term the error of ln u near u = 1 is as large as ln u itself.
__device__ __forceinline__ cf gaussian_pair(uint32_t k0, uint32_t k1)
{
    const float m = (float)(k0 >> 8);
    const float uf = fmaf(m, 0x1p-24f, 0x1p-25f);
    const float d = fmaf(m, 0x1p-24f, -uf) + 0x1p-25f;
    const float ln_u = logf(uf) + d / uf;
    const float radius = sqrtf(-2.f * ln_u);
    float sn, cs;
    sincospif((float)(k1 >> 8) * 0x1p-23f, &sn, &cs);           // 2 t, exact
    return make_float2(radius * cs, radius * sn);
}

// SC16 = 0: out is complex64; 1: interleaved int16 I/Q
template <int SC16>
__global__ __launch_bounds__(kLanes) void k_channel(ChannelArgs a, void* __restrict__ out)
{
    constexpr int VPS = SC16 ? 4 : 2;            // samples per 16-byte vector
    __shared__ __attribute__((aligned(16))) cf xs[kStage];
    __shared__ __attribute__((aligned(16))) gfdm::stored_t<SC16> ys[kTile];
    const gfdm::StreamTiles tiles(out, VPS, a.n, kTile / VPS);
    for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
        const gfdm::TileSpan t = tiles.tile(tile);
        const int64_t s0 = t.s0, i_lo = t.i_lo, i_hi = t.i_hi;                        // ys[k] is sample s0 + k
        // 1. xs[k] = x[j0 + k] for j0 + k < i_hi + 1
        const int64_t j0 = gfdm::stage_first(a.in, i_lo - a.T);
        gfdm::stage_in<0>(xs, a.in, j0, (int)(i_hi + 1 - j0), a.history, a.n, kLanes);
        __syncthreads();
        // 2. the pairs of absolute indices that meet [i_lo, i_hi)
        const int64_t p_lo = (a.offset + i_lo) >> 1, p_hi = (a.offset + i_hi - 1) >> 1;
        const int npairs = (int)(p_hi - p_lo + 1);                                   // <= max_groups(kTile, 2)
#pragma unroll 1
        for (int u = 0; u < kPairsPerLane; ++u) {
            const int q = u * kLanes + threadIdx.x;
            if (q >= npairs) break;
            const int64_t pair = p_lo + q, idx = 2 * pair, i0 = idx - a.offset;      // samples i0 (may be i_lo - 1) and i0 + 1 (may be i_hi)
            cf y0, y1;
            const int k1 = (int)(i0 + 1 - j0);                                       // T + 1 <= k1 + ... : xs[k1 - 1 - t] stays inside for t < T
            if (a.real_taps) fir_pair<true>(a, xs, k1, y0, y1);
            else fir_pair<false>(a, xs, k1, y0, y1);
            if (a.mix) {
                y0 = mixed(y0, a.f, idx);
                y1 = mixed(y1, a.f, idx + 1);
            }
            if (a.noisy) {
                const gfdm::Philox4 r = gfdm::philox4x32_10((uint32_t)pair, (uint32_t)((uint64_t)pair >> 32), 0u, 0u, a.key0, a.key1);
                const cf w0 = gaussian_pair(r.v[0], r.v[1]), w1 = gaussian_pair(r.v[2], r.v[3]);
                y0 = make_float2(fmaf(a.sigma, w0.x, y0.x), fmaf(a.sigma, w0.y, y0.y));
                y1 = make_float2(fmaf(a.sigma, w1.x, y1.x), fmaf(a.sigma, w1.y, y1.y));
            }
            if (i0 >= i_lo) ys[i0 - s0] = gfdm::to_stored<SC16>(y0, a.gain);
            if (i0 + 1 < i_hi) ys[i0 + 1 - s0] = gfdm::to_stored<SC16>(y1, a.gain);
        }
        __syncthreads();
        // 3.
        gfdm::store_tile<SC16>(static_cast<unsigned char*>(out), tiles, t, ys, kLanes);
        // (xs is rewritten behind this barrier's predecessor only by lanes that have left step 2; ys is read here and rewritten behind the next tile's first barrier)
    }
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int channel_check(int n_taps, double f, double s, int64_t n, int64_t history, int64_t offset, double gain)
{
    if (n_taps < 1 || n_taps > kMaxTaps) return api_fail(GFDM_HIP_EINVAL, "n_taps must lie in 1 .. 64");
    if (!std::isfinite(f) || std::fabs(f) > 0.5) return api_fail(GFDM_HIP_EINVAL, "frequency_offset must be finite and lie in [-0.5, 0.5] cycles per sample");
    if (!std::isfinite(s) || s < 0.0) return api_fail(GFDM_HIP_EINVAL, "noise_voltage must be finite and >= 0");
    if (!std::isfinite(gain)) return api_fail(GFDM_HIP_EINVAL, "gain must be finite");
    return gfdm::check_stream_span(n, history, offset);
}

int taps_check(const float* taps, int n_taps)
{
    if (n_taps < 1 || n_taps > kMaxTaps) return api_fail(GFDM_HIP_EINVAL, "n_taps must lie in 1 .. 64");
    if (!taps) return api_fail(GFDM_HIP_EINVAL, "NULL taps");
    for (int i = 0; i < 2 * n_taps; ++i)
        if (!std::isfinite(taps[i])) return api_fail(GFDM_HIP_EINVAL, "taps must be finite");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_channel_model {
    gfdm::DeviceCtx ctx;
    int T = 0;
    int real_taps = 1;
    cf taps[kMaxTaps] = {};
    double f = 0.0, s = 0.0;
    uint64_t seed = 0;
};

namespace {

int check_call(const gfdm_hip_channel_model* h, const void* out, const void* in, int sc16, int64_t n, int64_t history, int64_t offset, double gain)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = channel_check(h->T, h->f, h->s, n, history, offset, gain);
    if (rc != GFDM_HIP_OK) return rc;
    if (n == 0) return GFDM_HIP_OK;
    if (!out || !in) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return gfdm::check_no_overlap(out, sc16 ? 4 : 8, n, in, sizeof(cf), n, history, "n", "the channel model");      // the FIR reads neighbours
}

// the one launch of a call; out and in are device pointers, the handle's setter values are read here
int channel_enqueue(const gfdm_hip_channel_model* h, int sc16, void* out, const cf* in, int64_t n, int64_t history, int64_t offset, double gain, hipStream_t s)
{
    if (n == 0) return GFDM_HIP_OK;
    const int rc = gfdm::check_sample_alignment(out, sc16 ? 4 : 8, in, sizeof(cf));
    if (rc != GFDM_HIP_OK) return rc;
    ChannelArgs a;
    a.in = in;
    a.n = n;
    a.history = history;
    a.offset = offset;
    a.f = h->f;
    a.sigma = (float)(h->s / std::sqrt(2.0));
    a.gain = (float)gain;
    a.key0 = (uint32_t)h->seed;
    a.key1 = (uint32_t)(h->seed >> 32);
    a.T = h->T;
    a.real_taps = h->real_taps;
    a.mix = h->f != 0.0;
    a.noisy = h->s != 0.0;
    std::copy(h->taps, h->taps + kMaxTaps, a.taps);
    const int vps = sc16 ? 4 : 2;
    const dim3 grid((unsigned)std::min<int64_t>(gfdm::StreamTiles(out, vps, n, kTile / vps).ntiles, kMaxTiles));
    if (sc16) hipLaunchKernelGGL(k_channel<1>, grid, dim3(kLanes), 0, s, a, out);
    else hipLaunchKernelGGL(k_channel<0>, grid, dim3(kLanes), 0, s, a, out);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// check_call, then channel_enqueue: on the caller's stream, or between an upload and a download on the handle's (gfdm::stream_call)
int channel_call(gfdm_hip_channel_model* h, bool host, int sc16, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain, void* stream)
{
    return gfdm::stream_call(h, host, sc16, out, in, n, history, offset, gain, stream, check_call, channel_enqueue);
}

}  // namespace

extern "C" {

int gfdm_hip_channel_model_create(gfdm_hip_channel_model** out, const float* taps, int n_taps, double frequency_offset, double noise_voltage, uint64_t seed,
                                  int device)
{
    return gfdm::create_handle(out, device, [&](gfdm_hip_channel_model& h) -> int {
        int rc = taps_check(taps, n_taps);
        if (rc == GFDM_HIP_OK) rc = channel_check(n_taps, frequency_offset, noise_voltage, 0, 0, 0, 1.0);
        if (rc != GFDM_HIP_OK) return rc;
        h.T = n_taps;
        for (int t = 0; t < n_taps; ++t) {
            h.taps[t] = make_float2(taps[2 * t], taps[2 * t + 1]);
            if (taps[2 * t + 1] != 0.f) h.real_taps = 0;
        }
        h.f = frequency_offset;
        h.s = noise_voltage;
        h.seed = seed;
        return GFDM_HIP_OK;
    });
}

int gfdm_hip_channel_model_destroy(gfdm_hip_channel_model* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_channel_model_n_taps(const gfdm_hip_channel_model* h) { return h ? h->T : GFDM_HIP_EINVAL; }
int gfdm_hip_channel_model_taps(const gfdm_hip_channel_model* h, float* taps)
{
    if (!h || !taps) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    for (int t = 0; t < h->T; ++t) {
        taps[2 * t] = h->taps[t].x;
        taps[2 * t + 1] = h->taps[t].y;
    }
    return GFDM_HIP_OK;
}
int gfdm_hip_channel_model_frequency_offset(const gfdm_hip_channel_model* h, double* frequency_offset)
{
    if (!h || !frequency_offset) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    *frequency_offset = h->f;
    return GFDM_HIP_OK;
}
int gfdm_hip_channel_model_noise_voltage(const gfdm_hip_channel_model* h, double* noise_voltage)
{
    if (!h || !noise_voltage) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    *noise_voltage = h->s;
    return GFDM_HIP_OK;
}
int gfdm_hip_channel_model_seed(const gfdm_hip_channel_model* h, uint64_t* seed)
{
    if (!h || !seed) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    *seed = h->seed;
    return GFDM_HIP_OK;
}

int gfdm_hip_channel_model_set_frequency_offset(gfdm_hip_channel_model* h, double frequency_offset)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = channel_check(h->T, frequency_offset, h->s, 0, 0, 0, 1.0);
    if (rc == GFDM_HIP_OK) h->f = frequency_offset;
    return rc;
}
int gfdm_hip_channel_model_set_noise_voltage(gfdm_hip_channel_model* h, double noise_voltage)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = channel_check(h->T, h->f, noise_voltage, 0, 0, 0, 1.0);
    if (rc == GFDM_HIP_OK) h->s = noise_voltage;
    return rc;
}
int gfdm_hip_channel_model_set_seed(gfdm_hip_channel_model* h, uint64_t seed)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    h->seed = seed;
    return GFDM_HIP_OK;
}

int gfdm_hip_channel_model_check(int n_taps, double frequency_offset, double noise_voltage, int64_t n, int64_t history, int64_t offset, double gain)
{
    return channel_check(n_taps, frequency_offset, noise_voltage, n, history, offset, gain);
}

int gfdm_hip_channel_model_apply_device(gfdm_hip_channel_model* h, void* out, const void* in, int64_t n, int64_t history, int64_t offset, void* stream)
{
    return channel_call(h, false, 0, out, in, n, history, offset, 1.0, stream);
}
int gfdm_hip_channel_model_apply_sc16_device(gfdm_hip_channel_model* h, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain,
                                             void* stream)
{
    return channel_call(h, false, 1, out, in, n, history, offset, gain, stream);
}
int gfdm_hip_channel_model_apply_host(gfdm_hip_channel_model* h, float* out, const float* in, int64_t n, int64_t history, int64_t offset)
{
    return channel_call(h, true, 0, out, in, n, history, offset, 1.0, nullptr);
}
int gfdm_hip_channel_model_apply_sc16_host(gfdm_hip_channel_model* h, int16_t* out, const float* in, int64_t n, int64_t history, int64_t offset, double gain)
{
    return channel_call(h, true, 1, out, in, n, history, offset, gain, nullptr);
}

}  // extern "C"
