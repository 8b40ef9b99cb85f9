// Channel model between the burst shaper and the synchroniser: a fixed FIR (multipath), a frequency offset and white Gaussian noise on a
// continuous stream, complex64 or interleaved int16 I/Q out (GNU Radio's channels.channel_model with epsilon = 1, as the reference's
// end-to-end flowgraph uses it: examples/gfdm_simulation_demo.grc).  The contract is written out in include/gfdm_hip.h.
//
// One kernel, k_channel<SC16>.  As in k_shaper_place the OUTPUT is tiled: the stream is cut into 16-byte vectors aligned in memory (2
// complex64 or 4 sc16 samples), a workgroup takes kTile samples' worth of them.  Per tile
//   1. the input samples [i_lo - T, i_hi + 1) -- the tile, its T - 1 halo and one more at either end for the pairs of step 2 -- go to
//      LDS once, in 16-byte loads aligned in memory, sample by sample where history, n or the alignment of `in` cuts a vector;
//   2. a lane owns aligned PAIRS of absolute sample indices (2p, 2p + 1): one Philox call serves both.  Whatever the parity of `offset`
//      and the alignment of `out` are, a tile meets at most kTile / 2 + 1 pairs, which is why kTile is 2044 and not 2048: four pairs a
//      lane.  FIR (LDS reads shared by the two samples), mixer, noise, and the results go to a second LDS array in output format;
//   3. the tile leaves in 16-byte stores aligned in memory; the first and last samples of an unaligned stream go out one by one.
// T, the all-real-taps case, f == 0 and s == 0 are launch-uniform branches; the taps are kernel arguments.
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
#include "gfdm_philox.h"
#include "gfdm_sc16out.h"

#include <algorithm>
#include <climits>
#include <cmath>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::misaligned;

namespace {

constexpr int kLanes = 256;
constexpr int kMaxTaps = 64;
constexpr int kTile = 2044;               // samples per tile: a multiple of 4 with kTile / 2 + 1 <= kPairsPerLane * kLanes
constexpr int kPairsPerLane = 4;
constexpr int kStage = kTile + kMaxTaps + 4;      // input samples in LDS: tile + T + 1, + 1 for the alignment of the first vector, rounded up to even
constexpr int kMaxTiles = 8192;           // workgroups per launch; the tiles beyond are strided over
constexpr int64_t kMaxIndex = (int64_t)1 << 62;
static_assert(kTile % 4 == 0 && kTile / 2 + 1 <= kPairsPerLane * kLanes && kStage % 2 == 0, "tile geometry");

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
    constexpr int SB = 16 / VPS;                 // bytes per sample
    constexpr int kTileVec = kTile / VPS;
    using Stored = typename std::conditional<SC16 != 0, unsigned, cf>::type;
    __shared__ __attribute__((aligned(16))) cf xs[kStage];
    __shared__ __attribute__((aligned(16))) Stored ys[kTile];
    const int mis = (int)(((uintptr_t)out / SB) % VPS);        // samples between the 16-byte boundary in front of `out` and `out`
    const int in_mis = (int)(((uintptr_t)a.in / sizeof(cf)) & 1);
    const int64_t nvec = (a.n + mis + VPS - 1) / VPS;
    const int64_t ntiles = (nvec + kTileVec - 1) / kTileVec;
    unsigned char* const base = static_cast<unsigned char*>(out);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t v0 = tile * kTileVec, v1 = std::min(v0 + kTileVec, nvec);
        const int64_t s0 = v0 * VPS - mis;                                            // ys[k] is sample s0 + k
        const int64_t i_lo = std::max(s0, (int64_t)0), i_hi = std::min(v1 * VPS - mis, a.n);
        // 1. xs[k] = x[j0 + k] for j0 + k < i_hi + 1; j0 <= i_lo - T sits on a 16-byte boundary of the input
        const int64_t g0 = i_lo - a.T, j0 = g0 - ((g0 + in_mis) & 1);
        const int nstage = (int)(i_hi + 1 - j0);                                     // <= kTile + T + 2
        for (int k = 2 * threadIdx.x; k < nstage; k += 2 * kLanes) {
            const int64_t j = j0 + k;
            float4 x2;
            if (j >= -a.history && j + 1 < a.n) {
                x2 = *reinterpret_cast<const float4*>(a.in + j);
            } else {
                const cf xa = (j >= -a.history && j < a.n) ? a.in[j] : make_float2(0.f, 0.f);
                const cf xb = (j + 1 >= -a.history && j + 1 < a.n) ? a.in[j + 1] : make_float2(0.f, 0.f);
                x2 = make_float4(xa.x, xa.y, xb.x, xb.y);
            }
            *reinterpret_cast<float4*>(xs + k) = x2;
        }
        __syncthreads();
        // 2. the pairs of absolute indices that meet [i_lo, i_hi)
        const int64_t p_lo = (a.offset + i_lo) >> 1, p_hi = (a.offset + i_hi - 1) >> 1;
        const int npairs = (int)(p_hi - p_lo + 1);                                   // <= kTile / 2 + 1
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
            if (i0 >= i_lo) {
                if constexpr (SC16) ys[i0 - s0] = gfdm::pack_sc16(y0, a.gain);
                else ys[i0 - s0] = y0;
            }
            if (i0 + 1 < i_hi) {
                if constexpr (SC16) ys[i0 + 1 - s0] = gfdm::pack_sc16(y1, a.gain);
                else ys[i0 + 1 - s0] = y1;
            }
        }
        __syncthreads();
        // 3. the tile's vectors; a vector that the stream fills only in part goes out sample by sample
        for (int64_t v = v0 + threadIdx.x; v < v1; v += kLanes) {
            const int64_t i = v * VPS - mis;
            const int k = (int)(i - s0);
            if (i >= 0 && i + VPS <= a.n) {
                *reinterpret_cast<uint4*>(base + i * SB) = *reinterpret_cast<const uint4*>(ys + k);
            } else {
                for (int e = 0; e < VPS; ++e)
                    if (i + e >= 0 && i + e < a.n) *reinterpret_cast<Stored*>(base + (i + e) * SB) = ys[k + e];
            }
        }
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
    if (n < 0) return api_fail(GFDM_HIP_EINVAL, "n must be >= 0");
    if (history < 0) return api_fail(GFDM_HIP_EINVAL, "history must be >= 0");
    if (offset < 0) return api_fail(GFDM_HIP_EINVAL, "offset must be >= 0");
    if (n > kMaxIndex || offset > kMaxIndex - n) return api_fail(GFDM_HIP_EINVAL, "offset + n must not exceed 2^62");
    const int64_t lim = INT64_MAX / (int64_t)sizeof(cf);
    if (n > lim || history > lim - n) return api_fail(GFDM_HIP_EINVAL, "the byte size of the input overflows int64");
    return GFDM_HIP_OK;
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
    // the FIR reads neighbours: there is no in-place call
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n * (sc16 ? 4 : 8);
    const uintptr_t i0 = (uintptr_t)in - (uintptr_t)history * sizeof(cf), i1 = (uintptr_t)in + (uintptr_t)n * sizeof(cf);
    if (o0 < i1 && i0 < o1) return api_fail(GFDM_HIP_EINVAL, "out overlaps [in - history, in + n): the channel model has no in-place call");
    return GFDM_HIP_OK;
}

// the one launch of a call; out and in are device pointers, the handle's setter values are read here
int channel_enqueue(const gfdm_hip_channel_model* h, int sc16, void* out, const cf* in, int64_t n, int64_t history, int64_t offset, double gain, hipStream_t s)
{
    if (n == 0) return GFDM_HIP_OK;
    if (misaligned(out, sc16 ? 4 : 8) || misaligned(in, 8)) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one sample");
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
    const int vps = sc16 ? 4 : 2, tile_vec = kTile / vps;
    const int64_t ntiles = ((n + vps - 1) / vps + 1 + tile_vec - 1) / tile_vec;      // + 1: an unaligned `out` adds a vector
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, kMaxTiles));
    if (sc16) hipLaunchKernelGGL(k_channel<1>, grid, dim3(kLanes), 0, s, a, out);
    else hipLaunchKernelGGL(k_channel<0>, grid, dim3(kLanes), 0, s, a, out);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int channel_device(gfdm_hip_channel_model* h, int sc16, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain, void* stream)
{
    const int rc = check_call(h, out, in, sc16, n, history, offset, gain);
    if (rc != GFDM_HIP_OK || n == 0) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return channel_enqueue(h, sc16, out, static_cast<const cf*>(in), n, history, offset, gain, s);
    });
}

// upload history + n samples, one enqueue on the handle's stream, download n
int channel_host(gfdm_hip_channel_model* h, int sc16, void* out, const float* in, int64_t n, int64_t history, int64_t offset, double gain)
{
    const int rc = check_call(h, out, in, sc16, n, history, offset, gain);
    if (rc != GFDM_HIP_OK || n == 0) return rc;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(reinterpret_cast<const cf*>(in) - history, (size_t)(history + n));
    const auto y = hc.out(static_cast<unsigned char*>(out), (size_t)n * (sc16 ? 2 * sizeof(int16_t) : sizeof(cf)));
    return hc.run([&](hipStream_t s) { return channel_enqueue(h, sc16, y.dev(), x.dev() + history, n, history, offset, gain, s); });
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
    return channel_device(h, 0, out, in, n, history, offset, 1.0, stream);
}
int gfdm_hip_channel_model_apply_sc16_device(gfdm_hip_channel_model* h, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain,
                                             void* stream)
{
    return channel_device(h, 1, out, in, n, history, offset, gain, stream);
}
int gfdm_hip_channel_model_apply_host(gfdm_hip_channel_model* h, float* out, const float* in, int64_t n, int64_t history, int64_t offset)
{
    return channel_host(h, 0, out, in, n, history, offset, 1.0);
}
int gfdm_hip_channel_model_apply_sc16_host(gfdm_hip_channel_model* h, int16_t* out, const float* in, int64_t n, int64_t history, int64_t offset, double gain)
{
    return channel_host(h, 1, out, in, n, history, offset, gain);
}

}  // extern "C"
