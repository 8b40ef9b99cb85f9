// Fading model between the burst shaper (or the resampler) and the channel model: P paths, each a real delay line of T coefficients times
// a gain that is a sum of S sinusoids of the ABSOLUTE sample index (a stratified Clarke model with an optional line-of-sight term), complex64
// or interleaved int16 I/Q out.  What GNU Radio's channels.selective_fading_model does in a flowgraph; the phases are 64-bit integers, so
// every sample is a pure function of the tables and its index.  The contract is written out in include/gfdm_hip.h.
//
// One kernel, k_fade<SC16>, a stream stage (gfdm_streamtile.h: the output tiles, step 1 and step 3) with tiles of kTile samples.
//   1. the halo: the input samples [i_lo - T - 7, i_hi + 7) -- the tile, its T past samples and up to seven more at either end for the runs
//      of step 2.  Sample k of the stage lies at xs[k + (k >> 3)]: the lanes of step 2 read samples 8 apart, which one padding sample per
//      eight spreads over all bank pairs (a stride of 18 dwords) where the plain layout would put sixteen lanes on one;
//   2. a lane owns one aligned RUN of eight absolute indices 8 r .. 8 r + 7: whatever offset and the alignment of `out` are, a tile meets at
//      most max_groups(kTile, 8) runs, which is why kTile is 2040 and not 2048.  Per path: for every sinusoid the phasor at 8 r (an integer
//      multiply, the top 24 bits through sincospif, the next 8 by a first-order correction, times A), the other seven by at most three fp32
//      rotations with exp(j 2 pi F m / 2^64), m = 1, 2, 4 (tables made at create in fp64); the delay line with a window of eight samples in
//      registers, one LDS read per tap for all eight; y += g * v.  The results go to a second LDS array in output format.
// The tables (48 bytes a sinusoid, P * T coefficients) go to LDS once per workgroup.  P, S and T are launch-uniform loop bounds.
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
#include "gfdm_streamtile.h"

#include <algorithm>
#include <cmath>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;

namespace {

constexpr int kLanes = 256;
constexpr int kMaxPaths = 8;
constexpr int kMaxSinusoids = 17;
constexpr int kMaxTaps = 64;
constexpr int kRun = 8;                   // absolute indices per run: one run a lane and tile
constexpr int kTile = 2040;               // samples per tile: a multiple of 4 whose runs fit kLanes
constexpr int kStage = kTile + kMaxTaps + 16;     // input samples in LDS
constexpr int kStagePad = kStage + kStage / 8 + 1;        // with one padding sample per eight
constexpr int kMaxTiles = 2048;           // workgroups per launch; the tiles beyond are strided over
static_assert(kTile % 4 == 0 && gfdm::max_groups(kTile, kRun) <= kLanes, "tile geometry");
static_assert(kStage % 2 == 0 && kStage >= gfdm::max_stage(kTile, kMaxTaps + kRun - 1, kRun - 1, 2), "the stage holds a tile's halo");

// one sinusoid as the kernel reads it: 48 bytes, three 16-byte LDS reads
struct Sinusoid {
    uint64_t F, Ph0;          // 2^-64 cycles per sample (two's complement), 2^-64 turns
    cf s1, s2, s4;            // exp(j 2 pi F m / 2^64) for m = 1, 2, 4: fp64 at create, rounded to fp32
    float A, pad;
};
static_assert(sizeof(Sinusoid) == 48, "table layout");
constexpr int kSinWords = (int)sizeof(Sinusoid) / 4;

struct FadeArgs {
    const cf* in;             // sample 0; `history` samples in front of it are readable
    const uint32_t* table;    // P * S Sinusoid, then P * T float
    int64_t n, history, offset;
    float gain;               // sc16
    int P, S, T;
};

__device__ __forceinline__ cf cmul(cf a, cf b)
{
    return make_float2(fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y));
}

constexpr int kPad = 3;                   // one padding sample per 2^kPad = kRun staged ones
__device__ __forceinline__ int padded(int k) { return gfdm::staged_at<kPad>(k); }

// A * exp(j 2 pi top / 2^32): the 24 bits nearest to `top` go through sincospif exactly (hi * 2^-23, in units of pi), the remainder r in
// [-128, 127] turns the result by delta = 2 pi r 2^-32 to first order (delta^2 / 2 < 2^-45)
__device__ __forceinline__ cf phasor(uint32_t top, float A)
{
    const uint32_t u = top + 128u;
    const int hi = (int)u >> 8;
    const float delta = (float)((int)(u & 255u) - 128) * 0x1.921fb6p-30f;        // 2 pi 2^-32
    float sn, cs;
    sincospif((float)hi * 0x1p-23f, &sn, &cs);
    return make_float2(A * fmaf(-sn, delta, cs), A * fmaf(cs, delta, sn));
}

// SC16 = 0: out is complex64; 1: interleaved int16 I/Q
template <int SC16>
__global__ __launch_bounds__(kLanes) void k_fade(FadeArgs a, void* __restrict__ out)
{
    constexpr int VPS = SC16 ? 4 : 2;            // samples per 16-byte vector
    __shared__ __attribute__((aligned(16))) cf xs[kStagePad];
    __shared__ __attribute__((aligned(16))) gfdm::stored_t<SC16> ys[kTile];
    __shared__ __attribute__((aligned(16))) uint32_t tab[kMaxPaths * kMaxSinusoids * kSinWords + kMaxPaths * kMaxTaps];
    const int nsin = a.P * a.S;
    for (int k = threadIdx.x; k < nsin * kSinWords + a.P * a.T; k += kLanes) tab[k] = a.table[k];
    const Sinusoid* const sins = reinterpret_cast<const Sinusoid*>(tab);
    const float* const coef = reinterpret_cast<const float*>(tab + nsin * kSinWords);
    // (the first barrier of the first tile stands between these writes and their readers)
    const gfdm::StreamTiles tiles(out, VPS, a.n, kTile / VPS);
    for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
        const gfdm::TileSpan t = tiles.tile(tile);
        const int64_t s0 = t.s0, i_lo = t.i_lo, i_hi = t.i_hi;                        // ys[k] is sample s0 + k
        // 1. sample j0 + k at xs[padded(k)] for j0 + k < i_hi + 7
        const int64_t j0 = gfdm::stage_first(a.in, i_lo - a.T - (kRun - 1));
        gfdm::stage_in<kPad>(xs, a.in, j0, (int)(i_hi + (kRun - 1) - j0), a.history, a.n, kLanes);
        __syncthreads();
        // 2. the runs of absolute indices that meet [i_lo, i_hi): at most max_groups(kTile, 8), one a lane
        const int64_t r_lo = (a.offset + i_lo) >> 3, r_hi = (a.offset + i_hi - 1) >> 3;
        if ((int64_t)threadIdx.x <= r_hi - r_lo) {
            const int64_t a0 = (r_lo + threadIdx.x) << 3, i0 = a0 - a.offset;        // samples i0 (>= i_lo - 7) .. i0 + 7 (<= i_hi + 6)
            const int b = (int)(i0 - j0);                                            // >= T: the stage holds sample i0 - t at b - t for t <= T
            cf y[kRun];
#pragma unroll
            for (int j = 0; j < kRun; ++j) y[j] = make_float2(0.f, 0.f);
#pragma unroll 1
            for (int p = 0; p < a.P; ++p) {
                // g[j] = sum_s A e(a0 + j), s ascending
                cf g[kRun];
#pragma unroll
                for (int j = 0; j < kRun; ++j) g[j] = make_float2(0.f, 0.f);
#pragma unroll 1
                for (int s = 0; s < a.S; ++s) {
                    const Sinusoid w = sins[p * a.S + s];
                    const uint64_t phi = w.F * (uint64_t)a0 + w.Ph0;
                    cf e[kRun];
                    e[0] = phasor((uint32_t)(phi >> 32), w.A);
                    e[1] = cmul(e[0], w.s1);
                    e[2] = cmul(e[0], w.s2);
                    e[3] = cmul(e[2], w.s1);
                    e[4] = cmul(e[0], w.s4);
                    e[5] = cmul(e[4], w.s1);
                    e[6] = cmul(e[4], w.s2);
                    e[7] = cmul(e[6], w.s1);
#pragma unroll
                    for (int j = 0; j < kRun; ++j) g[j] = make_float2(g[j].x + e[j].x, g[j].y + e[j].y);
                }
                // v[j] = sum_k c[k] x[i0 + j - k], k ascending: win[(j - k) & 7] is x[i0 + j - k] while tap k is at work
                cf v[kRun], win[kRun];
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    v[j] = make_float2(0.f, 0.f);
                    win[j] = xs[padded(b + j)];
                }
                const float* const c = coef + p * a.T;
                // whole blocks of eight taps without a branch, then the T % 8 that are left; the slot of x[i0 + 7 - k], which has had its
                // last tap, takes x[i0 - k - 1] for the next one (behind the last tap that is xs[b - T]: staged, not used)
                int k0 = 0;
#pragma unroll 1
                for (; k0 + kRun <= a.T; k0 += kRun) {
#pragma unroll
                    for (int kk = 0; kk < kRun; ++kk) {
                        const float ck = c[k0 + kk];
#pragma unroll
                        for (int j = 0; j < kRun; ++j) {
                            v[j].x = fmaf(ck, win[(j - kk) & 7].x, v[j].x);
                            v[j].y = fmaf(ck, win[(j - kk) & 7].y, v[j].y);
                        }
                        win[(7 - kk) & 7] = xs[padded(b - k0 - kk - 1)];
                    }
                }
#pragma unroll
                for (int kk = 0; kk < kRun - 1; ++kk) {
                    if (k0 + kk < a.T) {
                        const float ck = c[k0 + kk];
#pragma unroll
                        for (int j = 0; j < kRun; ++j) {
                            v[j].x = fmaf(ck, win[(j - kk) & 7].x, v[j].x);
                            v[j].y = fmaf(ck, win[(j - kk) & 7].y, v[j].y);
                        }
                        win[(7 - kk) & 7] = xs[padded(b - k0 - kk - 1)];
                    }
                }
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    y[j].x = fmaf(-g[j].y, v[j].y, fmaf(g[j].x, v[j].x, y[j].x));
                    y[j].y = fmaf(g[j].y, v[j].x, fmaf(g[j].x, v[j].y, y[j].y));
                }
            }
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                const int64_t i = i0 + j;
                if (i >= i_lo && i < i_hi) ys[i - s0] = gfdm::to_stored<SC16>(y[j], a.gain);
            }
        }
        __syncthreads();
        // 3.
        gfdm::store_tile<SC16>(static_cast<unsigned char*>(out), tiles, t, ys, kLanes);
        // (xs is rewritten only behind the barrier above, which every lane passes after step 2; ys is read here and rewritten behind the next tile's first barrier)
    }
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int fading_check(int n_paths, int n_sinusoids, int n_taps, int64_t n, int64_t history, int64_t offset, double gain)
{
    if (n_paths < 1 || n_paths > kMaxPaths) return api_fail(GFDM_HIP_EINVAL, "n_paths must lie in 1 .. 8");
    if (n_sinusoids < 1 || n_sinusoids > kMaxSinusoids) return api_fail(GFDM_HIP_EINVAL, "n_sinusoids must lie in 1 .. 17");
    if (n_taps < 1 || n_taps > kMaxTaps) return api_fail(GFDM_HIP_EINVAL, "n_taps must lie in 1 .. 64");
    if (!std::isfinite(gain)) return api_fail(GFDM_HIP_EINVAL, "gain must be finite");
    return gfdm::check_stream_span(n, history, offset);
}

// exp(j 2 pi w / 2^64) of a 64-bit phase, in fp64, rounded to fp32
cf turn(uint64_t w)
{
    const double t = 6.283185307179586476925 * ((double)(int64_t)w * 0x1p-64);
    return make_float2((float)std::cos(t), (float)std::sin(t));
}

}  // namespace

struct gfdm_hip_fading_model {
    gfdm::DeviceCtx ctx;
    int P = 0, S = 0, T = 0;
    std::vector<float> c, A;
    std::vector<int64_t> F;
    std::vector<uint64_t> Ph0;
    uint32_t* d_table = nullptr;
    ~gfdm_hip_fading_model()
    {
        if (!d_table) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(d_table);
    }
};

namespace {

int check_call(const gfdm_hip_fading_model* h, const void* out, const void* in, int sc16, int64_t n, int64_t history, int64_t offset, double gain)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = fading_check(h->P, h->S, h->T, n, history, offset, gain);
    if (rc != GFDM_HIP_OK) return rc;
    if (n == 0) return GFDM_HIP_OK;
    if (!out || !in) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return gfdm::check_no_overlap(out, sc16 ? 4 : 8, n, in, sizeof(cf), n, history, "n", "the fading model");       // the delay lines read neighbours
}

// the one launch of a call; out and in are device pointers
int fading_enqueue(const gfdm_hip_fading_model* h, int sc16, void* out, const cf* in, int64_t n, int64_t history, int64_t offset, double gain, hipStream_t s)
{
    if (n == 0) return GFDM_HIP_OK;
    const int rc = gfdm::check_sample_alignment(out, sc16 ? 4 : 8, in, sizeof(cf));
    if (rc != GFDM_HIP_OK) return rc;
    FadeArgs a;
    a.in = in;
    a.table = h->d_table;
    a.n = n;
    a.history = history;
    a.offset = offset;
    a.gain = (float)gain;
    a.P = h->P;
    a.S = h->S;
    a.T = h->T;
    const int vps = sc16 ? 4 : 2;
    const dim3 grid((unsigned)std::min<int64_t>(gfdm::StreamTiles(out, vps, n, kTile / vps).ntiles, kMaxTiles));
    if (sc16) hipLaunchKernelGGL(k_fade<1>, grid, dim3(kLanes), 0, s, a, out);
    else hipLaunchKernelGGL(k_fade<0>, grid, dim3(kLanes), 0, s, a, out);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// check_call, then fading_enqueue: on the caller's stream, or between an upload and a download on the handle's (gfdm::stream_call)
int fading_call(gfdm_hip_fading_model* h, bool host, int sc16, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain, void* stream)
{
    return gfdm::stream_call(h, host, sc16, out, in, n, history, offset, gain, stream, check_call, fading_enqueue);
}

template <class V, class E>
int read_table(const gfdm_hip_fading_model* h, const V& table, E* to)
{
    if (!h || !to) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    std::copy(table.begin(), table.end(), to);
    return GFDM_HIP_OK;
}

}  // namespace

extern "C" {

int gfdm_hip_fading_model_create(gfdm_hip_fading_model** out, const float* c, const float* A, const int64_t* F, const uint64_t* Ph0, int n_paths,
                                 int n_sinusoids, int n_taps, int device)
{
    return gfdm::create_handle(
        out, device,
        [&](gfdm_hip_fading_model& h) -> int {
            const int rc = fading_check(n_paths, n_sinusoids, n_taps, 0, 0, 0, 1.0);
            if (rc != GFDM_HIP_OK) return rc;
            if (!c || !A || !F || !Ph0) return api_fail(GFDM_HIP_EINVAL, "NULL table");
            const int nc = n_paths * n_taps, ns = n_paths * n_sinusoids;
            for (int i = 0; i < nc; ++i)
                if (!std::isfinite(c[i])) return api_fail(GFDM_HIP_EINVAL, "the coefficients c must be finite");
            for (int i = 0; i < ns; ++i)
                if (!std::isfinite(A[i])) return api_fail(GFDM_HIP_EINVAL, "the amplitudes A must be finite");
            h.P = n_paths;
            h.S = n_sinusoids;
            h.T = n_taps;
            h.c.assign(c, c + nc);
            h.A.assign(A, A + ns);
            h.F.assign(F, F + ns);
            h.Ph0.assign(Ph0, Ph0 + ns);
            return GFDM_HIP_OK;
        },
        [&](gfdm_hip_fading_model& h) -> int {
            const int ns = h.P * h.S, nc = h.P * h.T;
            std::vector<uint32_t> words((size_t)ns * kSinWords + nc, 0u);
            Sinusoid* const sins = reinterpret_cast<Sinusoid*>(words.data());
            for (int i = 0; i < ns; ++i) {
                const uint64_t f = (uint64_t)h.F[i];
                sins[i].F = f;
                sins[i].Ph0 = h.Ph0[i];
                sins[i].s1 = turn(f);
                sins[i].s2 = turn(2 * f);
                sins[i].s4 = turn(4 * f);
                sins[i].A = h.A[i];
                sins[i].pad = 0.f;
            }
            std::copy(h.c.begin(), h.c.end(), reinterpret_cast<float*>(words.data() + (size_t)ns * kSinWords));
            const size_t bytes = words.size() * sizeof(uint32_t);
            hipError_t e = hipMalloc(&h.d_table, bytes);
            if (e == hipSuccess) e = hipMemcpy(h.d_table, words.data(), bytes, hipMemcpyHostToDevice);
            return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "fading model table upload");
        });
}

int gfdm_hip_fading_model_destroy(gfdm_hip_fading_model* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_fading_model_n_paths(const gfdm_hip_fading_model* h) { return h ? h->P : GFDM_HIP_EINVAL; }
int gfdm_hip_fading_model_n_sinusoids(const gfdm_hip_fading_model* h) { return h ? h->S : GFDM_HIP_EINVAL; }
int gfdm_hip_fading_model_n_taps(const gfdm_hip_fading_model* h) { return h ? h->T : GFDM_HIP_EINVAL; }
int gfdm_hip_fading_model_taps(const gfdm_hip_fading_model* h, float* c) { return read_table(h, h ? h->c : std::vector<float>(), c); }
int gfdm_hip_fading_model_amplitudes(const gfdm_hip_fading_model* h, float* A) { return read_table(h, h ? h->A : std::vector<float>(), A); }
int gfdm_hip_fading_model_frequencies(const gfdm_hip_fading_model* h, int64_t* F) { return read_table(h, h ? h->F : std::vector<int64_t>(), F); }
int gfdm_hip_fading_model_phases(const gfdm_hip_fading_model* h, uint64_t* Ph0) { return read_table(h, h ? h->Ph0 : std::vector<uint64_t>(), Ph0); }

int gfdm_hip_fading_model_check(int n_paths, int n_sinusoids, int n_taps, int64_t n, int64_t history, int64_t offset, double gain)
{
    return fading_check(n_paths, n_sinusoids, n_taps, n, history, offset, gain);
}

int gfdm_hip_fading_model_apply_device(gfdm_hip_fading_model* h, void* out, const void* in, int64_t n, int64_t history, int64_t offset, void* stream)
{
    return fading_call(h, false, 0, out, in, n, history, offset, 1.0, stream);
}
int gfdm_hip_fading_model_apply_sc16_device(gfdm_hip_fading_model* h, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain,
                                            void* stream)
{
    return fading_call(h, false, 1, out, in, n, history, offset, gain, stream);
}
int gfdm_hip_fading_model_apply_host(gfdm_hip_fading_model* h, float* out, const float* in, int64_t n, int64_t history, int64_t offset)
{
    return fading_call(h, true, 0, out, in, n, history, offset, 1.0, nullptr);
}
int gfdm_hip_fading_model_apply_sc16_host(gfdm_hip_fading_model* h, int16_t* out, const float* in, int64_t n, int64_t history, int64_t offset, double gain)
{
    return fading_call(h, true, 1, out, in, n, history, offset, gain, nullptr);
}

}  // extern "C"
