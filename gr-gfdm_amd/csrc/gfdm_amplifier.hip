// Amplifier model between the burst shaper (or the resampler) and the fading / channel model: the transmitter's power amplifier on a
// continuous stream, complex64 or interleaved int16 I/Q out.  Four kinds, fixed at create: a hard clipper, Rapp's solid-state AM/AM curve,
// Saleh's travelling-wave-tube AM/AM + AM/PM curves and a memory polynomial of odd orders.  The contract is written out in
// include/gfdm_hip.h.
//
// One kernel, k_amplify<KIND, SC16>, a stream stage (gfdm_streamtile.h: the output tiles, step 1 and step 3) with tiles of kTile samples.
//   CLIP, RAPP, SALEH (memoryless): no halo and no LDS.  A lane takes one 16-byte output vector at a time: its 2 (sc16: 4) input samples in
//      16-byte loads where the vector lies in the stream as a whole and `in` is 16-byte aligned under it, else in 8-byte loads, one a
//      sample (the two ends of a stream, and every vector where `in` and `out` differ in alignment); amp_sample; store_vector.
//   POLY: as k_channel.  1. the halo: the input samples [i_lo - (Q - 1), i_hi) go to LDS;  2. a lane owns the samples kLanes apart (LDS
//      reads of neighbouring lanes are neighbours: no bank conflict), per delay q one LDS read, u = d x, r = |u|^2, Horner for
//      G_q(r) = sum_k c[q][k] r^k, y += G_q u; the results go to a second LDS array in output format;  3. store_tile.
// A sample's arithmetic is one function of its input samples (amp_sample, poly_sample, contraction off, every fma written out), so it does
// not depend on the tile, the lane, the load path or the call it falls into.  Q, K and the all-real-coefficients case are launch-uniform
// branches; the coefficients are kernel arguments.
//
// hipcc -O3 --offload-arch=gfx950 (ROCm 7.x), -Rpass-analysis=kernel-resource-usage, VGPRs / scratch bytes / LDS bytes:
//   k_amplify<CLIP, 0> 30 / 0 / 0       k_amplify<CLIP, 1> 35 / 0 / 0
//   k_amplify<RAPP, 0> 44 / 0 / 0       k_amplify<RAPP, 1> 53 / 0 / 0
//   k_amplify<SALEH, 0> 52 / 0 / 0      k_amplify<SALEH, 1> 67 / 0 / 0
//   k_amplify<POLY, 0> 32 / 0 / 32896   k_amplify<POLY, 1> 34 / 0 / 24704
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
#include "gfdm_streamtile.h"

#include <algorithm>
#include <cmath>

using gfdm::cf;
using gfdm::api_fail;

namespace {

constexpr int kLanes = 256;
constexpr int kMaxDelays = 16;            // Q
constexpr int kMaxOrders = 5;             // K: the odd orders 1, 3, .. 2 K - 1
constexpr int kMaxParams = 4;
constexpr int kTile = 2048;               // samples per tile
constexpr int kPerLane = kTile / kLanes;  // POLY: samples a lane and tile
constexpr int kStage = kTile + kMaxDelays;        // POLY: input samples in LDS
constexpr int kMaxTiles = 2048;           // workgroups per launch; the tiles beyond are strided over
static_assert(kTile % 4 == 0 && kTile % kLanes == 0, "tile geometry");
static_assert(kStage % 2 == 0 && kStage >= gfdm::max_stage(kTile, kMaxDelays - 1, 0, 2), "the stage holds a tile's halo");

constexpr int CLIP = GFDM_HIP_AMPLIFIER_CLIP, RAPP = GFDM_HIP_AMPLIFIER_RAPP, SALEH = GFDM_HIP_AMPLIFIER_SALEH, POLY = GFDM_HIP_AMPLIFIER_POLY;

struct AmpArgs {
    const cf* in;            // sample 0; `history` samples in front of it are readable
    int64_t n, history;
    float drive;             // d
    float gain;              // sc16
    // CLIP: A, A^2.  RAPP: g, A, p, g^2 / A^2, 1 / (2 p).  SALEH: aa, ba, ap, bp.
    float p[5];
    int Q, K;
    int real_coef;           // every coefficient has imaginary part 0: the products with it are left out
    cf c[kMaxDelays * kMaxOrders];      // c[q * K + k]
};

// the memoryless kinds: y of one input sample
template <int KIND>
__device__ __forceinline__ cf amp_sample(const AmpArgs& a, cf x)
{
#pragma clang fp contract(off)
    const cf u = make_float2(a.drive * x.x, a.drive * x.y);
    const float r = fmaf(u.x, u.x, u.y * u.y);
    if constexpr (KIND == CLIP) {
        if (r <= a.p[1]) return u;
        const float s = a.p[0] / sqrtf(r);
        return make_float2(u.x * s, u.y * s);
    } else if constexpr (KIND == RAPP) {
        // t^p overflows long before r does: beyond t = 1 the curve is taken from its saturated end, g u / sqrt t = A u / sqrt r
        const float t = a.p[3] * r;
        float s;
        if (t <= 1.f) s = a.p[0] * powf(1.f + powf(t, a.p[2]), -a.p[4]);
        else s = (a.p[1] / sqrtf(r)) * powf(1.f + powf(t, -a.p[2]), -a.p[4]);
        return make_float2(u.x * s, u.y * s);
    } else {
        const float am = a.p[0] / fmaf(a.p[1], r, 1.f);
        const float ph = (a.p[2] * r) / fmaf(a.p[3], r, 1.f);
        float sn, cs;
        sincosf(ph, &sn, &cs);
        const cf v = make_float2(u.x * am, u.y * am);
        return make_float2(fmaf(-v.y, sn, v.x * cs), fmaf(v.y, cs, v.x * sn));
    }
}

// POLY: y[i] from the staged samples, x[i - q] at xs[k - q].  q ascending, Horner from the highest order down: the same chain for every i
template <bool REAL>
__device__ __forceinline__ cf poly_sample(const AmpArgs& a, const cf* xs, int k)
{
#pragma clang fp contract(off)
    cf y = make_float2(0.f, 0.f);
    for (int q = 0; q < a.Q; ++q) {
        const cf x = xs[k - q];
        const cf u = make_float2(a.drive * x.x, a.drive * x.y);
        const float r = fmaf(u.x, u.x, u.y * u.y);
        const cf* const c = a.c + q * a.K;
        cf g = c[a.K - 1];
        for (int o = a.K - 2; o >= 0; --o) {
            g.x = fmaf(g.x, r, c[o].x);
            if (!REAL) g.y = fmaf(g.y, r, c[o].y);
        }
        y.x = fmaf(g.x, u.x, y.x);
        y.y = fmaf(g.x, u.y, y.y);
        if (!REAL) {
            y.x = fmaf(-g.y, u.y, y.x);
            y.y = fmaf(g.y, u.x, y.y);
        }
    }
    return y;
}

// SC16 = 0: out is complex64; 1: interleaved int16 I/Q
template <int KIND, int SC16>
__global__ __launch_bounds__(kLanes) void k_amplify(AmpArgs a, void* __restrict__ out)
{
    constexpr int VPS = SC16 ? 4 : 2;            // samples per 16-byte vector
    const gfdm::StreamTiles tiles(out, VPS, a.n, kTile / VPS);
    if constexpr (KIND != POLY) {
        const bool in_odd = (((uintptr_t)a.in / 8) & 1) != 0;
        for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
            const gfdm::TileSpan t = tiles.tile(tile);
#pragma unroll 2
            for (int64_t v = t.v0 + threadIdx.x; v < t.v1; v += kLanes) {
                const int64_t i0 = tiles.first(v);
                cf x[VPS];
                if (tiles.whole(i0) && (((i0 & 1) != 0) == in_odd)) {            // in + i0 is 16-byte aligned
#pragma unroll
                    for (int j = 0; j < VPS; j += 2) {
                        const float4 x2 = *reinterpret_cast<const float4*>(a.in + i0 + j);
                        x[j] = make_float2(x2.x, x2.y);
                        x[j + 1] = make_float2(x2.z, x2.w);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < VPS; ++j) x[j] = (i0 + j >= 0 && i0 + j < a.n) ? a.in[i0 + j] : make_float2(0.f, 0.f);
                }
                cf y[VPS];
#pragma unroll
                for (int j = 0; j < VPS; ++j) y[j] = amp_sample<KIND>(a, x[j]);
                gfdm::store_vector<SC16>(static_cast<unsigned char*>(out), tiles, i0, y, a.gain);
            }
        }
    } else {
        __shared__ __attribute__((aligned(16))) cf xs[kStage];
        __shared__ __attribute__((aligned(16))) gfdm::stored_t<SC16> ys[kTile];
        for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
            const gfdm::TileSpan t = tiles.tile(tile);
            const int64_t s0 = t.s0, i_lo = t.i_lo, i_hi = t.i_hi;                        // ys[k] is sample s0 + k
            // 1. xs[k] = x[j0 + k] for j0 + k < i_hi
            const int64_t j0 = gfdm::stage_first(a.in, i_lo - (a.Q - 1));
            gfdm::stage_in<0>(xs, a.in, j0, (int)(i_hi - j0), a.history, a.n, kLanes);
            __syncthreads();
            // 2. sample i_lo + u * kLanes + lane: xs[i - j0 - q] lies inside for q < Q, as i - (Q - 1) >= i_lo - (Q - 1) >= j0
            const int count = (int)(i_hi - i_lo);
#pragma unroll 1
            for (int u = 0; u < kPerLane; ++u) {
                const int m = u * kLanes + threadIdx.x;
                if (m >= count) break;
                const int64_t i = i_lo + m;
                const cf y = a.real_coef ? poly_sample<true>(a, xs, (int)(i - j0)) : poly_sample<false>(a, xs, (int)(i - j0));
                ys[i - s0] = gfdm::to_stored<SC16>(y, a.gain);
            }
            __syncthreads();
            // 3.
            gfdm::store_tile<SC16>(static_cast<unsigned char*>(out), tiles, t, ys, kLanes);
            // (xs is rewritten only behind the barrier above, which every lane passes after step 2; ys is read here and rewritten behind the next tile's first barrier)
        }
    }
}

int bad(const char* msg) { return api_fail(GFDM_HIP_EINVAL, msg); }

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int amplifier_check(int kind, const double* params, int n_params, int n_delays, int n_orders, double drive, int64_t n, int64_t history, double gain)
{
    if (kind < CLIP || kind > POLY) return bad("kind must be one of CLIP, RAPP, SALEH, POLY");
    const int want = kind == CLIP ? 1 : kind == RAPP ? 3 : kind == SALEH ? 4 : 0;
    if (n_params != want) return bad("n_params must be 1 (CLIP: A), 3 (RAPP: g, A, p), 4 (SALEH: aa, ba, ap, bp) or 0 (POLY)");
    if (want && !params) return bad("NULL params");
    for (int i = 0; i < n_params; ++i)
        if (!std::isfinite(params[i]) || !std::isfinite((float)params[i])) return bad("params must be finite (in fp32)");
    if (kind == CLIP && !((float)params[0] > 0.f)) return bad("A must be > 0");
    if (kind == RAPP) {
        if (!((float)params[0] > 0.f)) return bad("g must be > 0");
        if (!((float)params[1] > 0.f)) return bad("A must be > 0");
        if (!(params[2] >= 0.5 && params[2] <= 16.0)) return bad("p must lie in 0.5 .. 16");
        // the constant of t = fl32(g^2 / A^2) * r, from the fp32 values: 0 or inf there would leave no curve (and inf * 0 at r = 0)
        const double g = (double)(float)params[0], A = (double)(float)params[1];
        const float ratio = (float)((g * g) / (A * A));
        if (!std::isfinite(ratio) || !(ratio > 0.f)) return bad("g^2 / A^2 must be finite and > 0 in fp32");
    }
    if (kind == SALEH) {
        if (params[1] < 0.0) return bad("ba must be >= 0");
        if (params[3] < 0.0) return bad("bp must be >= 0");
    }
    if (kind == POLY) {
        if (n_delays < 1 || n_delays > kMaxDelays) return bad("n_delays must lie in 1 .. 16");
        if (n_orders < 1 || n_orders > kMaxOrders) return bad("n_orders must lie in 1 .. 5");
    } else if (n_delays != 0 || n_orders != 0) {
        return bad("n_delays and n_orders must be 0 for a kind without coefficients");
    }
    if (!std::isfinite(drive) || drive < 0.0 || !std::isfinite((float)drive)) return bad("drive must be finite (in fp32) and >= 0");
    if (!std::isfinite(gain)) return bad("gain must be finite");
    // check_stream_span without an offset, in this stage's words
    if (n < 0) return bad("n must be >= 0");
    if (history < 0) return bad("history must be >= 0");
    if (n > ((int64_t)1 << 62)) return bad("n must not exceed 2^62");
    const int64_t lim = INT64_MAX / (int64_t)sizeof(cf);
    if (n > lim || history > lim - n) return bad("the byte size of the input overflows int64");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_amplifier_model {
    gfdm::DeviceCtx ctx;
    int kind = CLIP;
    int n_params = 0;
    double params[kMaxParams] = {};       // as rounded to fp32
    int Q = 0, K = 0;
    int real_coef = 1;
    cf c[kMaxDelays * kMaxOrders] = {};
    double drive = 1.0;
};

namespace {

int check_call(const gfdm_hip_amplifier_model* h, const void* out, const void* in, int sc16, int64_t n, int64_t history, int64_t, double gain)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = amplifier_check(h->kind, h->params, h->n_params, h->Q, h->K, h->drive, n, history, gain);
    if (rc != GFDM_HIP_OK) return rc;
    if (n == 0) return GFDM_HIP_OK;
    if (!out || !in) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return gfdm::check_no_overlap(out, sc16 ? 4 : 8, n, in, sizeof(cf), n, history, "n", "the amplifier model");
}

template <int KIND>
void launch(int sc16, dim3 grid, hipStream_t s, const AmpArgs& a, void* out)
{
    if (sc16) hipLaunchKernelGGL((k_amplify<KIND, 1>), grid, dim3(kLanes), 0, s, a, out);
    else hipLaunchKernelGGL((k_amplify<KIND, 0>), grid, dim3(kLanes), 0, s, a, out);
}

// the one launch of a call; out and in are device pointers, the handle's drive is read here
int amplifier_enqueue(const gfdm_hip_amplifier_model* h, int sc16, void* out, const cf* in, int64_t n, int64_t history, int64_t, double gain, hipStream_t s)
{
    if (n == 0) return GFDM_HIP_OK;
    const int rc = gfdm::check_sample_alignment(out, sc16 ? 4 : 8, in, sizeof(cf));
    if (rc != GFDM_HIP_OK) return rc;
    AmpArgs a;
    a.in = in;
    a.n = n;
    a.history = history;
    a.drive = (float)h->drive;
    a.gain = (float)gain;
    for (float& v : a.p) v = 0.f;
    const double* const p = h->params;
    if (h->kind == CLIP) {
        a.p[0] = (float)p[0];
        a.p[1] = (float)(p[0] * p[0]);
    } else if (h->kind == RAPP) {
        a.p[0] = (float)p[0];
        a.p[1] = (float)p[1];
        a.p[2] = (float)p[2];
        a.p[3] = (float)((p[0] * p[0]) / (p[1] * p[1]));
        a.p[4] = (float)(1.0 / (2.0 * p[2]));
    } else if (h->kind == SALEH) {
        for (int i = 0; i < 4; ++i) a.p[i] = (float)p[i];
    }
    a.Q = h->Q;
    a.K = h->K;
    a.real_coef = h->real_coef;
    std::copy(h->c, h->c + kMaxDelays * kMaxOrders, a.c);
    const int vps = sc16 ? 4 : 2;
    const dim3 grid((unsigned)std::min<int64_t>(gfdm::StreamTiles(out, vps, n, kTile / vps).ntiles, kMaxTiles));
    switch (h->kind) {
    case CLIP: launch<CLIP>(sc16, grid, s, a, out); break;
    case RAPP: launch<RAPP>(sc16, grid, s, a, out); break;
    case SALEH: launch<SALEH>(sc16, grid, s, a, out); break;
    default: launch<POLY>(sc16, grid, s, a, out); break;
    }
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// check_call, then amplifier_enqueue: on the caller's stream, or between an upload and a download on the handle's (gfdm::stream_call)
int amplifier_call(gfdm_hip_amplifier_model* h, bool host, int sc16, void* out, const void* in, int64_t n, int64_t history, double gain, void* stream)
{
    return gfdm::stream_call(h, host, sc16, out, in, n, history, (int64_t)0, gain, stream, check_call, amplifier_enqueue);
}

}  // namespace

extern "C" {

int gfdm_hip_amplifier_model_create(gfdm_hip_amplifier_model** out, int kind, const double* params, int n_params, const float* coefficients, int n_delays,
                                    int n_orders, double drive, int device)
{
    return gfdm::create_handle(out, device, [&](gfdm_hip_amplifier_model& h) -> int {
        const int rc = amplifier_check(kind, params, n_params, n_delays, n_orders, drive, 0, 0, 1.0);
        if (rc != GFDM_HIP_OK) return rc;
        h.kind = kind;
        h.n_params = n_params;
        for (int i = 0; i < n_params; ++i) h.params[i] = (double)(float)params[i];
        if (kind == POLY) {
            if (!coefficients) return api_fail(GFDM_HIP_EINVAL, "NULL coefficients");
            for (int i = 0; i < 2 * n_delays * n_orders; ++i)
                if (!std::isfinite(coefficients[i])) return api_fail(GFDM_HIP_EINVAL, "the coefficients must be finite");
            h.Q = n_delays;
            h.K = n_orders;
            for (int i = 0; i < n_delays * n_orders; ++i) {
                h.c[i] = make_float2(coefficients[2 * i], coefficients[2 * i + 1]);
                if (coefficients[2 * i + 1] != 0.f) h.real_coef = 0;
            }
        }
        h.drive = drive;
        return GFDM_HIP_OK;
    });
}

int gfdm_hip_amplifier_model_destroy(gfdm_hip_amplifier_model* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_amplifier_model_kind(const gfdm_hip_amplifier_model* h) { return h ? h->kind : GFDM_HIP_EINVAL; }
int gfdm_hip_amplifier_model_n_params(const gfdm_hip_amplifier_model* h) { return h ? h->n_params : GFDM_HIP_EINVAL; }
int gfdm_hip_amplifier_model_n_delays(const gfdm_hip_amplifier_model* h) { return h ? h->Q : GFDM_HIP_EINVAL; }
int gfdm_hip_amplifier_model_n_orders(const gfdm_hip_amplifier_model* h) { return h ? h->K : GFDM_HIP_EINVAL; }
int gfdm_hip_amplifier_model_params(const gfdm_hip_amplifier_model* h, double* params)
{
    if (!h || !params) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    std::copy(h->params, h->params + h->n_params, params);
    return GFDM_HIP_OK;
}
int gfdm_hip_amplifier_model_coefficients(const gfdm_hip_amplifier_model* h, float* coefficients)
{
    if (!h || !coefficients) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    for (int i = 0; i < h->Q * h->K; ++i) {
        coefficients[2 * i] = h->c[i].x;
        coefficients[2 * i + 1] = h->c[i].y;
    }
    return GFDM_HIP_OK;
}
int gfdm_hip_amplifier_model_drive(const gfdm_hip_amplifier_model* h, double* drive)
{
    if (!h || !drive) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    *drive = h->drive;
    return GFDM_HIP_OK;
}
int gfdm_hip_amplifier_model_set_drive(gfdm_hip_amplifier_model* h, double drive)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = amplifier_check(h->kind, h->params, h->n_params, h->Q, h->K, drive, 0, 0, 1.0);
    if (rc == GFDM_HIP_OK) h->drive = drive;
    return rc;
}

int gfdm_hip_amplifier_model_check(int kind, const double* params, int n_params, int n_delays, int n_orders, double drive, int64_t n, int64_t history,
                                   double gain)
{
    return amplifier_check(kind, params, n_params, n_delays, n_orders, drive, n, history, gain);
}

int gfdm_hip_amplifier_model_apply_device(gfdm_hip_amplifier_model* h, void* out, const void* in, int64_t n, int64_t history, void* stream)
{
    return amplifier_call(h, false, 0, out, in, n, history, 1.0, stream);
}
int gfdm_hip_amplifier_model_apply_sc16_device(gfdm_hip_amplifier_model* h, void* out, const void* in, int64_t n, int64_t history, double gain, void* stream)
{
    return amplifier_call(h, false, 1, out, in, n, history, gain, stream);
}
int gfdm_hip_amplifier_model_apply_host(gfdm_hip_amplifier_model* h, float* out, const float* in, int64_t n, int64_t history)
{
    return amplifier_call(h, true, 0, out, in, n, history, 1.0, nullptr);
}
int gfdm_hip_amplifier_model_apply_sc16_host(gfdm_hip_amplifier_model* h, int16_t* out, const float* in, int64_t n, int64_t history, double gain)
{
    return amplifier_call(h, true, 1, out, in, n, history, gain, nullptr);
}

}  // extern "C"
