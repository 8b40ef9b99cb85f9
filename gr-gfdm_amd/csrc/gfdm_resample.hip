// Fractional-rate resampler between the burst shaper and the channel model, and between a capture at a radio's rate and the synchroniser:
// a polyphase interpolator on a continuous stream, complex64 or interleaved int16 I/Q in, complex64 out (the work of GNU Radio's
// mmse_resampler_cc / pfb_arb_resampler_ccf, and of the resampler that channels.channel_model drives with epsilon).  The contract is
// written out in include/gfdm_hip.h.
//
// One kernel, k_resample<SC16, INTERP, T>, a stream stage (gfdm_streamtile.h: the output tiles, step 1 of a complex64 input and the
// store of step 3) whose tile size is a run-time value: the host chooses tile_vec from `step` so that the input span of a tile, which
// grows with step, fits kStage samples.  Per workgroup the tap table goes to LDS once (rows padded to an odd stride: lanes on different
// rows then meet different banks); per tile
//   1. the halo: the input samples [idx(first) - D, idx(last) - D + T); an sc16 input in one 4-byte load per sample, widened there;
//   2. a lane owns output vectors: two consecutive samples, each with its own position P = pos + i * step (mul-hi / mul-lo, no float),
//      its own row(s) of the table and its own window of the staged span; the vector leaves from registers.
// In interp 1 the difference h[q + 1][t] - h[q][t] is formed from the two rows in LDS: the same single fp32 rounding as a table made at
// create, at half the LDS footprint, so every (L, T) of the contract takes this one path (at most 53.8 KB of LDS:
// 16 928 bytes of samples and the 1025 x 9 floats of L = 1024, T = 8).
#include "../../include/gfdm_hip.h"
#include "gfdm_burstfetch.h"
#include "gfdm_hostcall.h"
#include "gfdm_streamtile.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;

namespace {

typedef unsigned __int128 u128;

constexpr int kLanes = 256;
constexpr int kMaxTaps = 64;
constexpr int kMaxPhases = 1024;
constexpr int kMaxTable = 8256;              // (L + 1) * T: 129 rows of 64, 1025 rows of 8
constexpr int kTileVecMax = 1024;            // output vectors per tile: four a lane
constexpr int kStage = 2 * kTileVecMax + kMaxTaps + 4;      // input samples in LDS; even
constexpr int kMaxGroups = 2048;             // workgroups per launch; the tiles beyond are strided over
constexpr uint64_t kStepMin = (uint64_t)1 << 29, kStepMax = (uint64_t)1 << 35;
constexpr int64_t kMaxPos = (int64_t)1 << 62;
static_assert(kStage % 2 == 0, "the staging loop stores pairs");

struct ResampleArgs {
    const void* in;          // sample 0; `history` samples in front of it are readable
    const float* table;      // (L + 1) * T floats on the device
    int64_t n_out, n_in, history;
    uint64_t pos, step;
    int T, L, lg;
    int tile_vec;            // output vectors per tile
};

// P(i) = pos + i * step as (idx, frac): i < 2^60, step <= 2^35, P < 2^94
__device__ __forceinline__ void position(const ResampleArgs& a, int64_t i, int64_t& idx, uint32_t& frac)
{
    const uint64_t lo = (uint64_t)i * a.step, hi = __umul64hi((uint64_t)i, a.step);
    const uint64_t s = lo + a.pos;
    const uint64_t h = hi + (s < lo ? 1u : 0u);
    idx = (int64_t)((h << 32) | (s >> 32));
    frac = (uint32_t)s;
}

// y[i]: x = the staged span from sample idx - D on, hs the table in LDS with row stride TS
template <int INTERP>
__device__ __forceinline__ cf output(const cf* x, const float* hs, uint32_t frac, int lg, int T, int TS)
{
    cf y;
    if (INTERP) {
        const uint32_t q = (uint32_t)((uint64_t)frac >> (32 - lg));
        const float w = (float)((uint32_t)(frac << lg) >> 8) * 0x1p-24f;
        const float* h0 = hs + q * TS;
        const float* h1 = h0 + TS;
        float c = fmaf(w, h1[0] - h0[0], h0[0]);
        y = make_float2(c * x[0].x, c * x[0].y);
#pragma unroll 8
        for (int t = 1; t < T; ++t) {
            c = fmaf(w, h1[t] - h0[t], h0[t]);
            y.x = fmaf(c, x[t].x, y.x);
            y.y = fmaf(c, x[t].y, y.y);
        }
    } else {
        const uint32_t p = (uint32_t)(((uint64_t)frac + ((uint64_t)1 << (31 - lg))) >> (32 - lg));
        const float* h0 = hs + p * TS;
        y = make_float2(h0[0] * x[0].x, h0[0] * x[0].y);
#pragma unroll 8
        for (int t = 1; t < T; ++t) {
            y.x = fmaf(h0[t], x[t].x, y.x);
            y.y = fmaf(h0[t], x[t].y, y.y);
        }
    }
    return y;
}

// SC16 = 0: in is complex64; 1: interleaved int16 I/Q.  TT: n_taps at compile time, 0 = a.T
template <int SC16, int INTERP, int TT>
__global__ __launch_bounds__(kLanes) void k_resample(ResampleArgs a, cf* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    cf* const xs = reinterpret_cast<cf*>(lds);                                      // kStage samples
    float* const hs = reinterpret_cast<float*>(lds + kStage * sizeof(cf));          // (L + 1) rows of TS floats
    const int T = TT ? TT : a.T;
    const int TS = T | 1, D = (T - 1) / 2;
    const int table = (a.L + 1) * T;
    for (int e = threadIdx.x; e < table; e += kLanes) {
        const int p = e / T;
        hs[p * TS + (e - p * T)] = a.table[e];
    }
    const gfdm::StreamTiles tiles(out, 2, a.n_out, a.tile_vec);
    for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
        const gfdm::TileSpan t = tiles.tile(tile);
        // 1. xs[k] = x[j0 + k] for k < nstage
        int64_t idx_lo, idx_hi;
        uint32_t frac;
        position(a, t.i_lo, idx_lo, frac);
        position(a, t.i_hi - 1, idx_hi, frac);
        const int64_t j0 = SC16 ? idx_lo - D : gfdm::stage_first(a.in, idx_lo - D);
        const int nstage = (int)std::min<int64_t>(idx_hi - D + T - j0, kStage);     // <= kStage by the host's choice of tile_vec
        if (SC16) {
            const gfdm::sc16_io* const s = static_cast<const gfdm::sc16_io*>(a.in);
            for (int k = threadIdx.x; k < nstage; k += kLanes) {
                const int64_t j = j0 + k;
                xs[k] = (j >= -a.history && j < a.n_in) ? gfdm::sc16_to_cf(s[j]) : make_float2(0.f, 0.f);
            }
        } else {
            gfdm::stage_in<0>(xs, static_cast<const cf*>(a.in), j0, nstage, a.history, a.n_in, kLanes);
        }
        __syncthreads();
        // 2. the tile's vectors: samples i (may be -1) and i + 1 (may be n_out)
        for (int64_t v = t.v0 + threadIdx.x; v < t.v1; v += kLanes) {
            const int64_t i = tiles.first(v);
            cf y[2] = { make_float2(0.f, 0.f), make_float2(0.f, 0.f) };
            int64_t idx;
            if (i >= 0) {
                position(a, i, idx, frac);
                y[0] = output<INTERP>(xs + (int)(idx - D - j0), hs, frac, a.lg, T, TS);
            }
            if (i + 1 < a.n_out) {
                position(a, i + 1, idx, frac);
                y[1] = output<INTERP>(xs + (int)(idx - D - j0), hs, frac, a.lg, T, TS);
            }
            gfdm::store_vector<0>(reinterpret_cast<unsigned char*>(out), tiles, i, y, 1.f);
        }
        __syncthreads();             // xs is rewritten for the next tile
    }
}

int table_shape_check(int n_taps, int n_phases, int interp)
{
    if (n_taps < 1 || n_taps > kMaxTaps) return api_fail(GFDM_HIP_EINVAL, "n_taps must lie in 1 .. 64");
    if (n_phases < 1 || n_phases > kMaxPhases || (n_phases & (n_phases - 1))) return api_fail(GFDM_HIP_EINVAL, "n_phases must be a power of two in 1 .. 1024");
    if ((n_phases + 1) * n_taps > kMaxTable) return api_fail(GFDM_HIP_EINVAL, "(n_phases + 1) * n_taps must not exceed 8256");
    if (interp != 0 && interp != 1) return api_fail(GFDM_HIP_EINVAL, "interp must be 0 (nearest row) or 1 (linear between rows)");
    return GFDM_HIP_OK;
}

int step_check(uint64_t step)
{
    if (step < kStepMin || step > kStepMax) return api_fail(GFDM_HIP_EINVAL, "step must lie in 2^29 .. 2^35 (Q32.32: 1/8 .. 8)");
    return GFDM_HIP_OK;
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int resampler_check(int n_taps, int n_phases, int interp, uint64_t step, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    int rc = table_shape_check(n_taps, n_phases, interp);
    if (rc == GFDM_HIP_OK) rc = step_check(step);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_out < 0) return api_fail(GFDM_HIP_EINVAL, "n_out must be >= 0");
    if (n_in < 0) return api_fail(GFDM_HIP_EINVAL, "n_in must be >= 0");
    if (history < 0) return api_fail(GFDM_HIP_EINVAL, "history must be >= 0");
    if (pos < 0 || pos >= kMaxPos) return api_fail(GFDM_HIP_EINVAL, "pos must lie in 0 .. 2^62 - 1");
    const int64_t lim = INT64_MAX / (int64_t)sizeof(cf);
    if (n_out > lim) return api_fail(GFDM_HIP_EINVAL, "the byte size of the output overflows int64");
    if (n_in > lim || history > lim - n_in) return api_fail(GFDM_HIP_EINVAL, "the byte size of the input overflows int64");
    if ((u128)pos + (u128)n_out * step >= (u128)1 << 94) return api_fail(GFDM_HIP_EINVAL, "pos + n_out * step must stay below 2^94");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_resampler {
    gfdm::DeviceCtx ctx;
    int T = 0, L = 0, lg = 0, interp = 0;
    uint64_t step = 0;
    std::vector<float> taps;
    float* d_taps = nullptr;
    ~gfdm_hip_resampler()
    {
        if (!d_taps) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(d_taps);
    }
};

namespace {

int check_call(const gfdm_hip_resampler* h, const void* out, const void* in, int sc16, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = resampler_check(h->T, h->L, h->interp, h->step, n_out, n_in, history, pos);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_out == 0) return GFDM_HIP_OK;
    if (!out || (!in && history + n_in > 0)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return gfdm::check_no_overlap(out, sizeof(cf), n_out, in, sc16 ? 4 : 8, n_in, history, "n_in", "the resampler");      // the interpolator reads neighbours
}

// the largest number of output vectors whose input span fits kStage for any pos and any alignment: the 2 tile_vec outputs of a tile
// meet at most ((2 tile_vec - 1) * step >> 32) + 2 input positions, their windows add D in front and T - 1 - D behind
int tile_vec_for(uint64_t step, int T)
{
    const int D = (T - 1) / 2, room = kStage - gfdm::max_stage(2, D, T - 1 - D, 2);
    const uint64_t m = ((uint64_t)room << 32) / step;                              // (m * step >> 32) <= room
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((m + 1) / 2, kTileVecMax));
}
static_assert(gfdm::max_stage(2 + (int)(kStepMax >> 32), 0, kMaxTaps - 1, 2) <= kStage, "the one vector of the smallest tile fits the stage at the largest step and T");

template <int SC16, int INTERP>
void launch_T(const ResampleArgs& a, cf* out, dim3 grid, size_t lds, hipStream_t s)
{
    switch (a.T) {
    case 8: hipLaunchKernelGGL((k_resample<SC16, INTERP, 8>), grid, dim3(kLanes), lds, s, a, out); break;
    case 16: hipLaunchKernelGGL((k_resample<SC16, INTERP, 16>), grid, dim3(kLanes), lds, s, a, out); break;
    case 32: hipLaunchKernelGGL((k_resample<SC16, INTERP, 32>), grid, dim3(kLanes), lds, s, a, out); break;
    default: hipLaunchKernelGGL((k_resample<SC16, INTERP, 0>), grid, dim3(kLanes), lds, s, a, out); break;
    }
}

// the one launch of a call; out and in are device pointers, the handle's step is read here
int resample_enqueue(const gfdm_hip_resampler* h, int sc16, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos, hipStream_t s)
{
    if (n_out == 0) return GFDM_HIP_OK;
    const int rc = gfdm::check_sample_alignment(out, sizeof(cf), in, sc16 ? 4 : 8);
    if (rc != GFDM_HIP_OK) return rc;
    ResampleArgs a;
    a.in = in;
    a.table = h->d_taps;
    a.n_out = n_out;
    a.n_in = n_in;
    a.history = history;
    a.pos = (uint64_t)pos;
    a.step = h->step;
    a.T = h->T;
    a.L = h->L;
    a.lg = h->lg;
    a.tile_vec = tile_vec_for(h->step, h->T);
    const dim3 grid((unsigned)std::min<int64_t>(gfdm::StreamTiles(out, 2, n_out, a.tile_vec).ntiles, kMaxGroups));
    const size_t lds = kStage * sizeof(cf) + (size_t)(h->L + 1) * (h->T | 1) * sizeof(float);
    cf* const o = static_cast<cf*>(out);
    if (sc16) {
        if (h->interp) launch_T<1, 1>(a, o, grid, lds, s);
        else launch_T<1, 0>(a, o, grid, lds, s);
    } else {
        if (h->interp) launch_T<0, 1>(a, o, grid, lds, s);
        else launch_T<0, 0>(a, o, grid, lds, s);
    }
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int resample_device(gfdm_hip_resampler* h, int sc16, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos, void* stream)
{
    const int rc = check_call(h, out, in, sc16, n_out, n_in, history, pos);
    if (rc != GFDM_HIP_OK || n_out == 0) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) { return resample_enqueue(h, sc16, out, in, n_out, n_in, history, pos, s); });
}

// upload history + n_in samples, one enqueue on the handle's stream, download n_out
int resample_host(gfdm_hip_resampler* h, int sc16, float* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    const int rc = check_call(h, out, in, sc16, n_out, n_in, history, pos);
    if (rc != GFDM_HIP_OK || n_out == 0) return rc;
    const size_t sb = sc16 ? 4 : 8;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(in ? static_cast<const unsigned char*>(in) - (size_t)history * sb : nullptr, (size_t)(history + n_in) * sb);
    const auto y = hc.out(reinterpret_cast<cf*>(out), (size_t)n_out);
    return hc.run([&](hipStream_t s) {
        return resample_enqueue(h, sc16, y.dev(), x.dev() ? x.dev() + (size_t)history * sb : nullptr, n_out, n_in, history, pos, s);
    });
}

}  // namespace

extern "C" {

int gfdm_hip_resampler_create(gfdm_hip_resampler** out, const float* taps, int n_taps, int n_phases, int interp, uint64_t step, int device)
{
    return gfdm::create_handle(
        out, device,
        [&](gfdm_hip_resampler& h) -> int {
            const int rc = resampler_check(n_taps, n_phases, interp, step, 0, 0, 0, 0);
            if (rc != GFDM_HIP_OK) return rc;
            if (!taps) return api_fail(GFDM_HIP_EINVAL, "NULL taps");
            const int n = (n_phases + 1) * n_taps;
            for (int i = 0; i < n; ++i)
                if (!std::isfinite(taps[i])) return api_fail(GFDM_HIP_EINVAL, "taps must be finite");
            h.T = n_taps;
            h.L = n_phases;
            while ((1 << h.lg) < n_phases) ++h.lg;
            h.interp = interp;
            h.step = step;
            h.taps.assign(taps, taps + n);
            return GFDM_HIP_OK;
        },
        [&](gfdm_hip_resampler& h) -> int {
            const size_t bytes = h.taps.size() * sizeof(float);
            hipError_t e = hipMalloc(&h.d_taps, bytes);
            if (e == hipSuccess) e = hipMemcpy(h.d_taps, h.taps.data(), bytes, hipMemcpyHostToDevice);
            return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "resampler table upload");
        });
}

int gfdm_hip_resampler_destroy(gfdm_hip_resampler* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_resampler_n_taps(const gfdm_hip_resampler* h) { return h ? h->T : GFDM_HIP_EINVAL; }
int gfdm_hip_resampler_n_phases(const gfdm_hip_resampler* h) { return h ? h->L : GFDM_HIP_EINVAL; }
int gfdm_hip_resampler_interp(const gfdm_hip_resampler* h) { return h ? h->interp : GFDM_HIP_EINVAL; }
int gfdm_hip_resampler_taps(const gfdm_hip_resampler* h, float* taps)
{
    if (!h || !taps) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    std::copy(h->taps.begin(), h->taps.end(), taps);
    return GFDM_HIP_OK;
}
int gfdm_hip_resampler_step(const gfdm_hip_resampler* h, uint64_t* step)
{
    if (!h || !step) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    *step = h->step;
    return GFDM_HIP_OK;
}
int gfdm_hip_resampler_set_step(gfdm_hip_resampler* h, uint64_t step)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = step_check(step);
    if (rc == GFDM_HIP_OK) h->step = step;
    return rc;
}

int gfdm_hip_resampler_check(int n_taps, int n_phases, int interp, uint64_t step, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    return resampler_check(n_taps, n_phases, interp, step, n_out, n_in, history, pos);
}

int gfdm_hip_resampler_plan(uint64_t step, int n_taps, int64_t pos, int64_t n_in, int flush, int64_t* n_out, int64_t* advance, int64_t* next_pos)
{
    const int rc = resampler_check(n_taps, 1, 0, step, 0, n_in, 0, pos);
    if (rc != GFDM_HIP_OK) return rc;
    const int D = (n_taps - 1) / 2;
    const int64_t lim = flush ? n_in : n_in + D - n_taps + 1;                       // idx(i) < lim
    u128 count = 0;
    if (lim > 0 && ((u128)lim << 32) > (u128)pos) count = ((((u128)lim << 32) - (u128)pos) + step - 1) / step;
    if (count > (u128)(INT64_MAX / (int64_t)sizeof(cf))) return api_fail(GFDM_HIP_EINVAL, "the byte size of the output overflows int64");
    const u128 P = (u128)pos + count * step;
    const u128 adv = std::min<u128>((u128)n_in, P >> 32);
    if (n_out) *n_out = (int64_t)count;
    if (advance) *advance = (int64_t)adv;
    if (next_pos) *next_pos = (int64_t)(P - (adv << 32));
    return GFDM_HIP_OK;
}

int gfdm_hip_resampler_resample_device(gfdm_hip_resampler* h, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos, void* stream)
{
    return resample_device(h, 0, out, in, n_out, n_in, history, pos, stream);
}
int gfdm_hip_resampler_resample_sc16_device(gfdm_hip_resampler* h, void* out, const void* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos,
                                            void* stream)
{
    return resample_device(h, 1, out, in, n_out, n_in, history, pos, stream);
}
int gfdm_hip_resampler_resample_host(gfdm_hip_resampler* h, float* out, const float* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    return resample_host(h, 0, out, in, n_out, n_in, history, pos);
}
int gfdm_hip_resampler_resample_sc16_host(gfdm_hip_resampler* h, float* out, const int16_t* in, int64_t n_out, int64_t n_in, int64_t history, int64_t pos)
{
    return resample_host(h, 1, out, in, n_out, n_in, history, pos);
}

}  // extern "C"
