// Burst shaper behind the transmitter: scaled frames placed in a continuous TX stream, complex64 or interleaved int16 I/Q (gr-gfdm
// short_burst_shaper, lib/short_burst_shaper_impl.cc:161-182, batched; and `place`, the dual of find_frame_start_at / detect).  The
// contract is written out in include/gfdm_hip.h.
//
// One kernel writes the whole stream, frames and silence alike (no memset in front: gfdm_burst.hip, k_detect_scatter, records what a
// memset node did under graph replay).  The OUTPUT is tiled, not the bursts, as a stream stage without an input stream (gfdm_streamtile.h:
// the output tiles and the store of step 3 from registers): a workgroup takes kTileVec 16-byte vectors aligned in memory, a lane one at a
// time, so every store of a wave is 1 KiB contiguous wherever pre_padding or a start puts a frame.  Each sample
// looks its burst up -- the last live b with start(b) <= i -- and is y_b[i - start(b)] when that lies inside the frame, else 0.  The
// workgroup finds the counts for the two ends of its tile (64 probes of the start list per step and wave), copies that window of the list
// to LDS, and a lane bisects the window once per vector; a tile that holds more than 255 starts looks them up in global memory.  So
//   * every sample of [0, out_len) is written exactly once and nothing else is, whatever the starts are (they live on the device and
//     cannot be checked): a start only selects WHICH frame sample is read, and that index is range-checked;
//   * the load is spread evenly whether a call has one burst and a long gap or 32768+ bursts of five samples: the grid depends on
//     out_len alone (bursts are not a grid dimension, so there is no 32768 limit to stride over);
//   * shape() is the same kernel with start(b) = pre_padding + b S computed instead of loaded.
// Normalised sc16 needs the largest component of y first: k_shaper_peak leaves one partial maximum per workgroup in the workspace
// (plain stores: nothing to zero between calls or graph replays), k_shaper_gain folds them into the gain.  A maximum is exact and
// independent of order.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"
#include "gfdm_streamtile.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::live_rows;
using gfdm::misaligned;

namespace {

constexpr int kLanes = 256;
constexpr int kWave = 64;                 // gfx9 wavefront
constexpr int kTileVec = 4 * kLanes;     // 16-byte vectors per tile: 16 KiB of output
constexpr int kMaxTiles = 8192;          // workgroups per launch; the tiles beyond are strided over
constexpr int kPeakParts = 1024;         // partial maxima in the workspace (one per workgroup of k_shaper_peak)
constexpr int kPeakPer = 8;              // samples per lane and pass of k_shaper_peak
constexpr size_t kWorkspaceBytes = (size_t)(4 + kPeakParts) * sizeof(float);      // gain, top, two spare words, then the partials

struct ShapeArgs {
    const cf* frames;        // [n_bursts][F]
    int F;
    int64_t n_bursts;
    const int64_t* count;    // optional (device): live bursts = clamp(*count, 0, n_bursts)
    const int64_t* starts;   // place: [n_bursts] (device); shape: NULL, start(b) = first + b stride
    int64_t first, stride;
    int64_t out_len;
    float sr, si;            // scale
    const float* gain;       // sc16, normalised: the gain k_shaper_gain left (device); NULL = 1
};

__device__ __forceinline__ int64_t start_of(const ShapeArgs& a, int64_t b) { return a.starts ? a.starts[b] : a.first + b * a.stride; }

// lo + the number of b in [lo, hi) with start(b) <= i, for ascending starts; for any others some value in [lo, hi]
__device__ __forceinline__ int64_t count_le(const ShapeArgs& a, int64_t i, int64_t lo, int64_t hi)
{
    while (lo < hi) {
        const int64_t m = lo + (hi - lo) / 2;
        if (start_of(a, m) <= i) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__device__ __forceinline__ cf scaled(const ShapeArgs& a, cf x)
{
    return make_float2(fmaf(a.sr, x.x, -(a.si * x.y)), fmaf(a.sr, x.y, a.si * x.x));
}

// count_le for a wave-uniform i, by the wave: 64 probes per step, one load latency each (three steps for 2^18 bursts, where the
// bisection is a chain of 18 dependent loads -- measured: that chain, not the bytes, set the kernel's time)
__device__ __forceinline__ int64_t wave_count_le(const ShapeArgs& a, int64_t i, int64_t lo, int64_t hi)
{
    const int lane = threadIdx.x & (kWave - 1);
    while (lo < hi) {
        const int64_t step = (hi - lo + kWave - 1) / kWave, m = lo + lane * step;
        const int cnt = __popcll(__ballot(m < hi && start_of(a, m) <= i));      // ascending starts: the first cnt probes
        if (cnt == 0) return lo;
        hi = std::min(hi, lo + cnt * step);         // probe cnt (or the end) is above i
        lo += (cnt - 1) * step + 1;                 // probe cnt - 1 is not: at most step - 1 candidates are left
    }
    return lo;
}

// y at stream position i: the burst is looked up among the counts [c0, c1] of the tile's ends
__device__ __forceinline__ cf stream_sample(const ShapeArgs& a, int64_t i, int64_t c0, int64_t c1)
{
    const int64_t c = count_le(a, i, c0, c1);
    if (c == 0) return make_float2(0.f, 0.f);
    const int64_t b = c - 1;
    const uint64_t k = (uint64_t)i - (uint64_t)start_of(a, b);      // wraps to a huge value for a start above i (or absurdly far below)
    if (k >= (uint64_t)a.F) return make_float2(0.f, 0.f);
    return scaled(a, a.frames[b * a.F + (int64_t)k]);
}

// the samples i0 .. i0 + VPS - 1 of the stream (zero outside [0, out_len)), bursts looked up in global memory: any number per tile
template <int VPS>
__device__ __forceinline__ void vector_from_global(const ShapeArgs& a, int64_t i0, int64_t c0, int64_t c1, cf* y)
{
#pragma unroll
    for (int j = 0; j < VPS; ++j) {
        const int64_t i = i0 + j;
        y[j] = (i >= 0 && i < a.out_len) ? stream_sample(a, i, c0, c1) : make_float2(0.f, 0.f);
    }
}

// ... bursts looked up in the tile's window of the start list in LDS: win[j] = start(c0 - 1 + j), j < w (win[0] = INT64_MIN where there is
// no burst c0 - 1: its distance to any i is no frame index).  One bisection per vector, then a step to the next start where a sample reaches it.
template <int VPS>
__device__ __forceinline__ void vector_from_window(const ShapeArgs& a, int64_t i0, int64_t c0, const int64_t* win, int w, cf* y)
{
    const int64_t first = std::max(i0, (int64_t)0);
    int lo = 0, hi = w - 1;                          // entries of win[1 .. w) that are <= first
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (win[1 + m] <= first) lo = m + 1;
        else hi = m;
    }
    int idx = lo;
    int64_t st = win[idx], nxt = idx + 1 < w ? win[idx + 1] : INT64_MAX;
#pragma unroll
    for (int j = 0; j < VPS; ++j) {
        const int64_t i = i0 + j;
        y[j] = make_float2(0.f, 0.f);
        if (i < 0 || i >= a.out_len) continue;
        while (i >= nxt) {                           // at most w - 1 steps in all
            ++idx;
            st = nxt;
            nxt = idx + 1 < w ? win[idx + 1] : INT64_MAX;
        }
        const uint64_t k = (uint64_t)i - (uint64_t)st;
        if (k < (uint64_t)a.F) y[j] = scaled(a, a.frames[(c0 - 1 + idx) * a.F + (int64_t)k]);
    }
}

// SC16 = 0: out is complex64; 1: interleaved int16 I/Q
template <int SC16>
__global__ __launch_bounds__(kLanes) void k_shaper_place(ShapeArgs a, void* __restrict__ out)
{
    constexpr int VPS = SC16 ? 4 : 2;            // samples per 16-byte vector
    __shared__ int64_t win[kLanes];
    const int64_t n_live = live_rows(a.count, a.n_bursts);
    const float g = a.gain ? *a.gain : 1.f;
    const gfdm::StreamTiles tiles(out, VPS, a.out_len, kTileVec);
    unsigned char* const base = static_cast<unsigned char*>(out);
    for (int64_t tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
        const gfdm::TileSpan t = tiles.tile(tile);
        const int64_t v0 = t.v0, v1 = t.v1;
        const int64_t c0 = wave_count_le(a, t.i_lo, 0, n_live), c1 = wave_count_le(a, t.i_hi - 1, c0, n_live);
        const bool windowed = c1 - c0 + 1 <= kLanes;           // the usual case: the tile's starts, and the one before, fit the window
        const int w = windowed ? (int)(c1 - c0 + 1) : 0;
        if ((int)threadIdx.x < w) {
            const int64_t b = c0 - 1 + threadIdx.x;
            win[threadIdx.x] = b >= 0 ? start_of(a, b) : INT64_MIN;
        }
        __syncthreads();
        cf y[kTileVec / kLanes][VPS];            // all loads of a lane's vectors before its stores, so that their latencies overlap
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t v = v0 + u * kLanes + threadIdx.x;
            if (v >= v1) continue;
            if (windowed) vector_from_window<VPS>(a, tiles.first(v), c0, win, w, y[u]);
            else vector_from_global<VPS>(a, tiles.first(v), c0, c1, y[u]);
        }
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t v = v0 + u * kLanes + threadIdx.x;
            if (v < v1) gfdm::store_vector<SC16>(base, tiles, tiles.first(v), y[u], g);
        }
        __syncthreads();                         // win is rewritten for the next tile
    }
}

// part[blockIdx.x] = the largest |re| or |im| of y over the workgroup's share of the live frames (0 where it has none)
__global__ __launch_bounds__(kLanes) void k_shaper_peak(ShapeArgs a, float* __restrict__ part)
{
    __shared__ float wmax[kLanes / 32];
    const int64_t total = live_rows(a.count, a.n_bursts) * a.F;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x; i < total; i += (int64_t)gridDim.x * kLanes) {
        const cf y = scaled(a, a.frames[i]);
        m = fmaxf(m, fmaxf(fabsf(y.x), fabsf(y.y)));
    }
    for (int o = warpSize / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const int lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize, nwave = kLanes / warpSize;
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nwave; ++w) m = fmaxf(m, wmax[w]);
        part[blockIdx.x] = m;
    }
}

// res[0] = gain = (float)(peak / top), 1 where top is 0; res[1] = top.  One workgroup.
__global__ __launch_bounds__(kLanes) void k_shaper_gain(const float* __restrict__ part, int nparts, double peak, float* __restrict__ res)
{
    __shared__ float wmax[kLanes / 32];
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += kLanes) m = fmaxf(m, part[i]);
    for (int o = warpSize / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const int lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize, nwave = kLanes / warpSize;
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nwave; ++w) m = fmaxf(m, wmax[w]);
        res[0] = m > 0.f ? (float)(peak / (double)m) : 1.f;
        res[1] = m;
    }
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int shaper_check(int F, int pre, int post, double peak, int64_t n_bursts, int64_t out_len)
{
    if (F < 1) return api_fail(GFDM_HIP_EINVAL, "frame_len must be >= 1");
    if (pre < 0) return api_fail(GFDM_HIP_EINVAL, "Pre-padding length MUST be >= 0!");            // short_burst_shaper_impl.cc:78-83
    if (post < 0) return api_fail(GFDM_HIP_EINVAL, "Post-padding length MUST be >= 0!");
    if (!(peak == 0.0 || (peak > 0.0 && peak <= 32767.0))) return api_fail(GFDM_HIP_EINVAL, "peak must be 0 (fixed gain) or lie in (0, 32767]");
    if (n_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "n_bursts must be >= 0");
    if (out_len < 0) return api_fail(GFDM_HIP_EINVAL, "out_len must be >= 0");
    const int64_t lim = INT64_MAX / (int64_t)sizeof(cf);
    if (out_len > lim || n_bursts > lim / F) return api_fail(GFDM_HIP_EINVAL, "the byte size of the frames or of the stream overflows int64");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_burst_shaper {
    gfdm::DeviceCtx ctx;
    int F = 0, pre = 0, post = 0;
    float sr = 1.f, si = 0.f;
};

namespace {

// what one call places where: shape() and place() differ in this alone
struct Layout {
    const int64_t* starts;   // device, or NULL for the regular slots of shape()
    const int64_t* count;    // device, or NULL
    int64_t first, stride, out_len;
};

// n_bursts slots of S = pre + F + post samples; EINVAL when their byte size overflows
int shape_layout(const gfdm_hip_burst_shaper* h, int64_t n_bursts, Layout* l)
{
    const int64_t S = (int64_t)h->pre + h->F + h->post;
    if (n_bursts > INT64_MAX / (int64_t)sizeof(cf) / S) return api_fail(GFDM_HIP_EINVAL, "the byte size of the stream overflows int64");
    *l = Layout{ nullptr, nullptr, h->pre, S, n_bursts * S };
    return GFDM_HIP_OK;
}

int check_call(const gfdm_hip_burst_shaper* h, const void* out, const void* frames, const Layout& l, bool placed, double peak, int64_t n_bursts)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = shaper_check(h->F, h->pre, h->post, peak, n_bursts, l.out_len);
    if (rc != GFDM_HIP_OK) return rc;
    if (l.out_len > 0 && !out) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    if (n_bursts > 0 && (!frames || (placed && !l.starts))) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

// the launches of one call: (peak, gain,) place.  Everything is a device pointer.
int shaper_enqueue(gfdm_hip_burst_shaper* h, int sc16, void* out, const cf* frames, const Layout& l, int64_t n_bursts, double peak, void* workspace,
                   hipStream_t s)
{
    if (l.out_len == 0) return GFDM_HIP_OK;
    const int rc = gfdm::check_sample_alignment(out, sc16 ? 4 : 8, frames, sizeof(cf));
    if (rc != GFDM_HIP_OK) return rc;
    ShapeArgs a = { frames, h->F, n_bursts, l.count, l.starts, l.first, l.stride, l.out_len, h->sr, h->si, nullptr };
    if (sc16 && peak > 0.0) {
        if (!workspace || misaligned(workspace, 16)) return api_fail(GFDM_HIP_EINVAL, "normalised sc16 output needs a 16-byte aligned workspace");
        float* res = static_cast<float*>(workspace);
        float* part = res + 4;
        const int64_t per = (int64_t)kLanes * kPeakPer;
        const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(kPeakParts, (n_bursts * h->F + per - 1) / per));
        hipLaunchKernelGGL(k_shaper_peak, dim3((unsigned)nparts), dim3(kLanes), 0, s, a, part);
        GFDM_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_shaper_gain, dim3(1), dim3(kLanes), 0, s, (const float*)part, nparts, peak, res);
        GFDM_TRY(hipGetLastError());
        a.gain = res;
    }
    const dim3 grid((unsigned)std::min<int64_t>(gfdm::StreamTiles(out, sc16 ? 4 : 2, l.out_len, kTileVec).ntiles, kMaxTiles));
    if (sc16) hipLaunchKernelGGL(k_shaper_place<1>, grid, dim3(kLanes), 0, s, a, out);
    else hipLaunchKernelGGL(k_shaper_place<0>, grid, dim3(kLanes), 0, s, a, out);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int shaper_device(gfdm_hip_burst_shaper* h, int sc16, void* out, const void* frames, const Layout& l, bool placed, int64_t n_bursts, double peak,
                  void* workspace, void* stream)
{
    const int rc = check_call(h, out, frames, l, placed, peak, n_bursts);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return shaper_enqueue(h, sc16, out, static_cast<const cf*>(frames), l, n_bursts, peak, workspace, s);
    });
}

// what the host flavour of place can see of the live starts (include/gfdm_hip.h)
int check_starts(const gfdm_hip_burst_shaper* h, const int64_t* starts, int64_t n_live, int64_t out_len)
{
    char buf[200];
    for (int64_t b = 0; b < n_live; ++b) {
        const int64_t st = starts[b], end = b + 1 < n_live ? starts[b + 1] : out_len;
        if (st < 0) {
            snprintf(buf, sizeof(buf), "starts[%lld] = %lld is negative", (long long)b, (long long)st);
            return api_fail(GFDM_HIP_EINVAL, buf);
        }
        if (st > end || h->F > end - st) {
            snprintf(buf, sizeof(buf), "frame %lld (start %lld, %d samples) runs into %s at %lld", (long long)b, (long long)st, h->F,
                     b + 1 < n_live ? "its successor" : "the end of the stream", (long long)end);
            return api_fail(GFDM_HIP_EINVAL, buf);
        }
    }
    return GFDM_HIP_OK;
}

// upload the frames (and the starts and the count), one enqueue on the handle's stream, download the stream
int shaper_host(gfdm_hip_burst_shaper* h, int sc16, void* out, const float* frames, Layout l, bool placed, int64_t n_bursts, double peak)
{
    int rc = check_call(h, out, frames, l, placed, peak, n_bursts);
    if (rc != GFDM_HIP_OK) return rc;
    if (placed) {
        rc = check_starts(h, l.starts, live_rows(l.count, n_bursts), l.out_len);
        if (rc != GFDM_HIP_OK) return rc;
    }
    if (l.out_len == 0) return GFDM_HIP_OK;
    const size_t n = (size_t)n_bursts;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(reinterpret_cast<const cf*>(frames), n * h->F);
    const auto cnt = hc.in(l.count, 1);
    const auto st = hc.in(l.starts, n);
    const auto ws = hc.scratch<unsigned char>(kWorkspaceBytes);
    const auto y = hc.out(static_cast<unsigned char*>(out), (size_t)l.out_len * (sc16 ? 2 * sizeof(int16_t) : sizeof(cf)));
    return hc.run([&](hipStream_t s) {
        l.count = cnt.dev();
        l.starts = st.dev();
        return shaper_enqueue(h, sc16, y.dev(), x.dev(), l, n_bursts, peak, ws.dev(), s);
    });
}

}  // namespace

extern "C" {

int gfdm_hip_burst_shaper_create(gfdm_hip_burst_shaper** out, int frame_len, int pre_padding, int post_padding, float scale_re, float scale_im, int device)
{
    return gfdm::create_handle(out, device, [&](gfdm_hip_burst_shaper& h) {
        h.F = frame_len;
        h.pre = pre_padding;
        h.post = post_padding;
        h.sr = scale_re;
        h.si = scale_im;
        return shaper_check(frame_len, pre_padding, post_padding, 0.0, 0, 0);
    });
}

int gfdm_hip_burst_shaper_destroy(gfdm_hip_burst_shaper* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_burst_shaper_frame_len(const gfdm_hip_burst_shaper* h) { return h ? h->F : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_shaper_pre_padding(const gfdm_hip_burst_shaper* h) { return h ? h->pre : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_shaper_post_padding(const gfdm_hip_burst_shaper* h) { return h ? h->post : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_shaper_scale(const gfdm_hip_burst_shaper* h, float* scale)
{
    if (!h || !scale) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    scale[0] = h->sr;
    scale[1] = h->si;
    return GFDM_HIP_OK;
}

int gfdm_hip_burst_shaper_check(int frame_len, int pre_padding, int post_padding, double peak, int64_t n_bursts, int64_t out_len)
{
    return shaper_check(frame_len, pre_padding, post_padding, peak, n_bursts, out_len);
}

int64_t gfdm_hip_burst_shaper_workspace_bytes(const gfdm_hip_burst_shaper* h, int64_t n_bursts, int64_t out_len)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = shaper_check(h->F, h->pre, h->post, 0.0, n_bursts, out_len);
    if (rc != GFDM_HIP_OK) return rc;
    return (int64_t)kWorkspaceBytes;
}

int gfdm_hip_burst_shaper_shape_device(gfdm_hip_burst_shaper* h, void* out, const void* frames, int64_t n_bursts, void* workspace, void* stream)
{
    Layout l;
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "n_bursts must be >= 0");
    const int rc = shape_layout(h, n_bursts, &l);
    return rc != GFDM_HIP_OK ? rc : shaper_device(h, 0, out, frames, l, false, n_bursts, 0.0, workspace, stream);
}
int gfdm_hip_burst_shaper_shape_sc16_device(gfdm_hip_burst_shaper* h, void* out, const void* frames, int64_t n_bursts, double peak, void* workspace,
                                            void* stream)
{
    Layout l;
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "n_bursts must be >= 0");
    const int rc = shape_layout(h, n_bursts, &l);
    return rc != GFDM_HIP_OK ? rc : shaper_device(h, 1, out, frames, l, false, n_bursts, peak, workspace, stream);
}
int gfdm_hip_burst_shaper_shape_host(gfdm_hip_burst_shaper* h, float* out, const float* frames, int64_t n_bursts)
{
    Layout l;
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "n_bursts must be >= 0");
    const int rc = shape_layout(h, n_bursts, &l);
    return rc != GFDM_HIP_OK ? rc : shaper_host(h, 0, out, frames, l, false, n_bursts, 0.0);
}
int gfdm_hip_burst_shaper_shape_sc16_host(gfdm_hip_burst_shaper* h, int16_t* out, const float* frames, int64_t n_bursts, double peak)
{
    Layout l;
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "n_bursts must be >= 0");
    const int rc = shape_layout(h, n_bursts, &l);
    return rc != GFDM_HIP_OK ? rc : shaper_host(h, 1, out, frames, l, false, n_bursts, peak);
}

int gfdm_hip_burst_shaper_place_device(gfdm_hip_burst_shaper* h, void* out, int64_t out_len, const void* frames, const void* starts, const void* count,
                                       int64_t n_bursts, void* workspace, void* stream)
{
    const Layout l = { static_cast<const int64_t*>(starts), static_cast<const int64_t*>(count), 0, 0, out_len };
    return shaper_device(h, 0, out, frames, l, true, n_bursts, 0.0, workspace, stream);
}
int gfdm_hip_burst_shaper_place_sc16_device(gfdm_hip_burst_shaper* h, void* out, int64_t out_len, const void* frames, const void* starts, const void* count,
                                            int64_t n_bursts, double peak, void* workspace, void* stream)
{
    const Layout l = { static_cast<const int64_t*>(starts), static_cast<const int64_t*>(count), 0, 0, out_len };
    return shaper_device(h, 1, out, frames, l, true, n_bursts, peak, workspace, stream);
}
int gfdm_hip_burst_shaper_place_host(gfdm_hip_burst_shaper* h, float* out, int64_t out_len, const float* frames, const int64_t* starts, const int64_t* count,
                                     int64_t n_bursts)
{
    return shaper_host(h, 0, out, frames, Layout{ starts, count, 0, 0, out_len }, true, n_bursts, 0.0);
}
int gfdm_hip_burst_shaper_place_sc16_host(gfdm_hip_burst_shaper* h, int16_t* out, int64_t out_len, const float* frames, const int64_t* starts,
                                          const int64_t* count, int64_t n_bursts, double peak)
{
    return shaper_host(h, 1, out, frames, Layout{ starts, count, 0, 0, out_len }, true, n_bursts, peak);
}

}  // extern "C"
