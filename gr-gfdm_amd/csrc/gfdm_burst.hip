// Burst acquisition in front of the receive chain: preamble timing / CFO synchronisation (pygfdm's find_frame_start,
// python/pygfdm/synchronization.py:154-263) and burst extraction (gr-gfdm extract_burst_cc, lib/extract_burst_cc_impl.cc:72-242).
// Their outputs (frame starts, rotations) stay on the device and feed the extractor and the estimated receivers without a host
// round trip.  The contracts are written out in include/gfdm_hip.h.
//
// Synchroniser: the windows of one call lie on a regular grid (first, stride, n_windows), so every argument is checked on the host.
// Four launches per find_frame_start, every one a grid of (correlation tiles x windows):
//   k_sync_ic       |ac| over the tile and its cp_len halo, ic of the tile, first-index argmax of ic     -> key in coarse[w]
//   k_sync_coarse   one wave per window: ac[nm] again, cfo, metric, sc_rot
//   k_sync_fine     ic of the tile again, 2K-tap correlation with the CFO-rotated preamble, first-index argmax of |pcc| ic
//                                                                                                          -> key in frame_start[w]
//   k_sync_finalize keys -> stream indices
// The two argmax keys live in the caller's int64 outputs until the last launch: no scratch memory, so the device entry point
// neither allocates nor synchronises (hipGraph-capturable like the rest of the C-ABI).  Every position's ac is its own serial sum
// of 2K products, every ic its own serial sum of cp_len + 1 magnitudes in ascending order: no running sums (fp32 drift over a long
// window would move the argmax) and bit-equal values however a window is tiled or batched.  ic is recomputed in k_sync_fine rather
// than stored: about 1.5x the work of the correlation alone, against an n_windows-sized buffer the caller would have to provide.
//
// Extractor: out[b][n] = scale_b s[off_b - backoff + n] (conj(r_b) / |r_b|)^n, samples outside [0, stream_len) read as zero.  The
// phase of sample n is reduced in fp64 (n angle(r) mod 2 pi) and only then rounded to fp32 for sincos, so the rotation error does
// not grow with n (an fp32 recurrence as in volk's rotator drifts by ~n ulp).
#include "../../include/gfdm_hip.h"
#include "gfdm_plan.h"
#include "gfdm_dft.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::api_fail_hip;

namespace {

#define BURST_TRY(expr)                                          \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return api_fail_hip(_e, #expr);    \
    } while (0)

// as in gfdm_stages.hip: clears the sticky HIP error of earlier calls, selects the handle's device for the scope
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        (void)hipGetLastError();
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int open_device(int dev)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return api_fail(GFDM_HIP_ENODEV, "no HIP device available (this library has no CPU path)");
    if (dev < 0 || dev >= count) return api_fail(GFDM_HIP_ENODEV, "HIP device ordinal out of range");
    DeviceGuard guard(dev);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    return GFDM_HIP_OK;
}

constexpr int kTile = 256;               // correlation positions per workgroup, one per lane
constexpr int kMaxK = 1024;
constexpr unsigned kMaxGridY = 32768;    // windows / bursts beyond this are strided over

__device__ __forceinline__ cf czero() { return make_float2(0.f, 0.f); }

// first-index argmax in one 64-bit atomicMax: the value's bits (a non-negative float orders like its bit pattern; + 0.0f turns -0 into
// +0) above the complement of the index, so that of equal values the smaller index wins -- also across workgroups
__device__ __forceinline__ unsigned long long argmax_key(float v, int i)
{
    return ((unsigned long long)__float_as_uint(v + 0.0f) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}
__device__ __forceinline__ int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }
__device__ __forceinline__ float key_value(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }

// max of the workgroup's keys into *dst (one global atomic per workgroup)
__device__ void block_argmax(unsigned long long key, unsigned long long* dst)
{
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    for (int o = warpSize / 2; o > 0; o >>= 1) key = std::max(key, (unsigned long long)__shfl_xor(key, o));
    if ((threadIdx.x & (warpSize - 1)) == 0) atomicMax(&best, key);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(dst, best);
}

// ac at the position whose 2K samples start at x:  2 sum_{n<K} conj(x[n]) x[n+K] / sum_{n<2K} |x[n]|^2, 0 where the energy is 0
__device__ __forceinline__ cf ac_at(const cf* x, int K)
{
    float cr0 = 0.f, ci0 = 0.f, e0 = 0.f, cr1 = 0.f, ci1 = 0.f, e1 = 0.f;   // two chains: even / odd n
    int n = 0;
    for (; n + 1 < K; n += 2) {
        const cf a0 = x[n], b0 = x[n + K], a1 = x[n + 1], b1 = x[n + 1 + K];
        cr0 = fmaf(a0.x, b0.x, fmaf(a0.y, b0.y, cr0));
        ci0 = fmaf(a0.x, b0.y, fmaf(-a0.y, b0.x, ci0));
        e0 = fmaf(a0.x, a0.x, fmaf(a0.y, a0.y, fmaf(b0.x, b0.x, fmaf(b0.y, b0.y, e0))));
        cr1 = fmaf(a1.x, b1.x, fmaf(a1.y, b1.y, cr1));
        ci1 = fmaf(a1.x, b1.y, fmaf(-a1.y, b1.x, ci1));
        e1 = fmaf(a1.x, a1.x, fmaf(a1.y, a1.y, fmaf(b1.x, b1.x, fmaf(b1.y, b1.y, e1))));
    }
    const float e = e0 + e1;
    if (!(e > 0.f)) return czero();
    const float g = 2.f / e;
    return make_float2((cr0 + cr1) * g, (ci0 + ci1) * g);
}

// ic of the lane's position n = i0 + threadIdx.x of a window (W samples at `win`, P = W - 2K correlation positions):
//   ic[n] = mean(|ac|[n - cp .. n]) for cp <= n < P, else 0      (pygfdm abs_integrate, synchronization.py:146-151)
// |ac| is computed segment by segment (kTile positions each) from i0 - cp (rounded down to a whole segment) up to the tile itself, so
// LDS holds kTile + 2K samples whatever cp is.  On return xs[0 .. kTile + 2K - 1) holds the window's samples from i0 on (zero past W)
// -- the fine stage correlates straight out of it -- and *ac_n the lane's own ac.
__device__ float tile_ic(const cf* __restrict__ win, int W, int K, int cp, int P, int i0, cf* xs, float* mag, cf* ac_n)
{
    const int t = threadIdx.x, n = i0 + t;
    const int lo = std::max(0, i0 - cp), hi = std::min(P, i0 + kTile);
    const int span = kTile + 2 * K - 1;
    const bool live = (n >= cp) && (n < P);
    float acc = 0.f;
    for (int seg = i0 - (i0 - lo + kTile - 1) / kTile * kTile; seg <= i0; seg += kTile) {
        for (int j = t; j < span; j += kTile) {
            const int g = seg + j;
            xs[j] = (g >= 0 && g < W) ? win[g] : czero();
        }
        __syncthreads();
        const int m = seg + t;
        cf c = czero();
        if (m >= lo && m < hi) c = ac_at(xs + t, K);
        mag[t] = sqrtf(c.x * c.x + c.y * c.y);
        if (seg == i0) *ac_n = c;
        __syncthreads();
        if (live) {
            const int a0 = std::max(seg, n - cp), a1 = std::min(seg + kTile, n + 1);
            for (int j = a0; j < a1; ++j) acc += mag[j - seg];
        }
        __syncthreads();
    }
    return live ? acc / (float)(cp + 1) : 0.f;
}

struct SyncArgs {
    const cf* samples;       // window w starts at samples[first + w stride]
    int64_t first, stride, nwin;
    int64_t origin;          // stream index of samples[0] (host path: the uploaded span starts inside the caller's stream)
    int W, K, cp, P;
};

// dynamic LDS: xs [kTile + 2K] (+ q [2K] in the fine stage) complex, then mag [kTile]
__global__ __launch_bounds__(kTile) void k_sync_ic(SyncArgs a, cf* __restrict__ ac_out, float* __restrict__ ic_out, unsigned long long* __restrict__ key)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* xs = reinterpret_cast<cf*>(smem_raw);
    float* mag = reinterpret_cast<float*>(xs + kTile + 2 * a.K);
    const int i0 = blockIdx.x * kTile, n = i0 + threadIdx.x;
    for (int64_t w = blockIdx.y; w < a.nwin; w += gridDim.y) {
        cf acn;
        const float ic = tile_ic(a.samples + a.first + w * a.stride, a.W, a.K, a.cp, a.P, i0, xs, mag, &acn);
        if (n < a.P) {
            if (ac_out) ac_out[w * a.P + n] = acn;
            if (ic_out) ic_out[w * a.P + n] = ic;
        }
        if (key) block_argmax(n < a.P ? argmax_key(ic, n) : 0ull, key + w);
    }
}

// one wave per window: nm from the key, cfo = angle(ac[nm]) / 2 pi, metric = ic[nm], sc_rot = exp(j angle(ac[nm]) / K)
__global__ __launch_bounds__(64) void k_sync_coarse(SyncArgs a, const unsigned long long* __restrict__ key, float* __restrict__ cfo, float* __restrict__ metric,
                                                    cf* __restrict__ sc_rot)
{
    for (int64_t w = blockIdx.x; w < a.nwin; w += gridDim.x) {
        if (threadIdx.x != 0) continue;
        const unsigned long long k = key[w];
        const cf c = ac_at(a.samples + a.first + w * a.stride + key_index(k), a.K);
        const float ang = atan2f(c.y, c.x);
        cfo[w] = ang * (float)(0.5 / M_PI);
        metric[w] = key_value(k);
        float s, co;
        sincosf(ang / (float)a.K, &s, &co);
        sc_rot[w] = make_float2(co, s);
    }
}

// |pcc[i]| ic[i], pcc[i] = sum_{m<2K} s'[i+m] conj(p[m]) / 2K with s'[n] = s[n] exp(j pi cfo n / K).  The factor exp(j pi cfo i / K)
// has modulus 1 and drops out of |pcc|, so the preamble is rotated instead: q[m] = conj(p[m]) exp(j pi cfo m / K), once per workgroup.
__global__ __launch_bounds__(kTile) void k_sync_fine(SyncArgs a, const cf* __restrict__ preamble, const float* __restrict__ cfo,
                                                     unsigned long long* __restrict__ key)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* xs = reinterpret_cast<cf*>(smem_raw);
    cf* q = xs + kTile + 2 * a.K;
    float* mag = reinterpret_cast<float*>(q + 2 * a.K);
    const int K2 = 2 * a.K;
    const int i0 = blockIdx.x * kTile, n = i0 + threadIdx.x;
    for (int64_t w = blockIdx.y; w < a.nwin; w += gridDim.y) {
        const float th = (float)M_PI * cfo[w] / (float)a.K;
        for (int m = threadIdx.x; m < K2; m += kTile) {
            float s, c;
            sincosf(th * (float)m, &s, &c);
            const cf p = preamble[m];
            q[m] = make_float2(p.x * c + p.y * s, p.x * s - p.y * c);
        }
        cf acn;
        const float ic = tile_ic(a.samples + a.first + w * a.stride, a.W, a.K, a.cp, a.P, i0, xs, mag, &acn);   // syncs after q is written
        float score = 0.f;
        if (n < a.P) {
            float re = 0.f, im = 0.f;
            const cf* x = xs + threadIdx.x;
            for (int m = 0; m < K2; ++m) {
                const cf v = x[m], c = q[m];
                re = fmaf(v.x, c.x, fmaf(-v.y, c.y, re));
                im = fmaf(v.x, c.y, fmaf(v.y, c.x, im));
            }
            score = sqrtf(re * re + im * im) / (float)K2 * ic;
        }
        block_argmax(n < a.P ? argmax_key(score, n) : 0ull, key + w);
        __syncthreads();          // q and xs are rewritten for the next window
    }
}

__global__ void k_sync_finalize(SyncArgs a, int64_t* __restrict__ frame_start, int64_t* __restrict__ coarse)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.nwin) return;
    const int64_t start = a.origin + a.first + w * a.stride;
    frame_start[w] = start + key_index((unsigned long long)frame_start[w]);
    coarse[w] = start + key_index((unsigned long long)coarse[w]);
}

// out[b][n] = scale_b s[off_b - backoff + n] rot_b^n; one burst per blockIdx.y, samples strided over blockIdx.x
__global__ __launch_bounds__(kTile) void k_extract(cf* __restrict__ out, const cf* __restrict__ s, int64_t stream_len, const int64_t* __restrict__ offsets,
                                                   const float* __restrict__ scale, const cf* __restrict__ sc_rot, int correct, int burst_len, int backoff,
                                                   int64_t nbursts)
{
    __shared__ double phi;       // -angle(r_b): the phase step of conj(r_b) / |r_b|
    __shared__ int rotate;
    for (int64_t b = blockIdx.y; b < nbursts; b += gridDim.y) {
        if (threadIdx.x == 0) {
            rotate = 0;
            phi = 0.0;
            if (correct && sc_rot) {
                const cf r = sc_rot[b];
                if (r.x != 0.f || r.y != 0.f) {
                    rotate = 1;
                    phi = -atan2((double)r.y, (double)r.x);
                }
            }
        }
        __syncthreads();
        const int64_t base = offsets[b] - backoff;
        const float g = scale ? scale[b] : 1.f;
        for (int n = blockIdx.x * kTile + threadIdx.x; n < burst_len; n += gridDim.x * kTile) {
            const int64_t i = base + n;
            cf x = (i >= 0 && i < stream_len) ? gfdm::dft::ld_stream(s + i) : czero();
            x = make_float2(x.x * g, x.y * g);
            if (rotate) {
                double ph = phi * (double)n;
                ph -= 2.0 * M_PI * rint(ph * (0.5 / M_PI));
                float sn, cs;
                sincosf((float)ph, &sn, &cs);
                x = make_float2(x.x * cs - x.y * sn, x.x * sn + x.y * cs);
            }
            gfdm::dft::st_stream(out, b * burst_len + n, x);
        }
        __syncthreads();
    }
}

size_t sync_lds(int K, bool fine) { return (size_t)(kTile + 2 * K + (fine ? 2 * K : 0)) * sizeof(cf) + kTile * sizeof(float); }

// a device buffer that lives for one host call
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};

}  // namespace

struct gfdm_hip_burst_sync {
    int device = 0;
    hipStream_t stream = nullptr;
    int K = 0, cp = 0, W = 0;
    cf* d_preamble = nullptr;          // [2K], normalised to unit average energy
    ~gfdm_hip_burst_sync()
    {
        DeviceGuard guard(device);
        if (d_preamble) (void)hipFree(d_preamble);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct gfdm_hip_burst_extractor {
    int device = 0;
    hipStream_t stream = nullptr;
    int burst_len = 0, backoff = 0, correct = 1;
    ~gfdm_hip_burst_extractor()
    {
        DeviceGuard guard(device);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// the grid of windows must lie inside [0, stream_len)
int check_windows(const gfdm_hip_burst_sync* h, const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n < 0 || first < 0 || stride < 0 || stream_len < 0) return api_fail(GFDM_HIP_EINVAL, "negative window count, first, stride or stream_len");
    if (n == 0) return GFDM_HIP_OK;
    if (!samples) return api_fail(GFDM_HIP_EINVAL, "NULL sample buffer");
    if (n > (int64_t)1 << 31) return api_fail(GFDM_HIP_EINVAL, "more than 2^31 windows in one call");
    // last window: first + (n - 1) stride + W <= stream_len, without overflow
    const int64_t room = stream_len - h->W - first;
    if (room < 0 || (n > 1 && stride > room / (n - 1))) {
        char buf[200];
        snprintf(buf, sizeof(buf), "window grid (first %lld, stride %lld, %lld windows of %d) runs past stream_len %lld", (long long)first, (long long)stride,
                 (long long)n, h->W, (long long)stream_len);
        return api_fail(GFDM_HIP_EINVAL, buf);
    }
    return GFDM_HIP_OK;
}

// enqueue the synchroniser; fused (frame_start != NULL) or the auto-correlation stage (ac / ic)
int sync_enqueue(gfdm_hip_burst_sync* h, const cf* samples, int64_t first, int64_t stride, int64_t n, int64_t origin, int64_t* frame_start, int64_t* coarse,
                 float* cfo, float* metric, cf* sc_rot, cf* ac, float* ic, hipStream_t s)
{
    const SyncArgs a = { samples, first, stride, n, origin, h->W, h->K, h->cp, h->W - 2 * h->K };
    const dim3 grid((unsigned)((a.P + kTile - 1) / kTile), (unsigned)std::min<int64_t>(n, kMaxGridY));
    if (!frame_start) {
        hipLaunchKernelGGL(k_sync_ic, grid, dim3(kTile), sync_lds(h->K, false), s, a, ac, ic, (unsigned long long*)nullptr);
        BURST_TRY(hipGetLastError());
        return GFDM_HIP_OK;
    }
    BURST_TRY(hipMemsetAsync(frame_start, 0, (size_t)n * sizeof(int64_t), s));
    BURST_TRY(hipMemsetAsync(coarse, 0, (size_t)n * sizeof(int64_t), s));
    hipLaunchKernelGGL(k_sync_ic, grid, dim3(kTile), sync_lds(h->K, false), s, a, (cf*)nullptr, (float*)nullptr, (unsigned long long*)coarse);
    BURST_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_coarse, dim3((unsigned)std::min<int64_t>(n, 1 << 20)), dim3(64), 0, s, a, (const unsigned long long*)coarse, cfo, metric, sc_rot);
    BURST_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_fine, grid, dim3(kTile), sync_lds(h->K, true), s, a, (const cf*)h->d_preamble, (const float*)cfo, (unsigned long long*)frame_start);
    BURST_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_finalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, frame_start, coarse);
    BURST_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// host path of the synchroniser: the span the windows cover goes up, the results come back
int sync_host(gfdm_hip_burst_sync* h, const float* samples, int64_t first, int64_t stride, int64_t n, int64_t* frame_start, int64_t* coarse, float* cfo,
              float* metric, float* sc_rot, float* ac, float* ic)
{
    DeviceGuard guard(h->device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    const int64_t span = (n - 1) * stride + h->W, P = h->W - 2 * h->K;
    DevBuf d_in, d_out;
    BURST_TRY(d_in.alloc((size_t)span * sizeof(cf)));
    const size_t n_res = (size_t)n * (2 * sizeof(int64_t) + 2 * sizeof(float) + sizeof(cf));
    const size_t n_stage = (size_t)n * P * (sizeof(cf) + sizeof(float));
    BURST_TRY(d_out.alloc(frame_start ? n_res : n_stage));
    BURST_TRY(hipMemcpyAsync(d_in.p, samples + 2 * first, (size_t)span * sizeof(cf), hipMemcpyHostToDevice, h->stream));
    unsigned char* o = static_cast<unsigned char*>(d_out.p);
    int rc;
    if (frame_start) {
        int64_t* d_fs = reinterpret_cast<int64_t*>(o);
        int64_t* d_co = d_fs + n;
        cf* d_rot = reinterpret_cast<cf*>(d_co + n);
        float* d_cfo = reinterpret_cast<float*>(d_rot + n);
        float* d_met = d_cfo + n;
        rc = sync_enqueue(h, static_cast<const cf*>(d_in.p), 0, stride, n, first, d_fs, d_co, d_cfo, d_met, d_rot, nullptr, nullptr, h->stream);
        if (rc != GFDM_HIP_OK) return rc;
        BURST_TRY(hipMemcpyAsync(frame_start, d_fs, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        BURST_TRY(hipMemcpyAsync(coarse, d_co, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        BURST_TRY(hipMemcpyAsync(sc_rot, d_rot, (size_t)n * sizeof(cf), hipMemcpyDeviceToHost, h->stream));
        BURST_TRY(hipMemcpyAsync(cfo, d_cfo, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        BURST_TRY(hipMemcpyAsync(metric, d_met, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    } else {
        cf* d_ac = reinterpret_cast<cf*>(o);
        float* d_ic = reinterpret_cast<float*>(d_ac + (size_t)n * P);
        rc = sync_enqueue(h, static_cast<const cf*>(d_in.p), 0, stride, n, first, nullptr, nullptr, nullptr, nullptr, nullptr, d_ac, d_ic, h->stream);
        if (rc != GFDM_HIP_OK) return rc;
        if (ac) BURST_TRY(hipMemcpyAsync(ac, d_ac, (size_t)n * P * sizeof(cf), hipMemcpyDeviceToHost, h->stream));
        if (ic) BURST_TRY(hipMemcpyAsync(ic, d_ic, (size_t)n * P * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    BURST_TRY(hipStreamSynchronize(h->stream));
    return GFDM_HIP_OK;
}

int extract_check(const gfdm_hip_burst_extractor* h, const void* out, const void* samples, int64_t stream_len, const void* offsets, int64_t n)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n < 0 || stream_len < 0) return api_fail(GFDM_HIP_EINVAL, "negative burst count or stream_len");
    if (n > 0 && (!out || !offsets || (!samples && stream_len > 0))) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

int extract_enqueue(gfdm_hip_burst_extractor* h, cf* out, const cf* samples, int64_t stream_len, const int64_t* offsets, const float* scale, const cf* sc_rot,
                    int64_t n, hipStream_t s)
{
    const dim3 grid((unsigned)std::min((h->burst_len + kTile - 1) / kTile, 64), (unsigned)std::min<int64_t>(n, kMaxGridY));
    hipLaunchKernelGGL(k_extract, grid, dim3(kTile), 0, s, out, samples, stream_len, offsets, scale, sc_rot, h->correct, h->burst_len, h->backoff, n);
    BURST_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

}  // namespace

extern "C" {

int gfdm_hip_burst_sync_create(gfdm_hip_burst_sync** out, int fft_len, int cp_len, const float* core_preamble, int n_preamble, int64_t window_len, int device)
{
    if (!out) return api_fail(GFDM_HIP_EINVAL, "NULL handle pointer");
    *out = nullptr;
    const int K = fft_len;
    char buf[200];
    if (K < 2 || K > kMaxK) return api_fail(GFDM_HIP_EINVAL, "fft_len must lie in [2, 1024]");
    if (!core_preamble || n_preamble != 2 * K) {                                                    // synchronization.py:228-229
        snprintf(buf, sizeof(buf), "Preamble length(%d) must be equal to 2K(%d)!", n_preamble, 2 * K);
        return api_fail(GFDM_HIP_EINVAL, buf);
    }
    if (cp_len < 0) return api_fail(GFDM_HIP_EINVAL, "cp_len must be >= 0");
    if (window_len < (int64_t)2 * K + cp_len + 1) {
        snprintf(buf, sizeof(buf), "window_len(%lld) must be at least 2 fft_len + cp_len + 1 (%d)", (long long)window_len, 2 * K + cp_len + 1);
        return api_fail(GFDM_HIP_EINVAL, buf);
    }
    if (window_len > (int64_t)1 << 30) return api_fail(GFDM_HIP_EINVAL, "window_len above 2^30");
    // initialize_sync_algorithm (synchronization.py:225-236): unit average energy
    double e = 0.0;
    for (int i = 0; i < 4 * K; ++i) e += (double)core_preamble[i] * core_preamble[i];
    if (!(e > 0.0) || !std::isfinite(e)) return api_fail(GFDM_HIP_EINVAL, "preamble has no energy");
    const double g = 1.0 / std::sqrt(e / (2 * K));
    std::vector<float> pre(4 * K);
    for (int i = 0; i < 4 * K; ++i) pre[i] = (float)(core_preamble[i] * g);
    int rc = open_device(device);
    if (rc != GFDM_HIP_OK) return rc;
    gfdm_hip_burst_sync* h = new (std::nothrow) gfdm_hip_burst_sync();
    if (!h) return api_fail(GFDM_HIP_ENOMEM, "out of host memory");
    h->device = device;
    h->K = K;
    h->cp = cp_len;
    h->W = (int)window_len;
    DeviceGuard guard(device);
    hipError_t err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipMalloc(&h->d_preamble, pre.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(h->d_preamble, pre.data(), pre.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        delete h;
        return api_fail_hip(err, "burst_sync_create");
    }
    *out = h;
    return GFDM_HIP_OK;
}

int gfdm_hip_burst_sync_destroy(gfdm_hip_burst_sync* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_burst_sync_fft_len(const gfdm_hip_burst_sync* h) { return h ? h->K : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_sync_cp_len(const gfdm_hip_burst_sync* h) { return h ? h->cp : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_burst_sync_window_len(const gfdm_hip_burst_sync* h) { return h ? h->W : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_burst_sync_corr_len(const gfdm_hip_burst_sync* h) { return h ? h->W - 2 * h->K : GFDM_HIP_EINVAL; }

int gfdm_hip_burst_sync_find_frame_start_device(gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows, void* stream)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!frame_start || !coarse || !cfo || !metric || !sc_rot) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    DeviceGuard guard(h->device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    return sync_enqueue(h, static_cast<const cf*>(samples), first, stride, n_windows, 0, static_cast<int64_t*>(frame_start), static_cast<int64_t*>(coarse),
                        static_cast<float*>(cfo), static_cast<float*>(metric), static_cast<cf*>(sc_rot), nullptr, nullptr, (hipStream_t)stream);
}

int gfdm_hip_burst_sync_find_frame_start_host(gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                              const float* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!frame_start || !coarse || !cfo || !metric || !sc_rot) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    return sync_host(h, samples, first, stride, n_windows, frame_start, coarse, cfo, metric, sc_rot, nullptr, nullptr);
}

int gfdm_hip_burst_sync_auto_correlate_device(gfdm_hip_burst_sync* h, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
                                              int64_t stride, int64_t n_windows, void* stream)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!ac && !ic) return api_fail(GFDM_HIP_EINVAL, "NULL output buffers");
    DeviceGuard guard(h->device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    return sync_enqueue(h, static_cast<const cf*>(samples), first, stride, n_windows, 0, nullptr, nullptr, nullptr, nullptr, nullptr, static_cast<cf*>(ac),
                        static_cast<float*>(ic), (hipStream_t)stream);
}

int gfdm_hip_burst_sync_auto_correlate_host(gfdm_hip_burst_sync* h, float* ac, float* ic, const float* samples, int64_t stream_len, int64_t first,
                                            int64_t stride, int64_t n_windows)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!ac && !ic) return api_fail(GFDM_HIP_EINVAL, "NULL output buffers");
    return sync_host(h, samples, first, stride, n_windows, nullptr, nullptr, nullptr, nullptr, nullptr, ac, ic);
}

int gfdm_hip_burst_extractor_create(gfdm_hip_burst_extractor** out, int burst_len, int tag_backoff, int activate_cfo_correction, int device)
{
    if (!out) return api_fail(GFDM_HIP_EINVAL, "NULL handle pointer");
    *out = nullptr;
    if (burst_len < 1) return api_fail(GFDM_HIP_EINVAL, "burst_len must be >= 1");
    int rc = open_device(device);
    if (rc != GFDM_HIP_OK) return rc;
    gfdm_hip_burst_extractor* h = new (std::nothrow) gfdm_hip_burst_extractor();
    if (!h) return api_fail(GFDM_HIP_ENOMEM, "out of host memory");
    h->device = device;
    h->burst_len = burst_len;
    h->backoff = tag_backoff;
    h->correct = activate_cfo_correction ? 1 : 0;
    DeviceGuard guard(device);
    const hipError_t err = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (err != hipSuccess) {
        delete h;
        return api_fail_hip(err, "burst_extractor_create");
    }
    *out = h;
    return GFDM_HIP_OK;
}

int gfdm_hip_burst_extractor_destroy(gfdm_hip_burst_extractor* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_burst_extractor_burst_len(const gfdm_hip_burst_extractor* h) { return h ? h->burst_len : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_extractor_tag_backoff(const gfdm_hip_burst_extractor* h) { return h ? h->backoff : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_extractor_get_cfo_correction(const gfdm_hip_burst_extractor* h) { return h ? h->correct : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_extractor_set_cfo_correction(gfdm_hip_burst_extractor* h, int activate)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    h->correct = activate ? 1 : 0;
    return GFDM_HIP_OK;
}

int gfdm_hip_burst_extractor_extract_device(gfdm_hip_burst_extractor* h, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                            const void* scale, const void* sc_rot, int64_t n_bursts, void* stream)
{
    int rc = extract_check(h, out, samples, stream_len, offsets, n_bursts);
    if (rc != GFDM_HIP_OK || n_bursts == 0) return rc;
    DeviceGuard guard(h->device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    return extract_enqueue(h, static_cast<cf*>(out), static_cast<const cf*>(samples), stream_len, static_cast<const int64_t*>(offsets),
                           static_cast<const float*>(scale), static_cast<const cf*>(sc_rot), n_bursts, (hipStream_t)stream);
}

int gfdm_hip_burst_extractor_extract_host(gfdm_hip_burst_extractor* h, float* out, const float* samples, int64_t stream_len, const int64_t* offsets,
                                          const float* scale, const float* sc_rot, int64_t n_bursts)
{
    int rc = extract_check(h, out, samples, stream_len, offsets, n_bursts);
    if (rc != GFDM_HIP_OK || n_bursts == 0) return rc;
    DeviceGuard guard(h->device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    const size_t n = (size_t)n_bursts, L = (size_t)h->burst_len;
    DevBuf d_s, d_args, d_out;
    BURST_TRY(d_s.alloc((size_t)stream_len * sizeof(cf)));
    BURST_TRY(d_args.alloc(n * (sizeof(int64_t) + sizeof(float) + sizeof(cf))));
    BURST_TRY(d_out.alloc(n * L * sizeof(cf)));
    int64_t* d_off = static_cast<int64_t*>(d_args.p);
    cf* d_rot = reinterpret_cast<cf*>(d_off + n);
    float* d_scale = reinterpret_cast<float*>(d_rot + n);
    if (stream_len) BURST_TRY(hipMemcpyAsync(d_s.p, samples, (size_t)stream_len * sizeof(cf), hipMemcpyHostToDevice, h->stream));
    BURST_TRY(hipMemcpyAsync(d_off, offsets, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    if (sc_rot) BURST_TRY(hipMemcpyAsync(d_rot, sc_rot, n * sizeof(cf), hipMemcpyHostToDevice, h->stream));
    if (scale) BURST_TRY(hipMemcpyAsync(d_scale, scale, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = extract_enqueue(h, static_cast<cf*>(d_out.p), static_cast<const cf*>(d_s.p), stream_len, d_off, scale ? d_scale : nullptr, sc_rot ? d_rot : nullptr,
                         n_bursts, h->stream);
    if (rc != GFDM_HIP_OK) return rc;
    BURST_TRY(hipMemcpyAsync(out, d_out.p, n * L * sizeof(cf), hipMemcpyDeviceToHost, h->stream));
    BURST_TRY(hipStreamSynchronize(h->stream));
    return GFDM_HIP_OK;
}

}  // extern "C"
