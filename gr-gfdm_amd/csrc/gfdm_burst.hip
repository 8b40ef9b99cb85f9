// Burst acquisition in front of the receive chain: preamble timing / CFO synchronisation (pygfdm's find_frame_start,
// python/pygfdm/synchronization.py:154-263) and burst extraction (gr-gfdm extract_burst_cc, lib/extract_burst_cc_impl.cc:72-242).
// Their outputs (frame starts, rotations) stay on the device and feed the extractor and the estimated receivers without a host
// round trip.  The contracts are written out in include/gfdm_hip.h.
//
// Synchroniser: the windows of one call lie on a regular grid (first, stride, n_windows), so every argument is checked on the host, or at
// the starts of a device array (find_frame_start_at, and the detector's own list), which are clamped into the stream instead.
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
// Detector: the windows' starts found on the device (k_detect_scan, k_detect_offsets, k_detect_scatter; described above them).
//
// Extractor: out[b][n] = scale_b s[off_b - backoff + n] (conj(r_b) / |r_b|)^n, samples outside [0, stream_len) read as zero.  The
// phase of sample n is reduced in fp64 (n angle(r) mod 2 pi) and only then rounded to fp32 for sincos, so the rotation error does
// not grow with n (an fp32 recurrence as in volk's rotator drifts by ~n ulp).
//
// The *_host flavours are the enqueues of the device entry points inside a staged call (gfdm::HostCall, gfdm_hostcall.h): one allocation,
// uploads, the enqueue, downloads and one synchronise on the handle's own stream.
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
#include "gfdm_dft.h"
#include "gfdm_burstfetch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::DeviceGuard;
using gfdm::sample_bytes;

namespace {

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

// an sc16 capture read as complex samples (ac_at straight from global memory)
struct Sc16View {
    const gfdm::sc16_io* p;
    __device__ __forceinline__ cf operator[](int n) const { return gfdm::sc16_to_cf(p[n]); }
};

// ac at the position whose 2K samples start at x:  2 sum_{n<K} conj(x[n]) x[n+K] / sum_{n<2K} |x[n]|^2, 0 where the energy is 0.
// X: const cf* or Sc16View -- the sums are the same instructions in the same order on the same fp32 values.
template <class X>
__device__ __forceinline__ cf ac_at(X x, int K)
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
    if (n < K) {                                                             // odd K: the last n is even, so it extends the even chain
        const cf a0 = x[n], b0 = x[n + K];
        cr0 = fmaf(a0.x, b0.x, fmaf(a0.y, b0.y, cr0));
        ci0 = fmaf(a0.x, b0.y, fmaf(-a0.y, b0.x, ci0));
        e0 = fmaf(a0.x, a0.x, fmaf(a0.y, a0.y, fmaf(b0.x, b0.x, fmaf(b0.y, b0.y, e0))));
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
__device__ float tile_ic(const void* __restrict__ win, int fmt, int W, int K, int cp, int P, int i0, cf* xs, float* mag, cf* ac_n)
{
    const int t = threadIdx.x, n = i0 + t;
    const int lo = std::max(0, i0 - cp), hi = std::min(P, i0 + kTile);
    const int span = kTile + 2 * K - 1;
    const bool live = (n >= cp) && (n < P);
    float acc = 0.f;
    for (int seg = i0 - (i0 - lo + kTile - 1) / kTile * kTile; seg <= i0; seg += kTile) {
        for (int j = t; j < span; j += kTile) {
            const int g = seg + j;
            xs[j] = (g >= 0 && g < W) ? gfdm::capture_load(win, g, fmt) : czero();
        }
        __syncthreads();
        const int m = seg + t;
        cf c = czero();
        if (m >= lo && m < hi) c = ac_at((const cf*)(xs + t), K);
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
    const void* samples;     // window w starts at sample first + w stride, or at starts[w] when a start array is given
    int fmt;                 // gfdm::SampleFormat of samples
    int64_t first, stride, nwin;
    int64_t origin;          // stream index of samples[0] (host path: the uploaded span starts inside the caller's stream)
    int W, K, cp, P;
    const int64_t* starts;   // optional (device): window w starts at clamp(starts[w], 0, last)
    int64_t nstarts, last;   // entries of starts (windows beyond are empty), stream_len - W
    int skip_empty;          // the detector's lists: a negative start marks an empty slot (else it is clamped to 0)
};

// start of window w in samples, or -1 for an empty slot (only with a start array)
__device__ __forceinline__ int64_t window_start(const SyncArgs& a, int64_t w)
{
    if (!a.starts) return a.first + w * a.stride;
    if (w >= a.nstarts) return -1;
    const int64_t st = a.starts[w];
    if (st < 0 && a.skip_empty) return -1;
    return std::min(std::max(st, (int64_t)0), a.last);
}

// dynamic LDS: xs [kTile + 2K] (+ q [2K] in the fine stage) complex, then mag [kTile]
__global__ __launch_bounds__(kTile) void k_sync_ic(SyncArgs a, cf* __restrict__ ac_out, float* __restrict__ ic_out, unsigned long long* __restrict__ key)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* xs = reinterpret_cast<cf*>(smem_raw);
    float* mag = reinterpret_cast<float*>(xs + kTile + 2 * a.K);
    const int i0 = blockIdx.x * kTile, n = i0 + threadIdx.x;
    for (int64_t w = blockIdx.y; w < a.nwin; w += gridDim.y) {
        const int64_t st = window_start(a, w);
        if (st < 0) continue;       // empty slot: the key stays 0
        cf acn;
        const float ic = tile_ic(gfdm::capture_at(a.samples, st, a.fmt), a.fmt, a.W, a.K, a.cp, a.P, i0, xs, mag, &acn);
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
        const int64_t st = window_start(a, w);
        if (st < 0) {
            cfo[w] = 0.f;
            metric[w] = 0.f;
            sc_rot[w] = czero();
            continue;
        }
        const unsigned long long k = key[w];
        const void* x = gfdm::capture_at(a.samples, st + key_index(k), a.fmt);
        const cf c = a.fmt == gfdm::SAMPLES_SC16 ? ac_at(Sc16View{ static_cast<const gfdm::sc16_io*>(x) }, a.K) : ac_at(static_cast<const cf*>(x), a.K);
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
        const int64_t st = window_start(a, w);
        if (st < 0) continue;
        const float th = (float)M_PI * cfo[w] / (float)a.K;
        for (int m = threadIdx.x; m < K2; m += kTile) {
            float s, c;
            sincosf(th * (float)m, &s, &c);
            const cf p = preamble[m];
            q[m] = make_float2(p.x * c + p.y * s, p.x * s - p.y * c);
        }
        cf acn;
        const float ic = tile_ic(gfdm::capture_at(a.samples, st, a.fmt), a.fmt, a.W, a.K, a.cp, a.P, i0, xs, mag, &acn);   // syncs after q is written
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
    const int64_t st = window_start(a, w);
    if (st < 0) {
        frame_start[w] = -1;
        coarse[w] = -1;
        return;
    }
    const int64_t start = a.origin + st;
    frame_start[w] = start + key_index((unsigned long long)frame_start[w]);
    coarse[w] = start + key_index((unsigned long long)coarse[w]);
}

// out[b][n] = scale_b s[off_b - backoff + n] rot_b^n; one burst per blockIdx.y, samples strided over blockIdx.x
__global__ __launch_bounds__(kTile) void k_extract(cf* __restrict__ out, const void* __restrict__ s, int fmt, int64_t stream_len, const int64_t* __restrict__ offsets,
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
                gfdm::burst_phase_step(r, rotate, phi);
            }
        }
        __syncthreads();
        const int64_t base = offsets[b] - backoff;
        const float g = scale ? scale[b] : 1.f;
        for (int n = blockIdx.x * kTile + threadIdx.x; n < burst_len; n += gridDim.x * kTile)
            gfdm::dft::st_stream(out, b * burst_len + n, gfdm::burst_fetch(s, fmt, stream_len, base, n, g, rotate, phi));      // gfdm_burstfetch.h
        __syncthreads();
    }
}

// ---- detector: every burst of a stream (contract in include/gfdm_hip.h) ----
// One workgroup scans a tile of per * kTile positions of the whole stream taken as one window, segment by segment (kTile positions,
// one per lane) from R positions before the tile to R positions after it.  Each segment's ic comes from tile_ic -- the values
// auto_correlate yields, bit for bit; from a tile's second segment on, with cp <= kTile, the |ac| of the segment before is kept
// instead of computed again (segment_ic) -- and lives in LDS only while the segment is being compared: its running maxima from both
// ends (pre, suf) give every lane the maximum over the part of its +-R neighbourhood that falls into the segment in one read (a
// part strictly inside a segment, which needs R < kTile - 1, is walked).  Per own position a lane keeps one float in LDS -- the
// maximum to its left until its own segment arrives, its ic from then on -- and one "beaten" bit, so LDS is per * kTile floats
// whatever R is and nothing is written per position: the stream is read (per kTile + 2 R + cp) / (per kTile) times, and a tile
// writes its peak count and its peaks in ascending order (at most one per R + 1 positions).
constexpr int kScanMaxPer = 16;          // positions per lane and tile (one bit each in `beaten`); 32 measured 14 % slower (LDS per tile halves the residency)
constexpr int kScanTiles = 4096;         // per is chosen so that a long stream has about this many tiles

struct ScanArgs {
    const void* samples;
    int fmt;                 // gfdm::SampleFormat of samples
    int n, K, cp, P;         // stream_len, P = n - 2K positions
    int R, per, cap;         // min_distance, segments per tile, list entries per tile
    float thr;
};

// max of ic over the global positions [a, b] (inside the segment that starts at g)
__device__ __forceinline__ float seg_range_max(const float* icv, const float* pre, const float* suf, int g, int a, int b)
{
    if (a == g) return pre[b - g];
    if (b == g + kTile - 1) return suf[a - g];
    float m = icv[a - g];
    for (int j = a + 1; j <= b; ++j) m = fmaxf(m, icv[j - g]);
    return m;
}

size_t scan_lds(int K, int per) { return (size_t)(kTile + 2 * K) * sizeof(cf) + (size_t)(5 + per) * kTile * sizeof(float); }

// tile_ic for the segment at g (>= kTile) of a walk in ascending order with cp <= kTile: magp holds |ac| of the segment before, as
// tile_ic left it, so only this segment's |ac| is computed (into magc).  The lane's sum runs over the same magnitudes in the same
// ascending order as tile_ic's: the value is bit-equal.
__device__ float segment_ic(const void* __restrict__ win, int fmt, int W, int K, int cp, int P, int g, cf* xs, const float* magp, float* magc)
{
    const int t = threadIdx.x, n = g + t;
    for (int j = t; j < kTile + 2 * K - 1; j += kTile) xs[j] = (g + j < W) ? gfdm::capture_load(win, g + j, fmt) : czero();
    __syncthreads();
    cf c = czero();
    if (n < P) c = ac_at((const cf*)(xs + t), K);
    magc[t] = sqrtf(c.x * c.x + c.y * c.y);
    __syncthreads();
    if (n < cp || n >= P) return 0.f;
    float acc = 0.f;
    for (int j = n - cp; j < g; ++j) acc += magp[j - g + kTile];
    for (int j = std::max(g, n - cp); j <= n; ++j) acc += magc[j - g];
    return acc / (float)(cp + 1);
}

// dynamic LDS: xs [kTile + 2K] complex, mag [2][kTile], icv, pre, suf [kTile] float, own [per][kTile] float
__global__ __launch_bounds__(kTile) void k_detect_scan(ScanArgs a, int* __restrict__ counts, int* __restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* xs = reinterpret_cast<cf*>(smem_raw);
    float* mag = reinterpret_cast<float*>(xs + kTile + 2 * a.K);
    float* icv = mag + 2 * kTile;
    float* pre = icv + kTile;
    float* suf = pre + kTile;
    float* own = suf + kTile + threadIdx.x;             // own[r * kTile]: this lane's position of segment r; no other lane touches it
    __shared__ float wmax[kTile / 32];
    __shared__ int wcnt[kTile / 32];
    const int t = threadIdx.x, lane = t & (warpSize - 1), wave = t / warpSize, nwave = kTile / warpSize;
    const int c0 = blockIdx.x * a.per * kTile;
    const int hs = (a.R + kTile - 1) / kTile;           // halo segments on either side
    unsigned beaten = 0;                                // bit r: an ic at least as large within R before, or larger within R after
    for (int r = 0; r < a.per; ++r) own[r * kTile] = -1.f;

    // the neighbourhoods are cut at the stream ends: segments inside [0, P) only
    const int s_lo = std::max(-hs, -(c0 / kTile)), s_hi = std::min(a.per + hs, (a.P - c0 + kTile - 1) / kTile);
    for (int s = s_lo; s < s_hi; ++s) {
        const int g = c0 + s * kTile;
        float* magc = mag + (s & 1) * kTile;            // this segment's |ac|; the other half holds the segment's before
        float ic;
        if (s > s_lo && a.cp <= kTile) {
            ic = segment_ic(a.samples, a.fmt, a.n, a.K, a.cp, a.P, g, xs, mag + ((s & 1) ^ 1) * kTile, magc);
        } else {
            cf acn;
            ic = tile_ic(a.samples, a.fmt, a.n, a.K, a.cp, a.P, g, xs, magc, &acn);
        }
        const float val = (g + t < a.P) ? ic : -1.f;
        // running maxima from both ends: inside a wave by shuffles, across waves through wmax
        float p = val, q = val;
        for (int o = 1; o < warpSize; o <<= 1) {
            const float x = __shfl_up(p, o), y = __shfl_down(q, o);
            if (lane >= o) p = fmaxf(p, x);
            if (lane + o < warpSize) q = fmaxf(q, y);
        }
        if (lane == 0) wmax[wave] = q;
        icv[t] = val;
        __syncthreads();
        for (int w = 0; w < nwave; ++w) {
            const float m = wmax[w];
            if (w < wave) p = fmaxf(p, m);
            if (w > wave) q = fmaxf(q, m);
        }
        pre[t] = p;
        suf[t] = q;
        __syncthreads();
        for (int r = std::max(0, s - hs); r <= std::min(a.per - 1, s + hs); ++r) {
            const int n = c0 + r * kTile + t;
            float* slot = own + r * kTile;
            if (r >= s) {                                               // positions before n
                const int lo = std::max(g, n - a.R), hi = std::min(g + kTile - 1, n - 1);
                float m = *slot;
                if (lo <= hi) m = fmaxf(m, seg_range_max(icv, pre, suf, g, lo, hi));
                if (r == s) {                                           // the left side is complete: judge it, keep the own ic from here on
                    if (m >= val) beaten |= 1u << r;
                    m = val;
                }
                *slot = m;
            }
            if (r <= s) {                                               // positions after n
                const int lo = std::max(g, n + 1), hi = std::min(g + kTile - 1, n + a.R);
                if (lo <= hi && seg_range_max(icv, pre, suf, g, lo, hi) > *slot) beaten |= 1u << r;
            }
        }
        __syncthreads();                                                // icv, pre, suf are rewritten for the next segment
    }

    // ordered compaction inside the tile: position order is r-major, lane-minor
    int base = 0;
    int* mine = list + (int64_t)blockIdx.x * a.cap;
    for (int r = 0; r < a.per && c0 + r * kTile < a.P; ++r) {           // (a segment at or past P was never scanned: its slot holds no ic)
        const bool peak = own[r * kTile] >= a.thr && !((beaten >> r) & 1u);
        const unsigned long long b = __ballot(peak);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int k = base + __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < nwave; ++w) {
            if (w < wave) k += wcnt[w];
            base += wcnt[w];
        }
        if (peak && k < a.cap) mine[k] = c0 + r * kTile + t;
        __syncthreads();
    }
    if (t == 0) counts[blockIdx.x] = base;
}

// exclusive scan of the tiles' counts (one workgroup; a tile count is tiny against the scan itself), total -> *count
__global__ __launch_bounds__(kTile) void k_detect_offsets(const int* __restrict__ counts, int* __restrict__ offs, int ntiles, int64_t* __restrict__ count)
{
    __shared__ int wsum[kTile / 32];
    const int t = threadIdx.x, lane = t & (warpSize - 1), wave = t / warpSize, nwave = kTile / warpSize;
    int base = 0;
    for (int i0 = 0; i0 < ntiles; i0 += kTile) {
        const int i = i0 + t, c = i < ntiles ? counts[i] : 0;
        int incl = c;
        for (int o = 1; o < warpSize; o <<= 1) {
            const int x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (lane == warpSize - 1) wsum[wave] = incl;
        __syncthreads();
        int excl = base + incl - c;
        for (int w = 0; w < nwave; ++w) {
            if (w < wave) excl += wsum[w];
            base += wsum[w];
        }
        if (i < ntiles) offs[i] = excl;
        __syncthreads();
    }
    if (t == 0) *count = base;
}

// starts[slot] = clamp(peak - lead, 0, last) for the lowest nslots peaks, -1 (empty) for the slots from *count on.  The empty slots are
// written here and not by a byte-pattern memset in front: as a node of a captured graph that memset left them positive from the second
// replay on (measured: they then ran as windows at `last`), where a store does what it says on every replay.
__global__ __launch_bounds__(kTile) void k_detect_scatter(const int* __restrict__ counts, const int* __restrict__ offs, const int* __restrict__ list, int cap,
                                                          int ntiles, int lead, int64_t last, int64_t* __restrict__ starts, int64_t nslots,
                                                          const int64_t* __restrict__ count)
{
    for (int64_t slot = *count + (int64_t)blockIdx.x * kTile + threadIdx.x; slot < nslots; slot += (int64_t)gridDim.x * kTile) starts[slot] = -1;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int c = std::min(counts[tile], cap), o = offs[tile];
        for (int k = threadIdx.x; k < c; k += kTile) {
            const int64_t slot = (int64_t)o + k;
            if (slot < nslots) starts[slot] = std::min(std::max((int64_t)list[(int64_t)tile * cap + k] - lead, (int64_t)0), last);
        }
    }
}

size_t sync_lds(int K, bool fine) { return (size_t)(kTile + 2 * K + (fine ? 2 * K : 0)) * sizeof(cf) + kTile * sizeof(float); }

}  // namespace

struct gfdm_hip_burst_sync {
    gfdm::DeviceCtx ctx;
    int K = 0, cp = 0, W = 0;
    cf* d_preamble = nullptr;          // [2K], normalised to unit average energy
    ~gfdm_hip_burst_sync()
    {
        if (!d_preamble) return;
        DeviceGuard guard(ctx.device);
        (void)hipFree(d_preamble);
    }
};

struct gfdm_hip_burst_extractor {
    gfdm::DeviceCtx ctx;
    int burst_len = 0, backoff = 0, correct = 1;
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

SyncArgs grid_args(const gfdm_hip_burst_sync* h, const void* samples, int fmt, int64_t first, int64_t stride, int64_t n, int64_t origin)
{
    return SyncArgs{ samples, fmt, first, stride, n, origin, h->W, h->K, h->cp, h->W - 2 * h->K, nullptr, 0, 0, 0 };
}

// windows at starts[w] (device array of nstarts entries; windows w >= nstarts are empty), clamped to [0, stream_len - W]
SyncArgs list_args(const gfdm_hip_burst_sync* h, const void* samples, int fmt, int64_t stream_len, const int64_t* starts, int64_t nstarts, int64_t n, int skip_empty)
{
    return SyncArgs{ samples, fmt, 0, 0, n, 0, h->W, h->K, h->cp, h->W - 2 * h->K, starts, nstarts, stream_len - h->W, skip_empty };
}

// the five per-window outputs of a synchroniser call, on the device or (host paths) in the caller's arrays
struct SyncOut {
    int64_t* frame_start; int64_t* coarse; float* cfo; float* metric; cf* sc_rot;
    bool complete() const { return frame_start && coarse && cfo && metric && sc_rot; }
};
SyncOut sync_out(void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot)      // from the pointers of the C-ABI
{
    return SyncOut{ static_cast<int64_t*>(frame_start), static_cast<int64_t*>(coarse), static_cast<float*>(cfo), static_cast<float*>(metric), static_cast<cf*>(sc_rot) };
}

dim3 sync_grid(const SyncArgs& a) { return dim3((unsigned)((a.P + kTile - 1) / kTile), (unsigned)std::min<int64_t>(a.nwin, kMaxGridY)); }

// enqueue the auto-correlation stage: ac and / or ic of every position of every window
int ac_enqueue(gfdm_hip_burst_sync* h, const SyncArgs& a, cf* ac, float* ic, hipStream_t s)
{
    hipLaunchKernelGGL(k_sync_ic, sync_grid(a), dim3(kTile), sync_lds(h->K, false), s, a, ac, ic, (unsigned long long*)nullptr);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// enqueue the fused synchroniser: the four launches of the file head, the argmax keys in o.coarse and o.frame_start until the last one
int sync_enqueue(gfdm_hip_burst_sync* h, const SyncArgs& a, const SyncOut& o, hipStream_t s)
{
    const int64_t n = a.nwin;
    const dim3 grid = sync_grid(a);
    GFDM_TRY(hipMemsetAsync(o.frame_start, 0, (size_t)n * sizeof(int64_t), s));
    GFDM_TRY(hipMemsetAsync(o.coarse, 0, (size_t)n * sizeof(int64_t), s));
    hipLaunchKernelGGL(k_sync_ic, grid, dim3(kTile), sync_lds(h->K, false), s, a, (cf*)nullptr, (float*)nullptr, (unsigned long long*)o.coarse);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_coarse, dim3((unsigned)std::min<int64_t>(n, 1 << 20)), dim3(64), 0, s, a, (const unsigned long long*)o.coarse, o.cfo, o.metric, o.sc_rot);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_fine, grid, dim3(kTile), sync_lds(h->K, true), s, a, (const cf*)h->d_preamble, (const float*)o.cfo, (unsigned long long*)o.frame_start);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sync_finalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, o.frame_start, o.coarse);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// host paths: the five outputs of n windows as pieces of the staged call, in the caller's arrays afterwards
struct SyncPieces {
    gfdm::HostCall::Piece<int64_t> frame_start, coarse;
    gfdm::HostCall::Piece<float> cfo, metric;
    gfdm::HostCall::Piece<cf> sc_rot;
    SyncOut dev() const { return SyncOut{ frame_start.dev(), coarse.dev(), cfo.dev(), metric.dev(), sc_rot.dev() }; }
};
SyncPieces sync_pieces(gfdm::HostCall& hc, const SyncOut& host, int64_t n)
{
    return SyncPieces{ hc.out(host.frame_start, (size_t)n), hc.out(host.coarse, (size_t)n), hc.out(host.cfo, (size_t)n), hc.out(host.metric, (size_t)n),
                       hc.out(host.sc_rot, (size_t)n) };
}

int check_at(const gfdm_hip_burst_sync* h, const void* samples, int64_t stream_len, const void* starts, int64_t n)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n < 0) return api_fail(GFDM_HIP_EINVAL, "negative window count");
    if (stream_len < h->W) return api_fail(GFDM_HIP_EINVAL, "stream_len is shorter than window_len");
    if (n > (int64_t)1 << 31) return api_fail(GFDM_HIP_EINVAL, "more than 2^31 windows in one call");
    if (n > 0 && (!samples || !starts)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

constexpr int64_t kMaxDetectLen = (int64_t)1 << 29;      // the scan indexes positions (and positions + R) in 32 bits
constexpr int64_t kMaxDetectDistance = (int64_t)1 << 16; // a tile walks 2 ceil(R / kTile) halo segments: the scan's cost grows with R

// the detector's argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int detect_check(int K, int cp, int64_t W, int64_t stream_len, float threshold, int64_t R, int64_t lead, int64_t max_bursts)
{
    char buf[200];
    if (K < 2 || K > kMaxK || cp < 0 || W < (int64_t)2 * K + cp + 1) return api_fail(GFDM_HIP_EINVAL, "fft_len, cp_len or window_len outside the synchroniser's range");
    if (!(threshold > 0.f)) return api_fail(GFDM_HIP_EINVAL, "threshold must be > 0");
    if (max_bursts < 0) return api_fail(GFDM_HIP_EINVAL, "max_bursts must be >= 0");
    if (lead < cp || lead > R) {
        snprintf(buf, sizeof(buf), "lead(%lld) must lie in [cp_len(%d), min_distance(%lld)]", (long long)lead, cp, (long long)R);
        return api_fail(GFDM_HIP_EINVAL, buf);
    }
    if (W - 2 * K - lead - 1 > R) {
        snprintf(buf, sizeof(buf), "min_distance(%lld) must be at least window_len - 2 fft_len - lead - 1 (%lld)", (long long)R, (long long)(W - 2 * K - lead - 1));
        return api_fail(GFDM_HIP_EINVAL, buf);
    }
    if (R > kMaxDetectDistance) return api_fail(GFDM_HIP_EINVAL, "min_distance above 2^16 (the scan's work grows with it)");
    if (stream_len < W) return api_fail(GFDM_HIP_EINVAL, "stream_len is shorter than window_len");
    if (stream_len > kMaxDetectLen) return api_fail(GFDM_HIP_EINVAL, "stream_len above 2^29 (split the capture into overlapping spans)");
    return GFDM_HIP_OK;
}

// tiling of the scan and layout of the workspace; depends on the handle and stream_len only (not on min_distance: the smallest
// one detect accepts, (W - 2K - 1) / 2, bounds the peaks per tile and per stream)
struct DetectGeom {
    int per, ntiles, cap;
    int64_t nstarts;
    size_t o_offs, o_list, o_starts, bytes;      // counts at 0
};
DetectGeom detect_geom(const gfdm_hip_burst_sync* h, int64_t stream_len)
{
    DetectGeom g;
    const int64_t P = stream_len - 2 * h->K, rmin = (h->W - 2 * h->K - 1) / 2;
    g.per = (int)std::min<int64_t>(kScanMaxPer, std::max<int64_t>(4, (P + (int64_t)kTile * kScanTiles - 1) / ((int64_t)kTile * kScanTiles)));
    const int64_t tile = (int64_t)g.per * kTile;
    g.ntiles = (int)((P + tile - 1) / tile);
    g.cap = (int)(tile / (rmin + 1) + 1);
    g.nstarts = P / (rmin + 1) + 1;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    g.o_offs = up((size_t)g.ntiles * sizeof(int));
    g.o_list = g.o_offs + up((size_t)g.ntiles * sizeof(int));
    g.o_starts = g.o_list + up((size_t)g.ntiles * g.cap * sizeof(int));
    g.bytes = g.o_starts + (size_t)g.nstarts * sizeof(int64_t);
    return g;
}

// scan -> ordered compaction -> fine stage over the window starts; count and the five outputs are device pointers
int detect_enqueue(gfdm_hip_burst_sync* h, int64_t* count, const SyncOut& o, const void* samples, int fmt, int64_t stream_len, float threshold, int64_t R, int64_t lead,
                   int64_t max_bursts, void* workspace, hipStream_t s)
{
    const DetectGeom g = detect_geom(h, stream_len);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    int* counts = reinterpret_cast<int*>(ws);
    int* offs = reinterpret_cast<int*>(ws + g.o_offs);
    int* list = reinterpret_cast<int*>(ws + g.o_list);
    int64_t* starts = reinterpret_cast<int64_t*>(ws + g.o_starts);
    const int P = (int)(stream_len - 2 * h->K);
    const ScanArgs a = { samples, fmt, (int)stream_len, h->K, h->cp, P, (int)std::min<int64_t>(R, P), g.per, g.cap, threshold };
    hipLaunchKernelGGL(k_detect_scan, dim3((unsigned)g.ntiles), dim3(kTile), scan_lds(h->K, g.per), s, a, counts, list);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_detect_offsets, dim3(1), dim3(kTile), 0, s, (const int*)counts, offs, g.ntiles, count);
    GFDM_TRY(hipGetLastError());
    if (max_bursts == 0) return GFDM_HIP_OK;
    const int64_t nslots = std::min(max_bursts, g.nstarts);
    hipLaunchKernelGGL(k_detect_scatter, dim3((unsigned)std::min(g.ntiles, 1024)), dim3(kTile), 0, s, (const int*)counts, (const int*)offs, (const int*)list, g.cap,
                       g.ntiles, (int)lead, stream_len - h->W, starts, nslots, (const int64_t*)count);
    GFDM_TRY(hipGetLastError());
    return sync_enqueue(h, list_args(h, samples, fmt, stream_len, starts, nslots, max_bursts, 1), o, s);
}

int extract_check(const gfdm_hip_burst_extractor* h, const void* out, const void* samples, int64_t stream_len, const void* offsets, int64_t n)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n < 0 || stream_len < 0) return api_fail(GFDM_HIP_EINVAL, "negative burst count or stream_len");
    if (n > 0 && (!out || !offsets || (!samples && stream_len > 0))) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

int extract_enqueue(gfdm_hip_burst_extractor* h, cf* out, const void* samples, int fmt, int64_t stream_len, const int64_t* offsets, const float* scale, const cf* sc_rot,
                    int64_t n, hipStream_t s)
{
    const dim3 grid((unsigned)std::min((h->burst_len + kTile - 1) / kTile, 64), (unsigned)std::min<int64_t>(n, kMaxGridY));
    hipLaunchKernelGGL(k_extract, grid, dim3(kTile), 0, s, out, samples, fmt, stream_len, offsets, scale, sc_rot, h->correct, h->burst_len, h->backoff, n);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

}  // namespace

// ---- the entry points that read a capture, once for both sample formats (fmt: gfdm::SampleFormat; `samples` is complex64 or interleaved
// int16 accordingly, stream_len counts samples).  The public calls and their *_sc16_* twins at the end of the file are thin wrappers.
namespace {

int sync_find_frame_start_device(int fmt, gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows, void* stream)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    const SyncOut o = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (!o.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) { return sync_enqueue(h, grid_args(h, samples, fmt, first, stride, n_windows, 0), o, s); });
}

// host paths over a window grid: the span the windows cover goes up (the grid starts at its sample 0, origin = first), the results come back
int sync_find_frame_start_host(int fmt, gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                              const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    const SyncOut host = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (!host.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    const int64_t n = n_windows;
    const size_t sb = sample_bytes(fmt);
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(samples) + (size_t)first * sb, (size_t)((n - 1) * stride + h->W) * sb);
    const SyncPieces o = sync_pieces(hc, host, n);
    return hc.run([&](hipStream_t s) { return sync_enqueue(h, grid_args(h, x.dev(), fmt, 0, stride, n, first), o.dev(), s); });
}

int sync_auto_correlate_device(int fmt, gfdm_hip_burst_sync* h, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
                                              int64_t stride, int64_t n_windows, void* stream)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!ac && !ic) return api_fail(GFDM_HIP_EINVAL, "NULL output buffers");
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return ac_enqueue(h, grid_args(h, samples, fmt, first, stride, n_windows, 0), static_cast<cf*>(ac), static_cast<float*>(ic), s);
    });
}

int sync_auto_correlate_host(int fmt, gfdm_hip_burst_sync* h, float* ac, float* ic, const void* samples, int64_t stream_len, int64_t first,
                                            int64_t stride, int64_t n_windows)
{
    int rc = check_windows(h, samples, stream_len, first, stride, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    if (!ac && !ic) return api_fail(GFDM_HIP_EINVAL, "NULL output buffers");
    const int64_t n = n_windows;
    const size_t sb = sample_bytes(fmt), np = (size_t)n * (h->W - 2 * h->K);
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(samples) + (size_t)first * sb, (size_t)((n - 1) * stride + h->W) * sb);
    const auto d_ac = hc.out(reinterpret_cast<cf*>(ac), np);          // (an output the caller left out is NULL to the kernel, which then skips it)
    const auto d_ic = hc.out(ic, np);
    return hc.run([&](hipStream_t s) { return ac_enqueue(h, grid_args(h, x.dev(), fmt, 0, stride, n, first), d_ac.dev(), d_ic.dev(), s); });
}

/* windows at arbitrary starts: the regular-grid kernels with a start array (bit-equal results per window) */
int sync_find_frame_start_at_device(int fmt, gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                                   const void* samples, int64_t stream_len, const void* starts, int64_t n_windows, void* stream)
{
    int rc = check_at(h, samples, stream_len, starts, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    const SyncOut o = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (!o.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return sync_enqueue(h, list_args(h, samples, fmt, stream_len, static_cast<const int64_t*>(starts), n_windows, n_windows, 0), o, s);
    });
}

int sync_find_frame_start_at_host(int fmt, gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                                 const void* samples, int64_t stream_len, const int64_t* starts, int64_t n_windows)
{
    int rc = check_at(h, samples, stream_len, starts, n_windows);
    if (rc != GFDM_HIP_OK || n_windows == 0) return rc;
    const SyncOut host = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (!host.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    const int64_t n = n_windows;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(samples), (size_t)stream_len * sample_bytes(fmt));
    const auto st = hc.in(starts, (size_t)n);
    const SyncPieces o = sync_pieces(hc, host, n);
    return hc.run([&](hipStream_t s) { return sync_enqueue(h, list_args(h, x.dev(), fmt, stream_len, st.dev(), n, n, 0), o.dev(), s); });
}

int sync_detect_device(int fmt, gfdm_hip_burst_sync* h, void* count, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
                                      const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts,
                                      void* workspace, void* stream)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    int rc = detect_check(h->K, h->cp, h->W, stream_len, threshold, min_distance, lead, max_bursts);
    if (rc != GFDM_HIP_OK) return rc;
    if (!samples || !count || !workspace) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    const SyncOut o = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (max_bursts > 0 && !o.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    if (max_bursts > (int64_t)1 << 31) return api_fail(GFDM_HIP_EINVAL, "max_bursts above 2^31");
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return detect_enqueue(h, static_cast<int64_t*>(count), o, samples, fmt, stream_len, threshold, min_distance, lead, max_bursts, workspace, s);
    });
}

int sync_detect_host(int fmt, gfdm_hip_burst_sync* h, int64_t* count, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
                                    const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    int rc = detect_check(h->K, h->cp, h->W, stream_len, threshold, min_distance, lead, max_bursts);
    if (rc != GFDM_HIP_OK) return rc;
    if (!samples || !count) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    const SyncOut host = sync_out(frame_start, coarse, cfo, metric, sc_rot);
    if (max_bursts > 0 && !host.complete()) return api_fail(GFDM_HIP_EINVAL, "NULL output buffer");
    if (max_bursts > (int64_t)1 << 31) return api_fail(GFDM_HIP_EINVAL, "max_bursts above 2^31");
    const int64_t n = max_bursts;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(samples), (size_t)stream_len * sample_bytes(fmt));
    const auto ws = hc.scratch<unsigned char>(detect_geom(h, stream_len).bytes);
    const auto cnt = hc.out(count, 1);
    const SyncPieces o = sync_pieces(hc, host, n);
    return hc.run([&](hipStream_t s) {
        return detect_enqueue(h, cnt.dev(), o.dev(), x.dev(), fmt, stream_len, threshold, min_distance, lead, n, ws.dev(), s);
    });
}

int extractor_extract_device(int fmt, gfdm_hip_burst_extractor* h, void* out, const void* samples, int64_t stream_len, const void* offsets,
                                            const void* scale, const void* sc_rot, int64_t n_bursts, void* stream)
{
    int rc = extract_check(h, out, samples, stream_len, offsets, n_bursts);
    if (rc != GFDM_HIP_OK || n_bursts == 0) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return extract_enqueue(h, static_cast<cf*>(out), samples, fmt, stream_len, static_cast<const int64_t*>(offsets), static_cast<const float*>(scale),
                               static_cast<const cf*>(sc_rot), n_bursts, s);
    });
}

int extractor_extract_host(int fmt, gfdm_hip_burst_extractor* h, float* out, const void* samples, int64_t stream_len, const int64_t* offsets,
                                          const float* scale, const float* sc_rot, int64_t n_bursts)
{
    int rc = extract_check(h, out, samples, stream_len, offsets, n_bursts);
    if (rc != GFDM_HIP_OK || n_bursts == 0) return rc;
    const size_t n = (size_t)n_bursts;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(samples), (size_t)stream_len * sample_bytes(fmt));
    const auto off = hc.in(offsets, n);
    const auto rot = hc.in(reinterpret_cast<const cf*>(sc_rot), n);
    const auto sc = hc.in(scale, n);
    const auto y = hc.out(reinterpret_cast<cf*>(out), n * (size_t)h->burst_len);
    return hc.run([&](hipStream_t s) { return extract_enqueue(h, y.dev(), x.dev(), fmt, stream_len, off.dev(), sc.dev(), rot.dev(), n_bursts, s); });
}

}  // namespace

extern "C" {

int gfdm_hip_burst_sync_create(gfdm_hip_burst_sync** out, int fft_len, int cp_len, const float* core_preamble, int n_preamble, int64_t window_len, int device)
{
    const int K = fft_len;
    std::vector<float> pre;
    return gfdm::create_handle(out, device, [&](gfdm_hip_burst_sync& h) -> int {
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
        pre.resize(4 * K);
        for (int i = 0; i < 4 * K; ++i) pre[i] = (float)(core_preamble[i] * g);
        h.K = K;
        h.cp = cp_len;
        h.W = (int)window_len;
        return GFDM_HIP_OK;
    }, [&](gfdm_hip_burst_sync& h) {
        hipError_t err = hipMalloc(&h.d_preamble, pre.size() * sizeof(float));
        if (err == hipSuccess) err = hipMemcpy(h.d_preamble, pre.data(), pre.size() * sizeof(float), hipMemcpyHostToDevice);
        return err == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(err, "burst_sync_create");
    });
}

int gfdm_hip_burst_sync_destroy(gfdm_hip_burst_sync* h) { delete h; return GFDM_HIP_OK; }
int gfdm_hip_burst_sync_fft_len(const gfdm_hip_burst_sync* h) { return h ? h->K : GFDM_HIP_EINVAL; }
int gfdm_hip_burst_sync_cp_len(const gfdm_hip_burst_sync* h) { return h ? h->cp : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_burst_sync_window_len(const gfdm_hip_burst_sync* h) { return h ? h->W : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_burst_sync_corr_len(const gfdm_hip_burst_sync* h) { return h ? h->W - 2 * h->K : GFDM_HIP_EINVAL; }

int gfdm_hip_burst_sync_detect_check(int fft_len, int cp_len, int64_t window_len, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead,
                                     int64_t max_bursts)
{
    return detect_check(fft_len, cp_len, window_len, stream_len, threshold, min_distance, lead, max_bursts);
}

int64_t gfdm_hip_burst_sync_detect_workspace_bytes(const gfdm_hip_burst_sync* h, int64_t stream_len)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (stream_len < h->W) return api_fail(GFDM_HIP_EINVAL, "stream_len is shorter than window_len");
    if (stream_len > kMaxDetectLen) return api_fail(GFDM_HIP_EINVAL, "stream_len above 2^29 (split the capture into overlapping spans)");
    return (int64_t)detect_geom(h, stream_len).bytes;
}

int gfdm_hip_burst_extractor_create(gfdm_hip_burst_extractor** out, int burst_len, int tag_backoff, int activate_cfo_correction, int device)
{
    return gfdm::create_handle(out, device, [&](gfdm_hip_burst_extractor& h) -> int {
        if (burst_len < 1) return api_fail(GFDM_HIP_EINVAL, "burst_len must be >= 1");
        h.burst_len = burst_len;
        h.backoff = tag_backoff;
        h.correct = activate_cfo_correction ? 1 : 0;
        return GFDM_HIP_OK;
    });
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

/* the calls that read a capture and their sc16 twins (include/gfdm_hip.h) */
int gfdm_hip_burst_sync_find_frame_start_device(gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows, void* stream)
{
    return sync_find_frame_start_device(gfdm::SAMPLES_CF32, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, first, stride, n_windows, stream);
}
int gfdm_hip_burst_sync_find_frame_start_sc16_device(gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows, void* stream)
{
    return sync_find_frame_start_device(gfdm::SAMPLES_SC16, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, first, stride, n_windows, stream);
}
int gfdm_hip_burst_sync_find_frame_start_host(gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
    const float* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows)
{
    return sync_find_frame_start_host(gfdm::SAMPLES_CF32, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, first, stride, n_windows);
}
int gfdm_hip_burst_sync_find_frame_start_sc16_host(gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
    const int16_t* samples, int64_t stream_len, int64_t first, int64_t stride, int64_t n_windows)
{
    return sync_find_frame_start_host(gfdm::SAMPLES_SC16, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, first, stride, n_windows);
}
int gfdm_hip_burst_sync_auto_correlate_device(gfdm_hip_burst_sync* h, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
    int64_t stride, int64_t n_windows, void* stream)
{
    return sync_auto_correlate_device(gfdm::SAMPLES_CF32, h, ac, ic, samples, stream_len, first, stride, n_windows, stream);
}
int gfdm_hip_burst_sync_auto_correlate_sc16_device(gfdm_hip_burst_sync* h, void* ac, void* ic, const void* samples, int64_t stream_len, int64_t first,
    int64_t stride, int64_t n_windows, void* stream)
{
    return sync_auto_correlate_device(gfdm::SAMPLES_SC16, h, ac, ic, samples, stream_len, first, stride, n_windows, stream);
}
int gfdm_hip_burst_sync_auto_correlate_host(gfdm_hip_burst_sync* h, float* ac, float* ic, const float* samples, int64_t stream_len, int64_t first,
    int64_t stride, int64_t n_windows)
{
    return sync_auto_correlate_host(gfdm::SAMPLES_CF32, h, ac, ic, samples, stream_len, first, stride, n_windows);
}
int gfdm_hip_burst_sync_auto_correlate_sc16_host(gfdm_hip_burst_sync* h, float* ac, float* ic, const int16_t* samples, int64_t stream_len, int64_t first,
    int64_t stride, int64_t n_windows)
{
    return sync_auto_correlate_host(gfdm::SAMPLES_SC16, h, ac, ic, samples, stream_len, first, stride, n_windows);
}
int gfdm_hip_burst_sync_find_frame_start_at_device(gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, const void* starts, int64_t n_windows, void* stream)
{
    return sync_find_frame_start_at_device(gfdm::SAMPLES_CF32, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, starts, n_windows, stream);
}
int gfdm_hip_burst_sync_find_frame_start_at_sc16_device(gfdm_hip_burst_sync* h, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, const void* starts, int64_t n_windows, void* stream)
{
    return sync_find_frame_start_at_device(gfdm::SAMPLES_SC16, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, starts, n_windows, stream);
}
int gfdm_hip_burst_sync_find_frame_start_at_host(gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
    const float* samples, int64_t stream_len, const int64_t* starts, int64_t n_windows)
{
    return sync_find_frame_start_at_host(gfdm::SAMPLES_CF32, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, starts, n_windows);
}
int gfdm_hip_burst_sync_find_frame_start_at_sc16_host(gfdm_hip_burst_sync* h, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
    const int16_t* samples, int64_t stream_len, const int64_t* starts, int64_t n_windows)
{
    return sync_find_frame_start_at_host(gfdm::SAMPLES_SC16, h, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, starts, n_windows);
}
int gfdm_hip_burst_sync_detect_device(gfdm_hip_burst_sync* h, void* count, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts, void* workspace, void* stream)
{
    return sync_detect_device(gfdm::SAMPLES_CF32, h, count, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, threshold, min_distance, lead, max_bursts, workspace, stream);
}
int gfdm_hip_burst_sync_detect_sc16_device(gfdm_hip_burst_sync* h, void* count, void* frame_start, void* coarse, void* cfo, void* metric, void* sc_rot,
    const void* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts, void* workspace, void* stream)
{
    return sync_detect_device(gfdm::SAMPLES_SC16, h, count, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, threshold, min_distance, lead, max_bursts, workspace, stream);
}
int gfdm_hip_burst_sync_detect_host(gfdm_hip_burst_sync* h, int64_t* count, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric, float* sc_rot,
    const float* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts)
{
    return sync_detect_host(gfdm::SAMPLES_CF32, h, count, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, threshold, min_distance, lead, max_bursts);
}
int gfdm_hip_burst_sync_detect_sc16_host(gfdm_hip_burst_sync* h, int64_t* count, int64_t* frame_start, int64_t* coarse, float* cfo, float* metric,
    float* sc_rot, const int16_t* samples, int64_t stream_len, float threshold, int64_t min_distance, int64_t lead, int64_t max_bursts)
{
    return sync_detect_host(gfdm::SAMPLES_SC16, h, count, frame_start, coarse, cfo, metric, sc_rot, samples, stream_len, threshold, min_distance, lead, max_bursts);
}
int gfdm_hip_burst_extractor_extract_device(gfdm_hip_burst_extractor* h, void* out, const void* samples, int64_t stream_len, const void* offsets,
    const void* scale, const void* sc_rot, int64_t n_bursts, void* stream)
{
    return extractor_extract_device(gfdm::SAMPLES_CF32, h, out, samples, stream_len, offsets, scale, sc_rot, n_bursts, stream);
}
int gfdm_hip_burst_extractor_extract_sc16_device(gfdm_hip_burst_extractor* h, void* out, const void* samples, int64_t stream_len, const void* offsets,
    const void* scale, const void* sc_rot, int64_t n_bursts, void* stream)
{
    return extractor_extract_device(gfdm::SAMPLES_SC16, h, out, samples, stream_len, offsets, scale, sc_rot, n_bursts, stream);
}
int gfdm_hip_burst_extractor_extract_host(gfdm_hip_burst_extractor* h, float* out, const float* samples, int64_t stream_len, const int64_t* offsets,
    const float* scale, const float* sc_rot, int64_t n_bursts)
{
    return extractor_extract_host(gfdm::SAMPLES_CF32, h, out, samples, stream_len, offsets, scale, sc_rot, n_bursts);
}
int gfdm_hip_burst_extractor_extract_sc16_host(gfdm_hip_burst_extractor* h, float* out, const int16_t* samples, int64_t stream_len, const int64_t* offsets,
    const float* scale, const float* sc_rot, int64_t n_bursts)
{
    return extractor_extract_host(gfdm::SAMPLES_SC16, h, out, samples, stream_len, offsets, scale, sc_rot, n_bursts);
}

}  // extern "C"
