// Spectrum meter: the Welch PSD (averaged periodogram) and the power statistics (PAPR, CCDF) of a stream or of the bursts of a capture,
// accumulated in totals that stay on the device.  The contract is written out in include/gfdm_hip.h; the host geometry in gfdm_spectrum.h.
//
// PSD (k_spectrum_psd<A, SC16, AT>, nfft = 2^A): a lane always holds 16 samples of a segment, so a segment takes nfft / 16 lanes and a
// workgroup of 256 lanes runs 4096 / nfft segments side by side (one trip).  The transform is decimation in frequency out of the radix
// 2 .. 16 codelets of gfdm_dft.h (literal twiddles), the twiddles BETWEEN the passes come from a table of nfft roots made on the host in
// double precision.  Pass 1 needs no LDS: lane l loads x[l + (nfft / 16) r], r = 0 .. 15, straight from memory (neighbouring lanes read
// neighbouring samples, 8 bytes each, 4 in sc16: any alignment of one sample takes the same path), multiplies by the window and runs the
// radix-16 codelet.  The later passes cross LDS in place; the LAST pass stays in registers, where |X|^2 is added to the lane's 16 fp64
// bins.  The output of a decimation-in-frequency chain is digit reversed; nothing is reordered, a lane just knows the bins it holds.
//     nfft   passes        lanes / segment   segments / trip   LDS crossings
//     16     16            1                 256               0
//     32     16 . 2        2                 128               1
//     64     16 . 4        4                 64                1
//     128    16 . 8        8                 32                1
//     256    16 . 16       16                16                1
//     512    16 . 16 . 2   32                8                 2
//     1024   16 . 16 . 4   64                4                 2
//     2048   16 . 16 . 8   128               2                 2
//     4096   16 . 16 . 16  256               1                 2
// LDS: 4096 samples + one padding sample per 16 (element p lies at p + p / 16: the stride-16 reads of the last pass and the stride-256
// reads of the middle one both spread over the 64 banks) = 34 816 bytes, reused for the final sum over the side-by-side segments, + 2 KiB
// of flags: 36 880 bytes, four workgroups a CU.  VGPRs (hipcc -Rpass-analysis=kernel-resource-usage with the Makefile's flags, gfx950):
// 103 at nfft 16, 121 .. 128 at 32 .. 256 (16 samples + 16 fp64 bins + the codelet's temporaries), 211 .. 236 at 512 .. 4096 (the middle
// radix-16 pass keeps a second set of 16 samples alive): two waves a SIMD there; ScratchSize 0 in every one of the 36
// instantiations.  With hop < nfft the overlap is read again through the caches, not kept in LDS (DESIGN.md says why).
// A workgroup owns a contiguous run of segments (spectrum::Runs) and writes ONE partial row of nfft doubles; k_spectrum_sum adds the rows
// in ascending order into psd_sum and bumps the counters.  No float atomics anywhere.
// A segment with a non-finite sample, or with a product x w that overflows fp32, is found at load time; its lanes raise the segment's flag in LDS, read behind the barrier that the
// first LDS crossing needs anyway (nfft = 16: the lane is the segment).  Such a segment adds nothing and counts in bad_segments.
//
// Power (k_spectrum_power<SC16>): tiles of 2048 samples, 8 per lane; p = fadd_rn(fmul_rn(re, re), fmul_rn(im, im)); the histogram in LDS
// (64-bit integer atomics) and then one 64-bit atomic per non-zero bin, one atomic max for the peak, and power_sum as fp64 partials: a
// lane adds its 8 samples, six shuffle levels add the lanes of a wave, a wave adds its tiles in order, the four waves are added at the
// end, and k_spectrum_sum_power adds the workgroups in ascending order.
#include "../../include/gfdm_hip.h"
#include "gfdm_hostcall.h"
// No implicit contraction in this translation unit: which of two products the compiler fuses into a sum may differ from one template
// instantiation to the next, and the sc16 kernels must be bit-equal to the complex64 ones.  Every fused multiply-add below is an fmaf.
#pragma clang fp contract(off)
#include "gfdm_dft.h"
#include "gfdm_spectrum.h"

#include <algorithm>
#include <cmath>
#include <vector>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::DeviceGuard;
using gfdm::misaligned;
namespace sp = gfdm::spectrum;
namespace dft = gfdm::dft;

namespace {

typedef unsigned long long u64;

constexpr int kLanes = sp::kLanes;
constexpr int kPadSamples = sp::kSlotSamples + sp::kSlotSamples / 16;      // 4352
enum { H_SEGMENTS, H_BAD_SEGMENTS, H_SAMPLES, H_BAD_SAMPLES, H_PEAK_BITS };

// the totals of a handle on the device: head int64[8] | power_sum double | psd_sum double[nfft] | hist int64[512]
struct Totals {
    u64* head;
    double* power_sum;
    double* psd_sum;
    u64* hist;
};

size_t totals_bytes(int nfft) { return (size_t)(sp::kHeadFields + 1 + nfft + sp::kHistBins) * 8; }

Totals totals_at(unsigned char* base, int nfft)
{
    Totals t;
    t.head = reinterpret_cast<u64*>(base);
    t.power_sum = reinterpret_cast<double*>(base) + sp::kHeadFields;
    t.psd_sum = t.power_sum + 1;
    t.hist = reinterpret_cast<u64*>(t.psd_sum + nfft);
    return t;
}

struct PsdArgs {
    const void* in;                  // complex64 or sc16 samples
    const float* window;             // [nfft]
    const cf* roots;                 // [nfft]: exp(-2 pi j e / nfft)
    double* part;                    // [groups][nfft]
    u64* part_counts;                // [groups][2]: segments, bad_segments
    int64_t total, hop;              // segments of the call
    const int64_t* starts;           // accumulate_at: [n_bursts] and the optional count
    const int64_t* count;
    int64_t stream_len, first, seg_per_burst, n_bursts;
};

template <int SC16>
__device__ __forceinline__ cf load_sample(const void* in, int64_t i)
{
    if constexpr (SC16) {
        const unsigned v = static_cast<const unsigned*>(in)[i];              // I in the low half, Q in the high one
        return make_float2((float)(short)(v & 0xffffu), (float)(short)(v >> 16));
    } else {
        return static_cast<const cf*>(in)[i];
    }
}

__device__ __forceinline__ int padded(int p) { return p + (p >> 4); }

// a b and |v|^2 with the fusion written out, and the power of a sample in two rounded products and a rounded sum.  Each states the
// contraction rule in its own body as well, so that none depends on where the file-scope pragma sits.  (hipcc inlines __fmul_rn /
// __fadd_rn as plain operators that carry their header's contract flag, and fused them: seen on the MI355X as a last-bit difference to
// numpy.  Hence plain operators with contraction off.)
__device__ __forceinline__ cf cmul_fixed(cf a, cf b)
{
#pragma clang fp contract(off)
    const float t0 = a.y * b.y, t1 = a.y * b.x;
    return make_float2(fmaf(a.x, b.x, -t0), fmaf(a.x, b.y, t1));
}
__device__ __forceinline__ float norm2(cf v)
{
#pragma clang fp contract(off)
    const float t = v.y * v.y;
    return fmaf(v.x, v.x, t);
}
__device__ __forceinline__ float sample_power(cf v)
{
#pragma clang fp contract(off)
    const float re2 = v.x * v.x, im2 = v.y * v.y;
    return re2 + im2;
}

// One pass across LDS of the segment at xs (nfft = N samples, N / 16 lanes, this is lane l): radix R, sub-transforms of length R S.  A lane
// runs 16 / R butterflies; butterfly q takes the elements base + S r, base = (q / S) R S + q % S.  Not LAST: the results go back in place,
// times the roots of the pass.  LAST (S = 1): they go to emit(q, k, value).
template <int N, int R, int S, bool LAST, class F>
__device__ __forceinline__ void lds_pass(cf* xs, int l, const cf* roots, F&& emit)
{
    constexpr int LPS = N / 16, U = 16 / R;
    dft::static_for<0, U>([&](auto ui) {
        constexpr int u = decltype(ui)::value;
        const int q = l + LPS * u;
        const int s = q % S, base = (q / S) * (R * S) + s;
        cf t[R];
        dft::static_for<0, R>([&](auto ri) { constexpr int r = decltype(ri)::value; t[r] = xs[padded(base + S * r)]; });
        dft::dft_inplace<R, false>(t);
        dft::static_for<0, R>([&](auto ki) {
            constexpr int k = decltype(ki)::value;
            if constexpr (LAST) {
                emit(q, k, u * R + k, t[k]);
            } else {
                const cf y = k == 0 ? t[0] : cmul_fixed(t[k], roots[(N / (R * S)) * s * k]);
                xs[padded(base + S * k)] = y;
            }
        });
    });
}

// AT = 0: segment t of a stream starts at t hop.  AT = 1: segment t = b seg_per_burst + j of a capture starts at starts[b] + first + j hop,
// where it is live.  -1: not live.
template <int AT>
__device__ __forceinline__ int64_t origin_of(const PsdArgs& a, int64_t t, int64_t n_live, int nfft)
{
    if constexpr (AT) {
        const int64_t b = t / a.seg_per_burst, j = t - b * a.seg_per_burst;
        if (b >= n_live) return -1;
        return sp::burst_origin(a.starts[b], a.first, j, a.hop, nfft, a.stream_len);
    } else {
        return t * a.hop;
    }
}

template <int A, int SC16, int AT>
__global__ __launch_bounds__(kLanes) void k_spectrum_psd(PsdArgs a)
{
    constexpr int N = 1 << A, LPS = N / 16, SLOTS = sp::kSlotSamples / N;
    constexpr int PASSES = A == 4 ? 1 : A <= 8 ? 2 : 3;
    constexpr int R2 = PASSES == 1 ? 1 : PASSES == 2 ? N / 16 : 16, R3 = PASSES == 3 ? N / 256 : 1;
    __shared__ double s_raw[kPadSamples];                                   // the samples between the passes (cf), then the sums (double)
    __shared__ int s_bad[2][kLanes];
    __shared__ u64 s_count[2];
    cf* const all = reinterpret_cast<cf*>(s_raw);
    const int tid = threadIdx.x, slot = tid / LPS, l = tid % LPS;
    cf* const xs = all + slot * (N + N / 16);
    s_bad[0][tid] = 0;
    s_bad[1][tid] = 0;
    if (tid < 2) s_count[tid] = 0;
    __syncthreads();
    const sp::Runs runs(a.total, N);
    const int64_t seg_lo = runs.lo(blockIdx.x), seg_hi = runs.hi(blockIdx.x);
    int64_t n_live = 0;
    if constexpr (AT) {
        // clamped on a loaded value: std::min / std::max return references, and a choice between one into memory and temporaries put the
        // temporaries into scratch
        const int64_t c = a.count ? *a.count : a.n_bursts;
        n_live = c < 0 ? 0 : c < a.n_bursts ? c : a.n_bursts;
    }
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.;
    unsigned good = 0, bad = 0;
    int parity = 0;
    for (int64_t t0 = seg_lo; t0 < seg_hi; t0 += SLOTS, parity ^= 1) {
        const int64_t t = t0 + slot;
        const int64_t o = t < seg_hi ? origin_of<AT>(a, t, n_live, N) : -1;
        const bool live = o >= 0;
        // ---- pass 1, out of memory: x[l + LPS r] w[l + LPS r], the radix-16 codelet, the roots W_N^(l k) ----
        cf x[16];
        bool nonfinite = false;
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = load_sample<SC16>(a.in, o + l + LPS * r);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float w = a.window[l + LPS * r];
                x[r] = make_float2(x[r].x * w, x[r].y * w);
                nonfinite |= !(isfinite(x[r].x) && isfinite(x[r].y));        // the sample was not finite, or its product overflows fp32
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = make_float2(0.f, 0.f);
        }
        dft::dft_inplace<16, false>(x);
        bool bad_segment = nonfinite;
        if constexpr (PASSES == 1) {
            if (live && !bad_segment) {
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] += (double)norm2(x[k]);
            }
        } else {
            if (nonfinite) s_bad[parity][slot] = 1;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const cf y = k == 0 ? x[0] : cmul_fixed(x[k], a.roots[l * k]);
                xs[padded(l + LPS * k)] = y;
            }
            __syncthreads();
            bad_segment = s_bad[parity][slot] != 0;
            if (l == 0) s_bad[parity ^ 1][slot] = 0;                         // read last in the trip before, raised next behind the barrier below
            const bool counted = live && !bad_segment;
            auto emit = [&](int, int, int reg, cf v) { acc[reg] += counted ? (double)norm2(v) : 0.; };
            if constexpr (PASSES == 2) {
                lds_pass<N, R2, 1, true>(xs, l, a.roots, emit);
            } else {
                lds_pass<N, R2, R3, false>(xs, l, a.roots, emit);
                __syncthreads();
                lds_pass<N, R3, 1, true>(xs, l, a.roots, emit);
            }
            __syncthreads();                                                 // xs is rewritten in the next trip
        }
        if (l == 0 && live) {
            good += !bad_segment;
            bad += bad_segment;
        }
    }
    // ---- the workgroup's partial row: the segments that ran side by side, added in ascending slot order, bin by bin ----
    double* const sums = s_raw;                                              // [SLOTS][N]
    {
        constexpr int RL = PASSES == 1 ? 16 : PASSES == 2 ? R2 : R3, U = 16 / RL;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int u = reg / RL, k = reg % RL, q = l + LPS * u;
            // the bin of (butterfly q of the last pass, output k): the digits of a decimation-in-frequency chain, reversed
            const int bin = PASSES == 1 ? k : PASSES == 2 ? q + 16 * k : q / 16 + 16 * (q % 16) + 256 * k;
            sums[slot * N + bin] = acc[reg];
        }
        (void)U;
    }
    if (l == 0) {
        if (good) atomicAdd(&s_count[0], (u64)good);
        if (bad) atomicAdd(&s_count[1], (u64)bad);
    }
    __syncthreads();
    for (int k = tid; k < N; k += kLanes) {
        double s = 0.;
        for (int j = 0; j < SLOTS; ++j) s += sums[j * N + k];
        a.part[(int64_t)blockIdx.x * N + k] = s;
    }
    if (tid < 2) a.part_counts[2 * blockIdx.x + tid] = s_count[tid];
}

// psd_sum[k] += the partial rows in ascending order; the two counters
// A workgroup takes kSumBins bins: the 256 lanes bring kSumRows rows of them to LDS at a time (the loads are independent and in flight
// together), then one lane per bin adds them in ascending row order.  (One lane per bin straight out of memory waited a memory latency
// per row: 345 us for 1024 rows, longer than the transform itself; profiles/r22/spectrum_kernel_durations.txt has the figure now.)
constexpr int kSumBins = 16, kSumRows = 256;

__global__ __launch_bounds__(kLanes) void k_spectrum_sum(const double* part, const u64* part_counts, int groups, int nfft, Totals t)
{
    __shared__ double tile[kSumRows * kSumBins];
    const int tid = threadIdx.x, bin = tid & (kSumBins - 1), b0 = blockIdx.x * kSumBins;
    double s = 0.;
    for (int g0 = 0; g0 < groups; g0 += kSumRows) {
        const int rows = min(kSumRows, groups - g0);
#pragma unroll
        for (int i = 0; i < kSumRows * kSumBins / kLanes; ++i) {
            const int row = (tid >> 4) + (kLanes / kSumBins) * i;
            if (row < rows) tile[row * kSumBins + bin] = part[(int64_t)(g0 + row) * nfft + b0 + bin];
        }
        __syncthreads();
        if (tid < kSumBins)
            for (int r = 0; r < rows; ++r) s += tile[r * kSumBins + tid];
        __syncthreads();
    }
    if (tid < kSumBins) t.psd_sum[b0 + tid] += s;
    if (blockIdx.x == 0) {                                                   // the two counters: integers, any order
        u64 c[2] = { 0, 0 };
        for (int g = tid; g < groups; g += kLanes) {
            c[0] += part_counts[2 * g];
            c[1] += part_counts[2 * g + 1];
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c[f] += __shfl_xor(c[f], d);
            if ((tid & 63) == 0 && c[f]) atomicAdd(&t.head[f == 0 ? H_SEGMENTS : H_BAD_SEGMENTS], c[f]);
        }
    }
}

struct PowerArgs {
    const void* in;
    int64_t n;
    double* part;                    // [groups]
    Totals t;
};

template <int SC16>
__global__ __launch_bounds__(kLanes) void k_spectrum_power(PowerArgs a)
{
    __shared__ u64 s_hist[sp::kHistBins];
    __shared__ double s_wave[kLanes / 64];
    __shared__ u64 s_count[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = tid; b < sp::kHistBins; b += kLanes) s_hist[b] = 0;
    if (tid < 3) s_count[tid] = 0;
    __syncthreads();
    const sp::PowerRuns runs(a.n);
    const int64_t tile_lo = (int64_t)blockIdx.x * runs.per, tile_hi = std::min(tile_lo + runs.per, runs.tiles);
    u64 n_ok = 0, n_bad = 0;
    unsigned peak = 0;
    double wave_sum = 0.;                                                    // the wave's tiles so far, in tile order (every lane holds it)
    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        const int64_t i0 = tile * sp::kPowerTile + tid;
        cf x[sp::kPowerPer];
#pragma unroll
        for (int u = 0; u < sp::kPowerPer; ++u) {
            const int64_t i = i0 + u * kLanes;
            x[u] = i < a.n ? load_sample<SC16>(a.in, i) : make_float2(0.f, 0.f);
        }
        double lane_sum = 0.;
#pragma unroll
        for (int u = 0; u < sp::kPowerPer; ++u) {
            if (i0 + u * kLanes >= a.n) continue;
            const float p = sample_power(x[u]);
            const unsigned bits = __float_as_uint(p);
            if ((bits & 0x7f800000u) == 0x7f800000u) {                       // inf or NaN
                ++n_bad;
                continue;
            }
            ++n_ok;
            peak = max(peak, bits);                                          // p >= +0: floats order as their bits
            const int bin = min(max((int)(bits >> 20) - sp::kHistBias, 0), sp::kHistBins - 1);
            atomicAdd(&s_hist[bin], (u64)1);
            lane_sum += (double)p;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lane_sum += __shfl_xor(lane_sum, d);
        wave_sum += lane_sum;
    }
    if (lane == 0) s_wave[wave] = wave_sum;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n_ok += __shfl_xor(n_ok, d);
        n_bad += __shfl_xor(n_bad, d);
        peak = max(peak, (unsigned)__shfl_xor((int)peak, d));
    }
    if (lane == 0) {
        if (n_ok) atomicAdd(&s_count[0], n_ok);
        if (n_bad) atomicAdd(&s_count[1], n_bad);
        atomicMax(&s_count[2], (u64)peak);
    }
    __syncthreads();
    for (int b = tid; b < sp::kHistBins; b += kLanes)
        if (s_hist[b]) atomicAdd(&a.t.hist[b], s_hist[b]);
    if (tid == 0) {
        a.part[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (s_count[0]) atomicAdd(&a.t.head[H_SAMPLES], s_count[0]);
        if (s_count[1]) atomicAdd(&a.t.head[H_BAD_SAMPLES], s_count[1]);
        if (s_count[2]) atomicMax(&a.t.head[H_PEAK_BITS], s_count[2]);
    }
}

// power_sum += the workgroups' partials in ascending order
__global__ __launch_bounds__(kLanes) void k_spectrum_sum_power(const double* part, int groups, Totals t)
{
    __shared__ double p[sp::kPowerGroups];
    for (int g = threadIdx.x; g < groups; g += kLanes) p[g] = part[g];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.;
    for (int g = 0; g < groups; ++g) s += p[g];
    *t.power_sum += s;
}

__global__ __launch_bounds__(kLanes) void k_spectrum_reset(u64* words, int n)
{
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i < n) words[i] = 0;                                                 // (+0.0 is all zero bits)
}

}  // namespace

struct gfdm_hip_spectrum_meter {
    gfdm::DeviceCtx ctx;
    int nfft = 0;
    int64_t hop = 0;
    std::vector<float> window;
    float* d_window = nullptr;
    cf* d_roots = nullptr;
    unsigned char* d_totals = nullptr;
    double* d_part = nullptr;        // [kMaxGroups][nfft]
    u64* d_part_counts = nullptr;    // [kMaxGroups][2]
    double* d_power_part = nullptr;  // [kPowerGroups]
    ~gfdm_hip_spectrum_meter()
    {
        if (!d_window && !d_roots && !d_totals && !d_part && !d_part_counts && !d_power_part) return;
        DeviceGuard guard(ctx.device);
        (void)hipFree(d_window);
        (void)hipFree(d_roots);
        (void)hipFree(d_totals);
        (void)hipFree(d_part);
        (void)hipFree(d_part_counts);
        (void)hipFree(d_power_part);
    }
};

namespace {

template <int A, int SC16>
void launch_psd(bool at, unsigned grid, hipStream_t s, const PsdArgs& a)
{
    if (at) hipLaunchKernelGGL((k_spectrum_psd<A, SC16, 1>), dim3(grid), dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL((k_spectrum_psd<A, SC16, 0>), dim3(grid), dim3(kLanes), 0, s, a);
}

template <int SC16>
void launch_psd(int log2n, bool at, unsigned grid, hipStream_t s, const PsdArgs& a)
{
    switch (log2n) {
    case 4: launch_psd<4, SC16>(at, grid, s, a); break;
    case 5: launch_psd<5, SC16>(at, grid, s, a); break;
    case 6: launch_psd<6, SC16>(at, grid, s, a); break;
    case 7: launch_psd<7, SC16>(at, grid, s, a); break;
    case 8: launch_psd<8, SC16>(at, grid, s, a); break;
    case 9: launch_psd<9, SC16>(at, grid, s, a); break;
    case 10: launch_psd<10, SC16>(at, grid, s, a); break;
    case 11: launch_psd<11, SC16>(at, grid, s, a); break;
    default: launch_psd<12, SC16>(at, grid, s, a); break;
    }
}

// the two launches of an accumulate call over `total` segments.  Everything is a device pointer.
int psd_enqueue(const gfdm_hip_spectrum_meter* m, int sc16, bool at, PsdArgs a, hipStream_t s)
{
    if (a.total == 0) return GFDM_HIP_OK;
    if (misaligned(a.in, sc16 ? 4 : 8) || misaligned(a.starts, 8) || misaligned(a.count, 8)) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    a.window = m->d_window;
    a.roots = m->d_roots;
    a.part = m->d_part;
    a.part_counts = m->d_part_counts;
    a.hop = m->hop;
    const sp::Runs runs(a.total, m->nfft);
    if (sc16) launch_psd<1>(sp::log2_of(m->nfft), at, (unsigned)runs.groups, s, a);
    else launch_psd<0>(sp::log2_of(m->nfft), at, (unsigned)runs.groups, s, a);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_spectrum_sum, dim3((unsigned)(m->nfft / kSumBins)), dim3(kLanes), 0, s, m->d_part, m->d_part_counts, runs.groups, m->nfft,
                       totals_at(m->d_totals, m->nfft));
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int power_enqueue(const gfdm_hip_spectrum_meter* m, int sc16, const void* in, int64_t n, hipStream_t s)
{
    if (n == 0) return GFDM_HIP_OK;
    if (misaligned(in, sc16 ? 4 : 8)) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const sp::PowerRuns runs(n);
    const PowerArgs a = { in, n, m->d_power_part, totals_at(m->d_totals, m->nfft) };
    if (sc16) hipLaunchKernelGGL(k_spectrum_power<1>, dim3((unsigned)runs.groups), dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(k_spectrum_power<0>, dim3((unsigned)runs.groups), dim3(kLanes), 0, s, a);
    GFDM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_spectrum_sum_power, dim3(1), dim3(kLanes), 0, s, m->d_power_part, runs.groups, a.t);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int stream_check(const gfdm_hip_spectrum_meter* m, const void* in, int64_t n)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (const char* msg = sp::check_stream(n)) return api_fail(GFDM_HIP_EINVAL, msg);
    if (n > 0 && !in) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

PsdArgs stream_args(const void* in, int64_t total)
{
    PsdArgs a = {};
    a.in = in;
    a.total = total;
    return a;
}

// both flavours of accumulate and of power: n samples at `in`
int stream_call(gfdm_hip_spectrum_meter* m, bool host, int sc16, bool power, const void* in, int64_t n, void* stream)
{
    const int rc = stream_check(m, in, n);
    if (rc != GFDM_HIP_OK) return rc;
    const int64_t total = power ? n : sp::segments_of(m->nfft, m->hop, n);
    if (total == 0) return GFDM_HIP_OK;
    auto enqueue = [&](const void* x, hipStream_t s) { return power ? power_enqueue(m, sc16, x, n, s) : psd_enqueue(m, sc16, false, stream_args(x, total), s); };
    if (!host) return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) { return enqueue(in, s); });
    gfdm::HostCall hc(m->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(in), (size_t)n * gfdm::sample_bytes(sc16 ? gfdm::SAMPLES_SC16 : gfdm::SAMPLES_CF32));
    return hc.run([&](hipStream_t s) { return enqueue(x.dev(), s); });
}

int at_call(gfdm_hip_spectrum_meter* m, bool host, int sc16, const void* in, int64_t stream_len, const void* starts, const void* count, int64_t first,
            int64_t seg_per_burst, int64_t n_bursts, void* stream)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (const char* msg = sp::check_bursts(stream_len, first, seg_per_burst, n_bursts)) return api_fail(GFDM_HIP_EINVAL, msg);
    const int64_t total = seg_per_burst * n_bursts;
    if (total == 0) return GFDM_HIP_OK;
    if (!starts || (stream_len > 0 && !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    PsdArgs a = {};
    a.total = total;
    a.stream_len = stream_len;
    a.first = first;
    a.seg_per_burst = seg_per_burst;
    a.n_bursts = n_bursts;
    if (!host) {
        a.in = in;
        a.starts = static_cast<const int64_t*>(starts);
        a.count = static_cast<const int64_t*>(count);
        return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) { return psd_enqueue(m, sc16, true, a, s); });
    }
    gfdm::HostCall hc(m->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(in), (size_t)stream_len * gfdm::sample_bytes(sc16 ? gfdm::SAMPLES_SC16 : gfdm::SAMPLES_CF32));
    const auto st = hc.in(static_cast<const int64_t*>(starts), (size_t)n_bursts);
    const auto cnt = hc.in(static_cast<const int64_t*>(count), 1);
    return hc.run([&](hipStream_t s) {
        a.in = x.dev();
        a.starts = st.dev();
        a.count = cnt.dev();
        return psd_enqueue(m, sc16, true, a, s);
    });
}

}  // namespace

extern "C" {

int gfdm_hip_spectrum_meter_plan(int nfft, int64_t hop, int64_t n, int64_t* n_seg, int64_t* advance)
{
    if (const char* msg = sp::check_shape(nfft, hop)) return api_fail(GFDM_HIP_EINVAL, msg);
    if (const char* msg = sp::check_stream(n)) return api_fail(GFDM_HIP_EINVAL, msg);
    const int64_t s = sp::segments_of(nfft, hop, n);
    if (n_seg) *n_seg = s;
    if (advance) *advance = s * hop;
    return GFDM_HIP_OK;
}

int gfdm_hip_spectrum_meter_create(gfdm_hip_spectrum_meter** out, const float* window, int nfft, int64_t hop, int device)
{
    return gfdm::create_handle(
        out, device,
        [&](gfdm_hip_spectrum_meter& h) -> int {
            if (const char* msg = sp::check_shape(nfft, hop)) return api_fail(GFDM_HIP_EINVAL, msg);
            if (!window) return api_fail(GFDM_HIP_EINVAL, "NULL window");
            for (int i = 0; i < nfft; ++i)
                if (!std::isfinite(window[i])) return api_fail(GFDM_HIP_EINVAL, "the window holds a non-finite value");
            h.nfft = nfft;
            h.hop = hop;
            h.window.assign(window, window + nfft);
            return GFDM_HIP_OK;
        },
        [](gfdm_hip_spectrum_meter& h) -> int {
            const int n = h.nfft;
            std::vector<cf> roots((size_t)n);
            for (int e = 0; e < n; ++e) {
                // exact at the quarter turns
                const int o = (int)(((int64_t)8 * e) / n);
                const bool on_octant = ((int64_t)8 * e) % n == 0;
                const double ang = -2.0 * 3.141592653589793238462643383279502884 * (double)e / (double)n;
                double c = std::cos(ang), s = std::sin(ang);
                if (on_octant && o % 2 == 0) {
                    const double cs[4] = { 1., 0., -1., 0. }, sn[4] = { 0., -1., 0., 1. };
                    c = cs[o / 2];
                    s = sn[o / 2];
                }
                roots[(size_t)e] = make_float2((float)c, (float)s);
            }
            const size_t tb = totals_bytes(n);
            hipError_t e = hipMalloc(&h.d_window, (size_t)n * sizeof(float));
            if (e == hipSuccess) e = hipMalloc(&h.d_roots, (size_t)n * sizeof(cf));
            if (e == hipSuccess) e = hipMalloc(&h.d_totals, tb);
            if (e == hipSuccess) e = hipMalloc(&h.d_part, (size_t)sp::kMaxGroups * (size_t)n * sizeof(double));
            if (e == hipSuccess) e = hipMalloc(&h.d_part_counts, (size_t)sp::kMaxGroups * 2 * sizeof(u64));
            if (e == hipSuccess) e = hipMalloc(&h.d_power_part, (size_t)sp::kPowerGroups * sizeof(double));
            if (e == hipSuccess) e = hipMemcpy(h.d_window, h.window.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(h.d_roots, roots.data(), (size_t)n * sizeof(cf), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemset(h.d_totals, 0, tb);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "spectrum meter tables");
        });
}

int gfdm_hip_spectrum_meter_destroy(gfdm_hip_spectrum_meter* m) { delete m; return GFDM_HIP_OK; }
int gfdm_hip_spectrum_meter_nfft(const gfdm_hip_spectrum_meter* m) { return m ? m->nfft : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_spectrum_meter_hop(const gfdm_hip_spectrum_meter* m) { return m ? m->hop : GFDM_HIP_EINVAL; }
int gfdm_hip_spectrum_meter_window(const gfdm_hip_spectrum_meter* m, float* window)
{
    if (!m || !window) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    std::copy(m->window.begin(), m->window.end(), window);
    return GFDM_HIP_OK;
}

void* gfdm_hip_spectrum_meter_totals_device(gfdm_hip_spectrum_meter* m) { return m ? m->d_totals : nullptr; }
int64_t gfdm_hip_spectrum_meter_totals_bytes(const gfdm_hip_spectrum_meter* m) { return m ? (int64_t)totals_bytes(m->nfft) : GFDM_HIP_EINVAL; }

int gfdm_hip_spectrum_meter_reset(gfdm_hip_spectrum_meter* m, void* stream)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) -> int {
        const int words = (int)(totals_bytes(m->nfft) / 8);
        hipLaunchKernelGGL(k_spectrum_reset, dim3((unsigned)((words + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, reinterpret_cast<u64*>(m->d_totals), words);
        GFDM_TRY(hipGetLastError());
        return GFDM_HIP_OK;
    });
}

int gfdm_hip_spectrum_meter_read(gfdm_hip_spectrum_meter* m, int64_t* head, double* power_sum, double* psd_sum, int64_t* hist, void* stream)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) -> int {
        GFDM_TRY(hipStreamSynchronize(s));
        const Totals t = totals_at(m->d_totals, m->nfft);
        if (head) GFDM_TRY(hipMemcpy(head, t.head, sp::kHeadFields * 8, hipMemcpyDeviceToHost));
        if (power_sum) GFDM_TRY(hipMemcpy(power_sum, t.power_sum, 8, hipMemcpyDeviceToHost));
        if (psd_sum) GFDM_TRY(hipMemcpy(psd_sum, t.psd_sum, (size_t)m->nfft * 8, hipMemcpyDeviceToHost));
        if (hist) GFDM_TRY(hipMemcpy(hist, t.hist, sp::kHistBins * 8, hipMemcpyDeviceToHost));
        return GFDM_HIP_OK;
    });
}

int gfdm_hip_spectrum_meter_accumulate_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t n) { return stream_call(m, true, 0, false, in, n, nullptr); }
int gfdm_hip_spectrum_meter_accumulate_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream)
{
    return stream_call(m, false, 0, false, in, n, stream);
}
int gfdm_hip_spectrum_meter_accumulate_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t n) { return stream_call(m, true, 1, false, in, n, nullptr); }
int gfdm_hip_spectrum_meter_accumulate_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream)
{
    return stream_call(m, false, 1, false, in, n, stream);
}

int gfdm_hip_spectrum_meter_power_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t n) { return stream_call(m, true, 0, true, in, n, nullptr); }
int gfdm_hip_spectrum_meter_power_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream) { return stream_call(m, false, 0, true, in, n, stream); }
int gfdm_hip_spectrum_meter_power_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t n) { return stream_call(m, true, 1, true, in, n, nullptr); }
int gfdm_hip_spectrum_meter_power_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t n, void* stream)
{
    return stream_call(m, false, 1, true, in, n, stream);
}

int gfdm_hip_spectrum_meter_accumulate_at_host(gfdm_hip_spectrum_meter* m, const float* in, int64_t stream_len, const int64_t* starts, const int64_t* count,
                                               int64_t first, int64_t seg_per_burst, int64_t n_bursts)
{
    return at_call(m, true, 0, in, stream_len, starts, count, first, seg_per_burst, n_bursts, nullptr);
}
int gfdm_hip_spectrum_meter_accumulate_at_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t stream_len, const void* starts, const void* count, int64_t first,
                                                 int64_t seg_per_burst, int64_t n_bursts, void* stream)
{
    return at_call(m, false, 0, in, stream_len, starts, count, first, seg_per_burst, n_bursts, stream);
}
int gfdm_hip_spectrum_meter_accumulate_at_sc16_host(gfdm_hip_spectrum_meter* m, const int16_t* in, int64_t stream_len, const int64_t* starts, const int64_t* count,
                                                    int64_t first, int64_t seg_per_burst, int64_t n_bursts)
{
    return at_call(m, true, 1, in, stream_len, starts, count, first, seg_per_burst, n_bursts, nullptr);
}
int gfdm_hip_spectrum_meter_accumulate_at_sc16_device(gfdm_hip_spectrum_meter* m, const void* in, int64_t stream_len, const void* starts, const void* count,
                                                      int64_t first, int64_t seg_per_burst, int64_t n_bursts, void* stream)
{
    return at_call(m, false, 1, in, stream_len, starts, count, first, seg_per_burst, n_bursts, stream);
}

}  // extern "C"
