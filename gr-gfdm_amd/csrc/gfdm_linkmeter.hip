// Link meter behind the receivers: which sent burst a detection is (match), bit / symbol / row errors and the error-vector power of every
// row against the sent payload or against the decisions themselves (measure), and twelve 64-bit counters that stay on the device and
// add up over the calls of a curve point.  The contract is written out in include/gfdm_hip.h.
//
// measure is memory bound and keeps the shape of the mapper's decode (gfdm_symbols.hip): the flat symbol array is tiled, never the rows
// -- a tile is kTileSyms = 2048 symbols whatever rows lie there -- the loads are 16-byte vectors aligned in memory, the point table sits
// in LDS and the decision is decode's own device function (gfdm_decide.h).  A lane decides its symbols, reads the sent index out of the
// packed payload, and leaves |x - p|^2, |p|^2 and the popcount of idx ^ sent per symbol in LDS.  Then the tile reduces BY ROW: lane t
// walks the eight contiguous symbols 8 t .. 8 t + 7 in order (a row that begins and ends there is done), the open ends go through a
// segmented scan over the 256 lanes (six shuffle levels inside a wave, the four wave totals through LDS), and a row that ends in a
// lane but began in an earlier one takes the scan's carry.  All of it is fp32 in a fixed order.  A row that crosses a tile boundary
// leaves a partial record (fp64 sums) per tile, at most two per tile, and a second small kernel adds the records of every crossing row
// in ascending tile order: the store pass plus a per-destination sum pass, so two calls on the same inputs agree to the bit and no
// kernel ever waits for another workgroup.  Integer totals: per lane, per wave, per workgroup, then one 64-bit atomic per field.
// match is not hot: initialise one 64-bit key per sent burst, one lane per detection (binary search, atomicMin of (distance << 32) | d),
// resolve.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"
#include "gfdm_rowtile.h"

#include <algorithm>
#include <climits>

using gfdm::cf;
using gfdm::api_fail;
using gfdm::DeviceGuard;
using gfdm::row_bytes_of;
using gfdm::live_rows;
using gfdm::misaligned;
using gfdm::RowPos;
using gfdm::advance;
using gfdm::dist2;
using gfdm::decide2;

namespace {

constexpr int kLanes = 256;
constexpr int kPerLane = 8;                               // contiguous symbols a lane walks in the row reduction
constexpr int kTileSyms = kLanes * kPerLane;              // 2048 symbols per tile
constexpr int kMaxTiles = 8192;                           // workgroups per launch; the tiles beyond are strided over
constexpr int kLoads = (kTileSyms / 2 + 1 + kLanes - 1) / kLanes;      // vectors per lane: 1024, + 1 where the buffer is only 8-byte aligned
constexpr int kPadSlots = kTileSyms + kLanes;             // slot + slot / 8: the lanes' walks hit different LDS banks
constexpr int64_t kMaxIndex = (int64_t)1 << 31;
constexpr int kUnmeasured = 0xff;                        // in place of a symbol's bit errors (at most 8)

enum { T_ROWS, T_SYMBOLS, T_BITS, T_BIT_ERRORS, T_SYMBOL_ERRORS, T_ROW_ERRORS, T_DETECTIONS, T_MATCHED, T_MISSED, T_FALSE_ALARMS, T_FIELDS = 12 };

typedef unsigned long long u64;

struct Partial { double e, q; int32_t be, se; };          // what a tile knows of a row that crosses its boundary: 24 bytes

struct MeasureArgs {
    const cf* points;                // [1 << k] (device)
    const cf* sym;                   // [n_rows][n_sym]
    const unsigned char* payload;    // optional: [n_ref][row_bytes]; NULL = decision-directed
    const int64_t* ref_row;          // optional: [n_rows]; NULL = the identity
    const int64_t* count;            // optional: live rows = clamp(*count, 0, n_rows)
    int64_t n_sym, n_rows, n_ref, row_bytes;
    int32_t* bit_errors;             // optional outputs, [n_rows] each
    float* err_power;
    float* ref_power;
    Partial* part;                   // [ntiles][2]: [0] the row that began before the tile, [1] the row that began in it and ends behind it
    u64* totals;
};

// the payload row of row r, or -1 where r is not measured
__device__ __forceinline__ int64_t ref_of(const MeasureArgs& a, int64_t r, int64_t n_live)
{
    if (r >= n_live) return -1;
    const int64_t j = a.ref_row ? a.ref_row[r] : r;
    if (j < 0 || (a.payload && j >= a.n_ref)) return -1;
    return j;
}

// A stretch of one row: the sums so far (b: bit errors + (symbol errors << 16), both below 2^15 inside a tile) and whether a row boundary
// lies inside the stretch.  seg_join is the operator of the segmented scan: what lies behind a boundary forgets what was in front of it.
struct Seg { float e, q; int b, f; };

__device__ __forceinline__ Seg seg_join(const Seg& front, const Seg& back)
{
    if (back.f) return back;
    return Seg{ front.e + back.e, front.q + back.q, front.b + back.b, front.f };
}

__device__ __forceinline__ Seg seg_up(const Seg& x, int d)
{
    return Seg{ __shfl_up(x.e, d), __shfl_up(x.q, d), __shfl_up(x.b, d), __shfl_up(x.f, d) };
}

// a row is complete: its three outputs, each written here and nowhere else
__device__ __forceinline__ void store_row(const MeasureArgs& a, int64_t r, bool measured, int be, float e, float q)
{
    if (a.bit_errors) a.bit_errors[r] = measured ? be : -1;
    if (a.err_power) a.err_power[r] = measured ? e : 0.f;
    if (a.ref_power) a.ref_power[r] = measured ? q : 0.f;
}

// one step along the flat array inside a tile: (rows past the tile's first row, index in the row), 32-bit
struct TilePos { int dr, i; };
__device__ __forceinline__ TilePos step(TilePos p, int q, int rem, int n)      // q = d / n, rem = d % n of the step d
{
    uint32_t i = (uint32_t)p.i + (uint32_t)rem;                              // below 2 n: unsigned, n may be close to 2^31
    p.dr += q;
    if (i >= (uint32_t)n) {
        i -= (uint32_t)n;
        ++p.dr;
    }
    p.i = (int)i;
    return p;
}

template <int K, int RULE>
__global__ __launch_bounds__(kLanes) void k_meter_measure(MeasureArgs a)
{
    __shared__ cf pts[1 << K];
    __shared__ float s_e[kPadSlots + 1], s_q[kPadSlots + 1];                // + 1: where a lane's symbol outside the tile goes
    __shared__ unsigned char s_b[kPadSlots + 1];
    __shared__ Seg wave_total[kLanes / 64];
    __shared__ u64 block_total[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < (1 << K); i += kLanes) pts[i] = a.points[i];
    if (tid < 5) block_total[tid] = 0;
    __syncthreads();
    const bool aided = a.payload != nullptr;
    const int64_t n_live = live_rows(a.count, a.n_rows);
    const int n = (int)a.n_sym;                                              // n_sym k < 2^31
    const int64_t total = a.n_rows * a.n_sym;
    const int mis = (int)(((uintptr_t)a.sym / sizeof(cf)) & 1);             // symbols between the 16-byte boundary in front of `sym` and `sym`
    const int64_t ntiles = (total + kTileSyms - 1) / kTileSyms;
    const int q_vec = (2 * kLanes) / n, rem_vec = (2 * kLanes) % n;          // from a lane's vector to its next one: 512 symbols
    uint32_t c_rows = 0, c_syms = 0, c_be = 0, c_se = 0, c_re = 0;          // this lane's share of the totals
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s_lo = tile * kTileSyms;
        const int cnt = (int)std::min<int64_t>(kTileSyms, total - s_lo);     // symbols of the tile: slots 0 .. cnt - 1
        const int64_t r0 = s_lo / a.n_sym;
        const int i0 = (int)(s_lo - r0 * a.n_sym);
        const bool row0_starts_here = i0 == 0;
        // everything below is relative to the tile: slot = s - s_lo, dr = row - r0, in 32 bits (the tile's first symbol is even, so the
        // lane's vector u holds the slots 2 (256 u + tid) - mis and the next one)
        const int live_rel = (int)std::min<int64_t>(std::max<int64_t>(n_live - r0, 0), kTileSyms + 1);
        const int ref_rel = aided ? (int)std::min<int64_t>(std::max<int64_t>(a.n_ref - r0, 0), kTileSyms + 1) : kTileSyms + 1;
        const int64_t* ref_row0 = a.ref_row ? a.ref_row + r0 : nullptr;
        // ---- where the lane's symbols lie: one division, then steps ----
        const uint32_t t0 = (uint32_t)i0 + (uint32_t)n + (uint32_t)(2 * tid - mis);              // slot 2 tid - mis, one row early so that slot -1 stays positive
        TilePos vec = { (int)(t0 / (uint32_t)n) - 1, (int)(t0 % (uint32_t)n) };
        TilePos pos[kLoads][2];
        bool in_tile[kLoads][2], ok[kLoads][2];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int slot = 2 * (u * kLanes + tid) - mis;
            pos[u][0] = vec;
            pos[u][1] = step(vec, 0, 1, n);
            in_tile[u][0] = slot >= 0 && slot < cnt;
            in_tile[u][1] = slot + 1 < cnt;
            vec = step(vec, q_vec, rem_vec, n);
        }
        // ---- which of them are measured; with a ref_row its entries are loaded for all ten before any is looked at ----
        int64_t ref[kLoads][2];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                ok[u][e] = in_tile[u][e] && pos[u][e].dr < live_rel;
                ref[u][e] = r0 + pos[u][e].dr;
            }
        }
        if (ref_row0) {
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                ref[u][0] = ref_row0[in_tile[u][0] ? pos[u][0].dr : 0];
                ref[u][1] = ref_row0[in_tile[u][1] ? pos[u][1].dr : 0];
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
#pragma unroll
                for (int e = 0; e < 2; ++e) ok[u][e] = ok[u][e] && ref[u][e] >= 0 && (!aided || ref[u][e] < a.n_ref);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
#pragma unroll
                for (int e = 0; e < 2; ++e) ok[u][e] = ok[u][e] && pos[u][e].dr < ref_rel;
            }
        }
        // ---- load: a symbol of the tile whose row is measured, and no other (a vector that is not wholly measured reads the point table
        // in its place and takes its measured symbol alone) ----
        const cf* sym0 = a.sym + s_lo;
        cf x[kLoads][2];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int slot = 2 * (u * kLanes + tid) - mis;
            const bool whole = ok[u][0] && ok[u][1];                        // a whole vector: 16-byte aligned by construction
            const float4 q = *(whole ? reinterpret_cast<const float4*>(sym0 + slot) : reinterpret_cast<const float4*>(a.points));
            x[u][0] = make_float2(q.x, q.y);
            x[u][1] = make_float2(q.z, q.w);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int slot = 2 * (u * kLanes + tid) - mis;
            if (ok[u][0] != ok[u][1]) {                                     // seldom: a tile's first or last symbol, the edge of an unmeasured row
                if (ok[u][0]) x[u][0] = sym0[slot];
                else x[u][1] = sym0[slot + 1];
            }
        }
        // the one or two payload bytes of every symbol; an unmeasured symbol reads the point table, a symbol inside one byte that byte twice
        unsigned bits[kLoads][2];
        if (aided) {
            unsigned char b0[kLoads][2], b1[kLoads][2];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int q = pos[u][e].i * K;
                    const unsigned char* byte = ok[u][e] ? a.payload + ref[u][e] * a.row_bytes + (q >> 3) : reinterpret_cast<const unsigned char*>(a.points);
                    b0[u][e] = byte[0];
                    b1[u][e] = byte[(ok[u][e] && (q & 7) + K > 8) ? 1 : 0];  // the symbol's own bits reach into that byte: it is inside the row
                }
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
#pragma unroll
                for (int e = 0; e < 2; ++e) bits[u][e] = ((unsigned)b0[u][e] << 8) | b1[u][e];
            }
        }
        // ---- decide, compare with what was sent, leave the three terms of every symbol in LDS (s_b = kUnmeasured: the row is not
        // measured; whatever a lane holds for a slot outside the tile goes to the spare slot) ----
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            if (2 * (u * kLanes + tid) - mis >= cnt) continue;
            int idx[2];
            decide2<K, RULE>(x[u][0], x[u][1], pts, idx[0], idx[1]);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int slot = 2 * (u * kLanes + tid) - mis + e;
                const int ps = in_tile[u][e] ? slot + slot / kPerLane : kPadSlots;
                int sent = idx[e];
                if (aided) sent = (int)((bits[u][e] >> (16 - ((pos[u][e].i * K) & 7) - K)) & ((1u << K) - 1u));
                const cf p = pts[sent];
                s_e[ps] = dist2(x[u][e], p);
                s_q[ps] = p.x * p.x + p.y * p.y;
                s_b[ps] = ok[u][e] ? (unsigned char)__popc((unsigned)(idx[e] ^ sent)) : (unsigned char)kUnmeasured;
            }
        }
        __syncthreads();
        // ---- by row: lane t walks the symbols 8 t .. 8 t + 7 ----
        const int base = kPerLane * tid;
        const int mine = std::min(kPerLane, std::max(cnt - base, 0));
        const uint32_t w0 = (uint32_t)i0 + (uint32_t)base;
        int dr = (int)(w0 / (uint32_t)n), i = (int)(w0 % (uint32_t)n);
        Seg acc = { 0.f, 0.f, 0, 0 }, head = { 0.f, 0.f, 0, 0 };
        int head_dr = -1;
        bool head_measured = false, cur = false;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            if (j >= mine) break;
            const int ps = base + j + tid;                                  // slot + slot / 8
            const int b = s_b[ps];
            const float e = s_e[ps], q = s_q[ps];
            cur = b != kUnmeasured;
            const bool starts = i == 0;
            acc.e = starts ? 0.f : acc.e;
            acc.q = starts ? 0.f : acc.q;
            acc.b = starts ? 0 : acc.b;
            acc.f |= starts;
            c_rows += starts && cur;
            acc.e += cur ? e : 0.f;                                         // (+ 0: exact)
            acc.q += cur ? q : 0.f;
            acc.b += cur ? b + ((b != 0) << 16) : 0;
            c_syms += cur;
            c_be += cur ? b : 0;
            c_se += cur && b != 0;
            if (i == n - 1) {                                               // the row ends here
                if (acc.f) {                                                // ... and began in this lane
                    store_row(a, r0 + dr, cur, acc.b & 0xffff, acc.e, acc.q);
                    c_re += cur && (acc.b & 0xffff);
                } else {                                                    // ... and began in front of it: at most one such row a lane
                    head = acc;
                    head_dr = dr;
                    head_measured = cur;
                }
                acc = Seg{ 0.f, 0.f, 0, 1 };
                ++dr;
                i = 0;
            } else {
                ++i;
            }
        }
        // ---- the open ends: an inclusive segmented scan over the lanes, then the carry into every lane ----
        Seg inc = acc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Seg front = seg_up(inc, d);
            if (lane >= d) inc = seg_join(front, inc);
        }
        if (lane == 63) wave_total[wave] = inc;
        __syncthreads();
        Seg carry = { 0.f, 0.f, 0, 0 };
        for (int w = 0; w < wave; ++w) carry = seg_join(carry, wave_total[w]);
        const Seg before = seg_up(inc, 1);
        if (lane > 0) carry = seg_join(carry, before);
        if (head_dr >= 0) {
            const Seg t = seg_join(carry, head);
            if (head_dr > 0 || row0_starts_here) {                          // the row lies inside the tile
                store_row(a, r0 + head_dr, head_measured, t.b & 0xffff, t.e, t.q);
                c_re += head_measured && (t.b & 0xffff);
            } else if (head_measured) {
                a.part[2 * tile] = Partial{ (double)t.e, (double)t.q, t.b & 0xffff, t.b >> 16 };
            }
        }
        if (tid == kLanes - 1 && mine > 0 && i != 0 && cur) {               // the row that is still open where the tile ends
            const Seg t = seg_join(carry, acc);
            a.part[2 * tile + ((dr > 0 || row0_starts_here) ? 1 : 0)] = Partial{ (double)t.e, (double)t.q, t.b & 0xffff, t.b >> 16 };
        }
        __syncthreads();                             // s_e, s_q, s_b and wave_total are rewritten for the next tile
    }
    // ---- totals: lane -> wave -> workgroup -> one atomic per field ----
    u64 c[5] = { c_rows, c_syms, c_be, c_se, c_re };
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c[f] += __shfl_xor(c[f], d);
        if (lane == 0 && c[f]) atomicAdd(&block_total[f], c[f]);
    }
    __syncthreads();
    if (tid == 0) {
        if (block_total[0]) atomicAdd(&a.totals[T_ROWS], block_total[0]);
        if (block_total[1]) atomicAdd(&a.totals[T_SYMBOLS], block_total[1]);
        if (aided) {
            if (block_total[1]) atomicAdd(&a.totals[T_BITS], block_total[1] * (u64)K);
            if (block_total[2]) atomicAdd(&a.totals[T_BIT_ERRORS], block_total[2]);
            if (block_total[3]) atomicAdd(&a.totals[T_SYMBOL_ERRORS], block_total[3]);
            if (block_total[4]) atomicAdd(&a.totals[T_ROW_ERRORS], block_total[4]);
        }
    }
}

// The rows that cross a tile boundary: one lane per boundary, and the lane of the FIRST boundary a row crosses adds the row's partial
// records in ascending tile order, in fp64, and rounds once.
__global__ __launch_bounds__(kLanes) void k_meter_crossing_rows(MeasureArgs a, int64_t ntiles)
{
    const int64_t n = a.n_sym, n_live = live_rows(a.count, a.n_rows);
    const int64_t b = (int64_t)blockIdx.x * kLanes + threadIdx.x + 1;
    bool row_error = false;
    if (b < ntiles) {
        const int64_t s = b * kTileSyms, r = s / n;
        const int64_t first = (r * n) / kTileSyms;
        if (s != r * n && first == b - 1) {
            const int64_t last = ((r + 1) * n - 1) / kTileSyms;
            const bool measured = ref_of(a, r, n_live) >= 0;
            double e = 0., q = 0.;
            int be = 0;
            if (measured) {
                const Partial p = a.part[2 * first + 1];
                e = p.e, q = p.q, be = p.be;
                for (int64_t t = first + 1; t <= last; ++t) {
                    const Partial c = a.part[2 * t];
                    e += c.e, q += c.q, be += c.be;
                }
            }
            store_row(a, r, measured, be, (float)e, (float)q);
            row_error = measured && a.payload && be > 0;
        }
    }
    const int errors = __syncthreads_count(row_error);
    if (threadIdx.x == 0 && errors) atomicAdd(&a.totals[T_ROW_ERRORS], (u64)errors);
}

__global__ void k_meter_reset(u64* totals)
{
    if (threadIdx.x < T_FIELDS) totals[threadIdx.x] = 0;
}

// ---- match ----
struct MatchArgs {
    const int64_t* frame_start;      // [n_rows]
    const int64_t* count;            // optional
    const int64_t* sent_pos;         // [n_sent], ascending
    int64_t n_rows, n_sent, offset, tol;
    int64_t* ref_row;                // optional: [n_rows]
    int64_t* sent_row;               // optional: [n_sent]
    u64* key;                        // [n_sent]: (distance << 32) | d of the best detection so far
    u64* totals;
};

constexpr u64 kNoKey = ~(u64)0;

// e_j; the sum wraps where it overflows (such positions are far outside any tol)
__device__ __forceinline__ int64_t expected(const MatchArgs& a, int64_t j) { return (int64_t)((u64)a.sent_pos[j] + (u64)a.offset); }

// the first j with e_j >= v (n_sent where there is none)
__device__ __forceinline__ int64_t lower_bound(const MatchArgs& a, int64_t v)
{
    int64_t lo = 0, hi = a.n_sent;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (expected(a, mid) < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ u64 distance(int64_t x, int64_t y) { return x >= y ? (u64)x - (u64)y : (u64)y - (u64)x; }

// what detection d proposes: the key it bids with and the sent burst j, or false where d is no detection or nothing lies within tol
__device__ __forceinline__ bool proposal(const MatchArgs& a, int64_t d, int64_t n_live, bool& detection, int64_t& j, u64& key)
{
    detection = false;
    if (d >= n_live) return false;
    const int64_t fs = a.frame_start[d];
    if (fs < 0) return false;
    detection = true;
    if (a.n_sent == 0) return false;
    const int64_t hi = lower_bound(a, fs);                                  // e_(hi - 1) < fs <= e_hi
    int64_t v;
    if (hi == a.n_sent) v = expected(a, hi - 1);
    else if (hi == 0) v = expected(a, 0);
    else {
        const int64_t below = expected(a, hi - 1), above = expected(a, hi);
        v = distance(fs, below) <= distance(fs, above) ? below : above;     // a tie goes to the lower j
    }
    const u64 dist = distance(fs, v);
    if (dist > (u64)a.tol) return false;
    j = lower_bound(a, v);                                                  // the lowest j of equal positions
    if (j >= a.n_sent) return false;                                        // (a sent_pos that is not ascending)
    key = (dist << 32) | (u64)d;
    return true;
}

__global__ __launch_bounds__(kLanes) void k_meter_match_init(MatchArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (j < a.n_sent) a.key[j] = kNoKey;
}

__global__ __launch_bounds__(kLanes) void k_meter_match_propose(MatchArgs a)
{
    const int64_t d = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (d >= a.n_rows) return;
    bool detection;
    int64_t j = 0;
    u64 key = 0;
    if (proposal(a, d, live_rows(a.count, a.n_rows), detection, j, key)) atomicMin(&a.key[j], key);
}

__global__ __launch_bounds__(kLanes) void k_meter_match_resolve(MatchArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    bool detection = false, winner = false, sent = t < a.n_sent;
    if (t < a.n_rows) {
        int64_t j = 0;
        u64 key = 0;
        winner = proposal(a, t, live_rows(a.count, a.n_rows), detection, j, key) && a.key[j] == key;
        if (a.ref_row) a.ref_row[t] = winner ? j : -1;
    }
    if (sent && a.sent_row) {
        const u64 key = a.key[t];
        a.sent_row[t] = key == kNoKey ? -1 : (int64_t)(key & 0xffffffffu);
    }
    const int detections = __syncthreads_count(detection), winners = __syncthreads_count(winner);
    const int found = __syncthreads_count(sent && a.key[t] != kNoKey), all_sent = __syncthreads_count(sent);
    if (threadIdx.x == 0) {
        if (detections) atomicAdd(&a.totals[T_DETECTIONS], (u64)detections);
        if (winners) atomicAdd(&a.totals[T_MATCHED], (u64)winners);
        if (all_sent - found) atomicAdd(&a.totals[T_MISSED], (u64)(all_sent - found));
        if (detections - winners) atomicAdd(&a.totals[T_FALSE_ALARMS], (u64)(detections - winners));
    }
}

int64_t tiles_of(int64_t n_sym, int64_t n_rows) { return (n_sym * n_rows + kTileSyms - 1) / kTileSyms; }

}  // namespace

struct gfdm_hip_link_meter {
    gfdm::DeviceCtx ctx;
    gfdm::Constellation c;
    u64* d_totals = nullptr;
    ~gfdm_hip_link_meter()
    {
        if (!c.d_points && !d_totals) return;
        DeviceGuard guard(ctx.device);
        (void)hipFree(c.d_points);
        (void)hipFree(d_totals);
    }
};

namespace {

// the argument table of measure (include/gfdm_hip.h); needs no device
int measure_check(const gfdm_hip_link_meter* h, const void* bit_errors, const void* symbols, const void* payload, int64_t n_ref, int64_t n_sym, int64_t n_rows,
                  const void* workspace, bool device)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = gfdm_hip_symbol_mapper_check(1 << h->c.k, n_sym, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_sym > (int64_t)INT32_MAX / h->c.k) return api_fail(GFDM_HIP_EINVAL, "n_sym * k must be <= 2^31 - 1: the bit errors of a row are an int32");
    if (n_ref < 0) return api_fail(GFDM_HIP_EINVAL, "n_ref must be >= 0");
    if (!payload && bit_errors) return api_fail(GFDM_HIP_EINVAL, "bit_errors needs a payload: a decision-directed call counts no errors");
    if (n_rows > 0 && !symbols) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    if (n_rows > 0 && device && !workspace) return api_fail(GFDM_HIP_EINVAL, "NULL workspace");
    return GFDM_HIP_OK;
}

// the two launches of a measure call.  Everything is a device pointer.
int measure_enqueue(const gfdm_hip_link_meter* h, void* bit_errors, void* err_power, void* ref_power, const void* symbols, const void* payload, int64_t n_ref,
                    const void* ref_row, const void* count, int64_t n_sym, int64_t n_rows, void* workspace, hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(symbols, sizeof(cf)) || misaligned(bit_errors, sizeof(int32_t)) || misaligned(err_power, sizeof(float)) || misaligned(ref_power, sizeof(float)) ||
        misaligned(ref_row, sizeof(int64_t)) || misaligned(count, sizeof(int64_t)))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    if (misaligned(workspace, 16)) return api_fail(GFDM_HIP_EINVAL, "the workspace must be 16-byte aligned");
    const MeasureArgs a = { h->c.d_points, static_cast<const cf*>(symbols), static_cast<const unsigned char*>(payload), static_cast<const int64_t*>(ref_row),
                            static_cast<const int64_t*>(count), n_sym, n_rows, n_ref, row_bytes_of(h->c.k, n_sym), static_cast<int32_t*>(bit_errors),
                            static_cast<float*>(err_power), static_cast<float*>(ref_power), static_cast<Partial*>(workspace), h->d_totals };
    const int64_t ntiles = tiles_of(n_sym, n_rows);
    const unsigned grid = (unsigned)std::min<int64_t>(ntiles, kMaxTiles);
    gfdm::dispatch_bits(h->c.k, [&](auto bits) {
        gfdm::with_rule<decltype(bits)::value>(h->c.rule, [&](auto k, auto rule) {
            hipLaunchKernelGGL((k_meter_measure<decltype(k)::value, decltype(rule)::value>), dim3(grid), dim3(kLanes), 0, s, a);
        });
    });
    GFDM_TRY(hipGetLastError());
    if (ntiles > 1) {
        hipLaunchKernelGGL(k_meter_crossing_rows, dim3((unsigned)((ntiles - 1 + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a, ntiles);
        GFDM_TRY(hipGetLastError());
    }
    return GFDM_HIP_OK;
}

int match_check(const gfdm_hip_link_meter* h, const void* frame_start, int64_t n_rows, const void* sent_pos, int64_t n_sent, int64_t tol, const void* workspace,
                bool device)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (tol < 0 || tol >= kMaxIndex) return api_fail(GFDM_HIP_EINVAL, "tol must lie in 0 .. 2^31 - 1");
    if (n_rows < 0 || n_rows >= kMaxIndex) return api_fail(GFDM_HIP_EINVAL, "n_rows must lie in 0 .. 2^31 - 1");
    if (n_sent < 0 || n_sent >= kMaxIndex) return api_fail(GFDM_HIP_EINVAL, "n_sent must lie in 0 .. 2^31 - 1");
    if ((n_rows > 0 && !frame_start) || (n_sent > 0 && !sent_pos)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    if (n_sent > 0 && device && !workspace) return api_fail(GFDM_HIP_EINVAL, "NULL workspace");
    return GFDM_HIP_OK;
}

// the (at most three) launches of a match call.  Everything is a device pointer.
int match_enqueue(const gfdm_hip_link_meter* h, void* ref_row, void* sent_row, const void* frame_start, const void* count, int64_t n_rows, const void* sent_pos,
                  int64_t n_sent, int64_t offset, int64_t tol, void* workspace, hipStream_t s)
{
    if (n_rows == 0 && n_sent == 0) return GFDM_HIP_OK;
    if (misaligned(ref_row, 8) || misaligned(sent_row, 8) || misaligned(frame_start, 8) || misaligned(count, 8) || misaligned(sent_pos, 8) || misaligned(workspace, 8))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const MatchArgs a = { static_cast<const int64_t*>(frame_start), static_cast<const int64_t*>(count), static_cast<const int64_t*>(sent_pos), n_rows, n_sent, offset, tol,
                          static_cast<int64_t*>(ref_row), static_cast<int64_t*>(sent_row), static_cast<u64*>(workspace), h->d_totals };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + kLanes - 1) / kLanes)); };
    if (n_sent > 0) {
        hipLaunchKernelGGL(k_meter_match_init, blocks(n_sent), dim3(kLanes), 0, s, a);
        GFDM_TRY(hipGetLastError());
        if (n_rows > 0) {
            hipLaunchKernelGGL(k_meter_match_propose, blocks(n_rows), dim3(kLanes), 0, s, a);
            GFDM_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_meter_match_resolve, blocks(std::max(n_rows, n_sent)), dim3(kLanes), 0, s, a);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

}  // namespace

extern "C" {

int gfdm_hip_link_meter_create(gfdm_hip_link_meter** out, const float* points, int n_points, int decision, int device)
{
    return gfdm::create_handle(
        out, device, [&](gfdm_hip_link_meter& h) { return h.c.set(points, n_points, decision); },
        [](gfdm_hip_link_meter& h) -> int {
            const int rc = h.c.upload();
            if (rc != GFDM_HIP_OK) return rc;
            hipError_t e = hipMalloc(&h.d_totals, T_FIELDS * sizeof(u64));
            if (e == hipSuccess) e = hipMemset(h.d_totals, 0, T_FIELDS * sizeof(u64));
            if (e == hipSuccess) e = hipDeviceSynchronize();
            return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "constellation upload");
        });
}

int gfdm_hip_link_meter_destroy(gfdm_hip_link_meter* m) { delete m; return GFDM_HIP_OK; }
int gfdm_hip_link_meter_bits_per_symbol(const gfdm_hip_link_meter* m) { return m ? m->c.k : GFDM_HIP_EINVAL; }
int gfdm_hip_link_meter_n_points(const gfdm_hip_link_meter* m) { return m ? 1 << m->c.k : GFDM_HIP_EINVAL; }
int gfdm_hip_link_meter_decision(const gfdm_hip_link_meter* m) { return m ? m->c.rule : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_link_meter_row_bytes(const gfdm_hip_link_meter* m, int64_t n_sym)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = gfdm_hip_symbol_mapper_check(1 << m->c.k, n_sym, 0);
    return rc != GFDM_HIP_OK ? rc : row_bytes_of(m->c.k, n_sym);
}

void* gfdm_hip_link_meter_totals_device(gfdm_hip_link_meter* m) { return m ? m->d_totals : nullptr; }

int gfdm_hip_link_meter_reset(gfdm_hip_link_meter* m, void* stream)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) -> int {
        hipLaunchKernelGGL(k_meter_reset, dim3(1), dim3(64), 0, s, m->d_totals);
        GFDM_TRY(hipGetLastError());
        return GFDM_HIP_OK;
    });
}

int gfdm_hip_link_meter_totals(gfdm_hip_link_meter* m, int64_t* out, void* stream)
{
    if (!m || !out) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) -> int {
        GFDM_TRY(hipStreamSynchronize(s));
        GFDM_TRY(hipMemcpy(out, m->d_totals, T_FIELDS * sizeof(u64), hipMemcpyDeviceToHost));
        return GFDM_HIP_OK;
    });
}

int64_t gfdm_hip_link_meter_match_workspace_bytes(int64_t n_sent)
{
    if (n_sent < 0 || n_sent >= kMaxIndex) return api_fail(GFDM_HIP_EINVAL, "n_sent must lie in 0 .. 2^31 - 1");
    return std::max<int64_t>(16, n_sent * (int64_t)sizeof(u64));
}

int64_t gfdm_hip_link_meter_measure_workspace_bytes(int64_t n_sym, int64_t n_rows)
{
    const int rc = gfdm_hip_symbol_mapper_check(2, n_sym, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return std::max<int64_t>(16, tiles_of(n_sym, n_rows) * 2 * (int64_t)sizeof(Partial));
}

int gfdm_hip_link_meter_match_device(gfdm_hip_link_meter* m, void* ref_row, void* sent_row, const void* frame_start, const void* count, int64_t n_rows,
                                     const void* sent_pos, int64_t n_sent, int64_t offset, int64_t tol, void* workspace, void* stream)
{
    const int rc = match_check(m, frame_start, n_rows, sent_pos, n_sent, tol, workspace, true);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) {
        return match_enqueue(m, ref_row, sent_row, frame_start, count, n_rows, sent_pos, n_sent, offset, tol, workspace, s);
    });
}

int gfdm_hip_link_meter_match_host(gfdm_hip_link_meter* m, int64_t* ref_row, int64_t* sent_row, const int64_t* frame_start, const int64_t* count, int64_t n_rows,
                                   const int64_t* sent_pos, int64_t n_sent, int64_t offset, int64_t tol)
{
    const int rc0 = match_check(m, frame_start, n_rows, sent_pos, n_sent, tol, nullptr, false);
    if (rc0 != GFDM_HIP_OK) return rc0;
    if (n_rows == 0 && n_sent == 0) return GFDM_HIP_OK;
    const size_t nr = (size_t)n_rows, ns = (size_t)n_sent;
    gfdm::HostCall hc(m->ctx);
    const auto fs = hc.in(frame_start, nr);
    const auto pos = hc.in(sent_pos, ns);
    const auto cnt = hc.in(count, 1);
    const auto ref = hc.out(ref_row, nr);
    const auto sent = hc.out(sent_row, ns);
    const auto key = hc.scratch<u64>(ns);
    return hc.run([&](hipStream_t s) {
        return match_enqueue(m, ref.dev(), sent.dev(), fs.dev(), cnt.dev(), n_rows, pos.dev(), n_sent, offset, tol, key.dev(), s);
    });
}

int gfdm_hip_link_meter_measure_device(gfdm_hip_link_meter* m, void* bit_errors, void* err_power, void* ref_power, const void* symbols, const void* payload,
                                       int64_t n_ref, const void* ref_row, const void* count, int64_t n_sym, int64_t n_rows, void* workspace, void* stream)
{
    const int rc = measure_check(m, bit_errors, symbols, payload, n_ref, n_sym, n_rows, workspace, true);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(m->ctx.device, stream, [&](hipStream_t s) {
        return measure_enqueue(m, bit_errors, err_power, ref_power, symbols, payload, n_ref, ref_row, count, n_sym, n_rows, workspace, s);
    });
}

int gfdm_hip_link_meter_measure_host(gfdm_hip_link_meter* m, int32_t* bit_errors, float* err_power, float* ref_power, const float* symbols, const uint8_t* payload,
                                     int64_t n_ref, const int64_t* ref_row, const int64_t* count, int64_t n_sym, int64_t n_rows)
{
    const int rc0 = measure_check(m, bit_errors, symbols, payload, n_ref, n_sym, n_rows, nullptr, false);
    if (rc0 != GFDM_HIP_OK) return rc0;
    if (n_rows == 0) return GFDM_HIP_OK;
    const size_t nr = (size_t)n_rows;
    gfdm::HostCall hc(m->ctx);
    const auto sym = hc.in(symbols, nr * (size_t)n_sym * 2);
    const auto pay = hc.in(payload, (size_t)n_ref * (size_t)row_bytes_of(m->c.k, n_sym));
    const auto ref = hc.in(ref_row, nr);
    const auto cnt = hc.in(count, 1);
    const auto be = hc.out(bit_errors, nr);
    const auto ep = hc.out(err_power, nr);
    const auto rp = hc.out(ref_power, nr);
    const auto ws = hc.scratch<unsigned char>((size_t)gfdm_hip_link_meter_measure_workspace_bytes(n_sym, n_rows));
    return hc.run([&](hipStream_t s) {
        return measure_enqueue(m, be.dev(), ep.dev(), rp.dev(), sym.dev(), pay.dev(), n_ref, ref.dev(), cnt.dev(), n_sym, n_rows, ws.dev(), s);
    });
}

}  // extern "C"
