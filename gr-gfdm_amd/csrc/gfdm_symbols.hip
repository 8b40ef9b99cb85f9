// Symbol mapper at both ends of the chain: payload bytes -> constellation points in front of the transmitter, demapped symbols -> payload
// bytes or max-log soft bits behind the receivers (GNU Radio's repack_bits_bb(8 -> k, MSB first) + chunks_to_symbols, and
// constellation_decoder_cb + repack_bits_bb(k -> 8); pygfdm's bits2symbols / symbols2bits).  The contract is written out in
// include/gfdm_hip.h.
//
// Three element-wise kernels, memory bound by design.  The OUTPUT is tiled, never the rows: a workgroup takes a fixed stretch of the flat
// output, so 32768 + 7 rows of 5 symbols spread as evenly as one row of 2^20.  map and soft stand on the row stages' tile skeleton
// (gfdm_rowtile.h); decode has byte stores and no aligned output vector, and tiles by itself.
//   decode: a tile is 256 k packed bytes.  The symbols behind them are ONE contiguous stretch of the input (at most 2048 + 2: rows are
//           contiguous on both sides); the lanes load it as 16-byte vectors aligned in memory (two symbols a lane, 1 KiB a wave; a head that
//           is only 8-byte aligned and a ragged tail go element by element), decide at once and leave one index byte per symbol in LDS.
//           Then lane t assembles output byte t from the (at most 8) index bytes it spans and stores it: 64 contiguous bytes a wave.
//   soft:   a tile is 1024 aligned 16-byte vectors of LLRs.  The symbols behind them (at most 4096 / k + 2) are loaded as above, each
//           lane leaves its symbols' k LLRs in LDS, and the tile goes out as 16 bytes a lane whatever k is.
//   map:    a tile is 1024 aligned 16-byte vectors of two symbols; the packed input is 1/32 .. 1/4 of that and read through the cache.
// The point table sits in LDS (none for the sign tests).  Rows from n_live on are written as zeros by the same kernel and their input
// is never read; nothing is written outside the output and every element of it once.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"
#include "gfdm_rowtile.h"

#include <algorithm>
#include <climits>

using gfdm::cf;
using gfdm::RowPos;
using gfdm::advance;
using gfdm::RowCursor;
using gfdm::StreamTiles;
using gfdm::row_grid;
using gfdm::store_elems;
using gfdm::dist2;
using gfdm::decide2;                 // gfdm_decide.h: shared with the link meter
using gfdm::api_fail;
using gfdm::bits_of;
using gfdm::row_bytes_of;
using gfdm::live_rows;
using gfdm::misaligned;

namespace {

constexpr int kLanes = 256;
constexpr int kTileVec = 4 * kLanes;                 // map, soft: 16-byte vectors of output per tile (16 KiB)
constexpr int kMaxTiles = 8192;                      // workgroups per launch; the tiles beyond are strided over
constexpr int kDecodeSyms = 8 * kLanes;              // decode: a tile is kLanes * k bytes = 2048 symbols' worth of bits
constexpr int kDecodeSlots = kDecodeSyms + 16;       // ... + 2 (rows begin on a byte) + 2 (vectors begin on 16 bytes), rounded up
constexpr int kSoftSlots = 4 * kTileVec + 8 * 8;     // floats: (4096 / k + 2 + 2) symbols of k LLRs
static_assert(4 * kTileVec - 1 <= gfdm::kMaxRowReach, "RowCursor::at: map steps over a tile's 2 kTileVec symbols, soft over those behind its 4 kTileVec LLRs");

struct MapperArgs {
    const cf* points;        // [1 << k] (device)
    int64_t n_sym, n_rows;
    int64_t row_bytes;       // ceil(n_sym k / 8)
    const int64_t* count;    // optional (device): live rows = clamp(*count, 0, n_rows)
    const float* scale;      // soft, optional (device): [n_rows]
};

// the 16-byte vector v of the symbol array (symbols 2 v - mis, 2 v - mis + 1 of the flat input; those outside [0, s_end) read as 0)
__device__ __forceinline__ void load_pair(const cf* __restrict__ in, int64_t s, int64_t s_end, cf& x0, cf& x1)
{
    x0 = x1 = make_float2(0.f, 0.f);
    if (s >= 0 && s + 1 < s_end) {                   // a whole vector: 16-byte aligned by construction
        const float4 q = *reinterpret_cast<const float4*>(in + s);
        x0 = make_float2(q.x, q.y);
        x1 = make_float2(q.z, q.w);
    } else {
        if (s >= 0 && s < s_end) x0 = in[s];
        if (s + 1 >= 0 && s + 1 < s_end) x1 = in[s + 1];
    }
}

template <int K>
__device__ __forceinline__ void load_points(cf* pts, const MapperArgs& a)
{
    for (int i = threadIdx.x; i < (1 << K); i += kLanes) pts[i] = a.points[i];
    __syncthreads();
}

template <int K, int RULE>
__global__ __launch_bounds__(kLanes) void k_symbols_decode(MapperArgs a, const cf* __restrict__ in, unsigned char* __restrict__ out)
{
    constexpr bool TABLE = RULE == GFDM_HIP_DECIDE_NEAREST;
    constexpr int kTileBytes = kLanes * K;
    constexpr int kLoads = (kDecodeSlots / 2 + kLanes - 1) / kLanes;         // vectors per lane (the last one is seldom there)
    __shared__ cf pts[TABLE ? (1 << K) : 1];
    __shared__ unsigned char idx[kDecodeSlots];
    if constexpr (TABLE) load_points<K>(pts, a);
    const int64_t n_live = live_rows(a.count, a.n_rows), rb = a.row_bytes;
    const int64_t total = a.n_rows * rb, live_bytes = n_live * rb, s_live = n_live * a.n_sym;
    const int mis = (int)(((uintptr_t)in / sizeof(cf)) & 1);                 // symbols between the 16-byte boundary in front of `in` and `in`
    const int64_t ntiles = (total + kTileBytes - 1) / kTileBytes;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t o0 = tile * kTileBytes, o1 = std::min(o0 + kTileBytes, total);
        const int64_t o_live = std::min(o1, live_bytes);                     // the bytes [o0, o_live) hold symbols
        const int64_t r0 = o0 / rb, b0 = o0 - r0 * rb;
        int64_t s_base = 0;
        if (o_live > o0) {
            const RowPos last = advance(r0, b0, (uint32_t)(o_live - 1 - o0), rb);
            const int64_t s_lo = r0 * a.n_sym + (8 * b0) / K;
            const int64_t s_hi = last.r * a.n_sym + std::min(a.n_sym, (8 * last.i + 7) / K + 1);       // <= s_live: last.r < n_live
            const int64_t v_lo = (s_lo + mis) >> 1, v_end = (s_hi + mis + 1) >> 1;
            s_base = 2 * v_lo - mis;
            cf x[kLoads][2];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int64_t v = v_lo + u * kLanes + threadIdx.x;
                if (v < v_end) load_pair(in, 2 * v - mis, s_live, x[u][0], x[u][1]);
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int64_t v = v_lo + u * kLanes + threadIdx.x;
                const int slot = 2 * (u * kLanes + (int)threadIdx.x);
                if (v < v_end && slot + 1 < kDecodeSlots) {
                    int i0, i1;
                    decide2<K, RULE>(x[u][0], x[u][1], pts, i0, i1);
                    idx[slot] = (unsigned char)i0;
                    idx[slot + 1] = (unsigned char)i1;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < K; ++p) {
            const int64_t o = o0 + p * kLanes + threadIdx.x;
            if (o >= o1) continue;
            unsigned byte = 0;
            if (o < o_live) {
                const RowPos pos = advance(r0, b0, (uint32_t)(o - o0), rb);
                const int64_t q = 8 * pos.i, i = q / K;
                const int j0 = (int)(q - i * K);
                const int slot = (int)(pos.r * a.n_sym + i - s_base);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int di = (j0 + t) / K, j = (j0 + t) % K;
                    if (i + di < a.n_sym) byte |= ((idx[slot + di] >> (K - 1 - j)) & 1u) << (7 - t);
                }
            }
            out[o] = (unsigned char)byte;
        }
        __syncthreads();                             // idx is rewritten for the next tile
    }
}

// the 2 K minima of one symbol: m0[j] / m1[j] over the points whose bit j (MSB first) is 0 / 1.  The points go by in groups of 16: the low
// four bits of the index are compile-time constants, the high ones are the same in every lane and take the group's minimum once.
template <int K>
__device__ __forceinline__ void soft_minima(cf x, const cf* pts, float* m0, float* m1)
{
    constexpr int LOW = K < 4 ? K : 4, HIGH = K - LOW;
#pragma unroll
    for (int j = 0; j < K; ++j) m0[j] = m1[j] = __builtin_huge_valf();
    for (int hi = 0; hi < (1 << HIGH); ++hi) {
        float c = __builtin_huge_valf();
#pragma unroll
        for (int lo = 0; lo < (1 << LOW); ++lo) {
            const float d = dist2(x, pts[(hi << LOW) + lo]);
            c = fminf(c, d);
#pragma unroll
            for (int j = 0; j < LOW; ++j) {
                if ((lo >> (LOW - 1 - j)) & 1) m1[HIGH + j] = fminf(m1[HIGH + j], d);
                else m0[HIGH + j] = fminf(m0[HIGH + j], d);
            }
        }
#pragma unroll
        for (int j = 0; j < HIGH; ++j) {
            if ((hi >> (HIGH - 1 - j)) & 1) m1[j] = fminf(m1[j], c);
            else m0[j] = fminf(m0[j], c);
        }
    }
}

template <int K>
__global__ __launch_bounds__(kLanes) void k_symbols_soft(MapperArgs a, const cf* __restrict__ in, float* __restrict__ out)
{
    __shared__ cf pts[1 << K];
    __shared__ float llr[kSoftSlots];
    load_points<K>(pts, a);
    const int64_t n_live = live_rows(a.count, a.n_rows);
    const int64_t s_live = n_live * a.n_sym, live_f = s_live * K;
    const int mis = (int)(((uintptr_t)in / sizeof(cf)) & 1);
    const StreamTiles tl(out, 4, a.n_rows * a.n_sym * K, kTileVec);
    for (int64_t tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto t = tl.tile(tile);
        const int64_t f_lo = t.i_lo, f_live = std::min(t.i_hi, live_f);      // the floats [f_lo, f_live) hold LLRs
        int64_t s_base = 0;
        if (f_live > f_lo) {
            const int64_t s_lo = f_lo / K, s_hi = (f_live - 1) / K + 1;      // <= s_live
            const RowCursor first(s_lo, a.n_sym);
            const int64_t v_lo = (s_lo + mis) >> 1, v_end = (s_hi + mis + 1) >> 1;
            s_base = 2 * v_lo - mis;
            for (int64_t v = v_lo + threadIdx.x; v < v_end; v += kLanes) {
                cf x[2];
                load_pair(in, 2 * v - mis, s_live, x[0], x[1]);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int64_t s = 2 * v - mis + e;
                    const int slot = (int)(s - s_base) * K;
                    if (s < s_lo || s >= s_hi || slot + K > kSoftSlots) continue;
                    const float sc = a.scale ? a.scale[first.at((uint32_t)(s - s_lo)).r] : 1.f;
                    float m0[K], m1[K];
                    soft_minima<K>(x[e], pts, m0, m1);
#pragma unroll
                    for (int j = 0; j < K; ++j) llr[slot + j] = sc * (m1[j] - m0[j]);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t w = t.v0 + u * kLanes + threadIdx.x;
            if (w >= t.v1) continue;
            const int64_t f0 = tl.first(w);
            uint32_t y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t f = f0 + e;
                y[e] = (f >= f_lo && f < f_live) ? __float_as_uint(llr[(int)(f - s_base * K)]) : 0u;
            }
            store_elems<float, 4>(out, tl, f0, y);
        }
        __syncthreads();                             // llr is rewritten for the next tile
    }
}

template <int K>
__global__ __launch_bounds__(kLanes) void k_symbols_map(MapperArgs a, const unsigned char* __restrict__ in, cf* __restrict__ out)
{
    __shared__ uint2 pts[1 << K];                    // moved as bits: a point goes out as it came in
    for (int i = threadIdx.x; i < (1 << K); i += kLanes) pts[i] = reinterpret_cast<const uint2*>(a.points)[i];
    __syncthreads();
    const int64_t n_live = live_rows(a.count, a.n_rows);
    const int64_t s_live = n_live * a.n_sym;
    const StreamTiles tl(out, 2, a.n_rows * a.n_sym, kTileVec);
    for (int64_t tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto t = tl.tile(tile);
        const RowCursor first(t.i_lo, a.n_sym);
        uint32_t y[kTileVec / kLanes][4];            // all loads of a lane's vectors before its stores, so that their latencies overlap
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t w = t.v0 + u * kLanes + threadIdx.x;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int64_t s = tl.first(w) + e;
                y[u][2 * e] = y[u][2 * e + 1] = 0u;
                if (w >= t.v1 || s < 0 || s >= s_live) continue;
                const RowCursor pos = first.at((uint32_t)(s - t.i_lo));
                const int64_t q = pos.i * K, at = pos.r * a.row_bytes + (q >> 3);
                const int sh = (int)(q & 7);
                unsigned bits = (unsigned)in[at] << 8;
                if (sh + K > 8) bits |= in[at + 1];  // the symbol's own bits reach into that byte: it is inside the row
                const uint2 p = pts[(bits >> (16 - sh - K)) & ((1u << K) - 1u)];
                y[u][2 * e] = p.x;
                y[u][2 * e + 1] = p.y;
            }
        }
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t w = t.v0 + u * kLanes + threadIdx.x;
            if (w < t.v1) store_elems<uint2, 2>(reinterpret_cast<uint2*>(out), tl, tl.first(w), y[u]);
        }
    }
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int mapper_check(int n_points, int64_t n_sym, int64_t n_rows)
{
    const int k = bits_of(n_points);
    if (!k) return api_fail(GFDM_HIP_EINVAL, "a constellation needs 2, 4, 8, ..., 256 points");
    if (n_sym < 1) return api_fail(GFDM_HIP_EINVAL, "n_sym must be >= 1");
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    const int64_t per = std::max<int64_t>((int64_t)sizeof(cf), (int64_t)sizeof(float) * k);      // bytes per symbol: as a sample, as k LLRs
    if (n_sym > INT64_MAX / per || (n_rows > 0 && n_sym * per > INT64_MAX / n_rows))
        return api_fail(GFDM_HIP_EINVAL, "the byte size of the symbols or of the soft bits overflows int64");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_symbol_mapper {
    gfdm::DeviceCtx ctx;
    gfdm::Constellation c;
    ~gfdm_hip_symbol_mapper()
    {
        if (!c.d_points) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(c.d_points);
    }
};

namespace {

enum Op { OP_MAP, OP_DECODE, OP_SOFT };

template <int K>
void launch_k(const gfdm_hip_symbol_mapper* h, Op op, const MapperArgs& a, void* out, const void* in, hipStream_t s)
{
    const dim3 block(kLanes);
    if (op == OP_MAP) {
        const dim3 grid(row_grid(out, 2, a.n_rows * a.n_sym, kTileVec, kMaxTiles));
        hipLaunchKernelGGL(k_symbols_map<K>, grid, block, 0, s, a, static_cast<const unsigned char*>(in), static_cast<cf*>(out));
    } else if (op == OP_SOFT) {
        const dim3 grid(row_grid(out, 4, a.n_rows * a.n_sym * K, kTileVec, kMaxTiles));
        hipLaunchKernelGGL(k_symbols_soft<K>, grid, block, 0, s, a, static_cast<const cf*>(in), static_cast<float*>(out));
    } else {
        const int64_t ntiles = (a.n_rows * a.row_bytes + kLanes * K - 1) / (kLanes * K);
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, kMaxTiles)));
        const cf* x = static_cast<const cf*>(in);
        unsigned char* y = static_cast<unsigned char*>(out);
        gfdm::with_rule<K>(h->c.rule, [&](auto k, auto rule) {
            hipLaunchKernelGGL((k_symbols_decode<decltype(k)::value, decltype(rule)::value>), grid, block, 0, s, a, x, y);
        });
    }
}

// the one launch of a call.  Everything is a device pointer.
int mapper_enqueue(const gfdm_hip_symbol_mapper* h, Op op, void* out, const void* in, const void* scale, const void* count, int64_t n_sym, int64_t n_rows,
                   hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    const void* syms = op == OP_MAP ? out : in;
    if (misaligned(syms, sizeof(cf)) || (op == OP_SOFT && (misaligned(out, sizeof(float)) || misaligned(scale, sizeof(float)))) || misaligned(count, sizeof(int64_t)))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const MapperArgs a = { h->c.d_points, n_sym, n_rows, row_bytes_of(h->c.k, n_sym), static_cast<const int64_t*>(count), static_cast<const float*>(scale) };
    gfdm::dispatch_bits(h->c.k, [&](auto k) { launch_k<decltype(k)::value>(h, op, a, out, in, s); });
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int check_call(const gfdm_hip_symbol_mapper* h, const void* out, const void* in, int64_t n_sym, int64_t n_rows)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = mapper_check(1 << h->c.k, n_sym, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows > 0 && (!out || !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

int mapper_device(gfdm_hip_symbol_mapper* h, Op op, void* out, const void* in, const void* scale, const void* count, int64_t n_sym, int64_t n_rows, void* stream)
{
    const int rc = check_call(h, out, in, n_sym, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) { return mapper_enqueue(h, op, out, in, scale, count, n_sym, n_rows, s); });
}

// upload the rows (and the scale and the count), one enqueue on the handle's stream, download the result
int mapper_host(gfdm_hip_symbol_mapper* h, Op op, void* out, const void* in, const float* scale, const int64_t* count, int64_t n_sym, int64_t n_rows)
{
    const int rc0 = check_call(h, out, in, n_sym, n_rows);
    if (rc0 != GFDM_HIP_OK) return rc0;
    if (n_rows == 0) return GFDM_HIP_OK;
    const size_t n = (size_t)n_rows, sym_bytes = n * (size_t)n_sym * sizeof(cf), packed = n * (size_t)row_bytes_of(h->c.k, n_sym),
                 llr_bytes = n * (size_t)n_sym * h->c.k * sizeof(float);
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(in), op == OP_MAP ? packed : sym_bytes);
    const auto cnt = hc.in(count, 1);
    const auto sc = hc.in(scale, n);
    const auto y = hc.out(static_cast<unsigned char*>(out), op == OP_MAP ? sym_bytes : op == OP_DECODE ? packed : llr_bytes);
    return hc.run([&](hipStream_t s) { return mapper_enqueue(h, op, y.dev(), x.dev(), sc.dev(), cnt.dev(), n_sym, n_rows, s); });
}

}  // namespace

extern "C" {

int gfdm_hip_symbol_mapper_create(gfdm_hip_symbol_mapper** out, const float* points, int n_points, int decision, int device)
{
    return gfdm::create_handle(
        out, device, [&](gfdm_hip_symbol_mapper& h) { return h.c.set(points, n_points, decision); },
        [](gfdm_hip_symbol_mapper& h) { return h.c.upload(); });
}

int gfdm_hip_symbol_mapper_destroy(gfdm_hip_symbol_mapper* m) { delete m; return GFDM_HIP_OK; }
int gfdm_hip_symbol_mapper_bits_per_symbol(const gfdm_hip_symbol_mapper* m) { return m ? m->c.k : GFDM_HIP_EINVAL; }
int gfdm_hip_symbol_mapper_n_points(const gfdm_hip_symbol_mapper* m) { return m ? 1 << m->c.k : GFDM_HIP_EINVAL; }
int gfdm_hip_symbol_mapper_decision(const gfdm_hip_symbol_mapper* m) { return m ? m->c.rule : GFDM_HIP_EINVAL; }
int gfdm_hip_symbol_mapper_points(const gfdm_hip_symbol_mapper* m, float* points)
{
    if (!m || !points) return api_fail(GFDM_HIP_EINVAL, "NULL handle or output");
    std::copy(m->c.points, m->c.points + (1 << m->c.k), reinterpret_cast<cf*>(points));
    return GFDM_HIP_OK;
}
int64_t gfdm_hip_symbol_mapper_row_bytes(const gfdm_hip_symbol_mapper* m, int64_t n_sym)
{
    if (!m) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    const int rc = mapper_check(1 << m->c.k, n_sym, 0);
    return rc != GFDM_HIP_OK ? rc : row_bytes_of(m->c.k, n_sym);
}
int gfdm_hip_symbol_mapper_check(int n_points, int64_t n_sym, int64_t n_rows) { return mapper_check(n_points, n_sym, n_rows); }

int gfdm_hip_symbol_mapper_map_device(gfdm_hip_symbol_mapper* m, void* out, const void* data, const void* count, int64_t n_sym, int64_t n_rows, void* stream)
{
    return mapper_device(m, OP_MAP, out, data, nullptr, count, n_sym, n_rows, stream);
}
int gfdm_hip_symbol_mapper_map_host(gfdm_hip_symbol_mapper* m, float* out, const uint8_t* data, const int64_t* count, int64_t n_sym, int64_t n_rows)
{
    return mapper_host(m, OP_MAP, out, data, nullptr, count, n_sym, n_rows);
}
int gfdm_hip_symbol_mapper_decode_device(gfdm_hip_symbol_mapper* m, void* out, const void* symbols, const void* count, int64_t n_sym, int64_t n_rows,
                                         void* stream)
{
    return mapper_device(m, OP_DECODE, out, symbols, nullptr, count, n_sym, n_rows, stream);
}
int gfdm_hip_symbol_mapper_decode_host(gfdm_hip_symbol_mapper* m, uint8_t* out, const float* symbols, const int64_t* count, int64_t n_sym, int64_t n_rows)
{
    return mapper_host(m, OP_DECODE, out, symbols, nullptr, count, n_sym, n_rows);
}
int gfdm_hip_symbol_mapper_soft_device(gfdm_hip_symbol_mapper* m, void* out, const void* symbols, const void* scale, const void* count, int64_t n_sym,
                                       int64_t n_rows, void* stream)
{
    return mapper_device(m, OP_SOFT, out, symbols, scale, count, n_sym, n_rows, stream);
}
int gfdm_hip_symbol_mapper_soft_host(gfdm_hip_symbol_mapper* m, float* out, const float* symbols, const float* scale, const int64_t* count, int64_t n_sym,
                                     int64_t n_rows)
{
    return mapper_host(m, OP_SOFT, out, symbols, scale, count, n_sym, n_rows);
}

}  // extern "C"
