// Rate matching: puncturing and interleaving of the coded bits, between the convolutional code's encode and the symbol mapper's map on the
// transmit side (match), between soft and decode (unmatch) or the mapper's decode and decode (unmatch_hard) on the receive side.  The
// contract -- the pattern, the permutation and the gather convention, all integer index arithmetic -- is written out in include/gfdm_hip.h.
//
// create composes the pattern and the permutation ON THE HOST into two tables that are the same for every row: src[j], the coded bit behind
// transmitted bit j (n_tx entries), and inv[i], the transmitted bit behind coded bit i or -1 (n_coded entries).  Both live on the device in
// one allocation.  The kernels are pure gathers over the flat OUTPUT, on the row stages' tile skeleton (gfdm_rowtile.h).
//   Table reuse: a workgroup copies its table -- src for match, inv for the two unmatch calls -- into LDS once (4 n_coded bytes at most,
//   sized by the row: dynamic LDS) and then walks its tiles, so the table is fetched once per workgroup, not once per row.  The grid is
//   bounded by kMaxGrid, which is what gives a workgroup many rows per copy.  Rows of more than GFDM_HIP_RM_LDS_BITS coded bits read the
//   table through the cache instead (template parameter).
//   unmatch / unmatch_hard: a lane builds four floats (four lookups, four 4-byte or 1-byte reads) and stores them as one 16-byte vector.
//   match: a lane builds four bytes (32 lookups and 32 byte reads through the cache) and stores one aligned 4-byte word, 256 contiguous
//   bytes a wave.  Deviation from a 16-byte store per lane: the kernel is bound by its 8 lookups per output byte, not by its stores, and
//   a frame's transmitted row is some 80 bytes, so 16 bytes a lane would leave a batch of a few thousand rows on a fraction of the CUs.
// The spare rows, the padding behind a row and the punctured positions are written by the same kernel: every output element exactly once.
// Not here: fusing unmatch into the decoder's LLR fetch, per-row patterns, repetition.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"
#include "gfdm_rowtile.h"

#include <algorithm>
#include <climits>
#include <vector>

using gfdm::RowCursor;
using gfdm::StreamTiles;
using gfdm::api_fail;
using gfdm::check_width;
using gfdm::live_rows;
using gfdm::misaligned;
using gfdm::row_grid;
using gfdm::write_elems;

namespace {

constexpr int kLanes = 256;                          // lanes of a workgroup, and vectors (match: words) of a tile: one a lane
constexpr int kVps = 4;                              // elements of a vector: four floats in 16 bytes, four bytes in a word
static_assert(kVps * kLanes - 1 <= gfdm::kMaxRowReach, "the in-tile distance of RowCursor::at");
constexpr int kMaxGrid = 1024;                       // workgroups per launch: four per CU, each walks the tiles beyond
constexpr int64_t kMaxCoded = (int64_t)1 << 21;      // twice the convolutional code's 2^20 trellis steps
constexpr int kMaxPeriod = 4096;

struct MatchArgs {
    const unsigned char* in;     // [n_rows][in_row_bytes]
    unsigned char* out;          // [n_rows][out_row_bytes]
    const int64_t* count;        // optional (device)
    const int32_t* src;          // [n_tx]
    int64_t n_rows, in_row_bytes, out_row_bytes;
    int n_tx;
};

struct UnmatchArgs {
    const void* in;              // soft: float [n_rows][in_width]; hard: uint8 [n_rows][in_width]
    uint32_t* out;               // float [n_rows][out_stride], written as bit patterns
    const int64_t* count;
    const int32_t* inv;          // [n_coded]
    int64_t n_rows, in_width, out_stride;
    int n_coded;
};

// the workgroup's copy of a table of n entries, where the row is short enough for one
template <bool LDS>
__device__ __forceinline__ void stage_table(int32_t* lds, const int32_t* __restrict__ table, int n)
{
    if constexpr (LDS) {
        for (int j = threadIdx.x; j < n; j += kLanes) lds[j] = table[j];
        __syncthreads();
    }
}

// byte i of a transmitted row: the coded bits src[8 i] .. src[8 i + 7], MSB first; 0 behind the n_tx bits
template <bool LDS>
__device__ __forceinline__ unsigned match_byte(const MatchArgs& a, const int32_t* lds, const unsigned char* __restrict__ row, int64_t i)
{
    const int64_t j0 = 8 * i;
    if (j0 >= a.n_tx) return 0u;
    unsigned byte = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int j = (int)j0 + b;
        if (j >= a.n_tx) break;
        const int s = LDS ? lds[j] : a.src[j];       // 0 <= s < n_coded <= 8 in_row_bytes
        byte |= ((row[s >> 3] >> (7 - (s & 7))) & 1u) << (7 - b);
    }
    return byte;
}

template <bool LDS>
__global__ __launch_bounds__(kLanes) void k_rm_match(MatchArgs a)
{
    extern __shared__ int32_t lds_table[];
    stage_table<LDS>(lds_table, a.src, a.n_tx);
    const int64_t n_live = live_rows(a.count, a.n_rows), orb = a.out_row_bytes;
    const StreamTiles tl(a.out, kVps, a.n_rows * orb, kLanes, 4);            // 4-byte words (above)
    for (int64_t tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto t = tl.tile(tile);
        const int64_t w = t.v0 + threadIdx.x;
        if (w >= t.v1) continue;
        write_elems<unsigned char, kVps>(a.out, tl, t, RowCursor(t.i_lo, orb), w, n_live,
                                         [&](int64_t r, int64_t i) { return match_byte<LDS>(a, lds_table, a.in + r * a.in_row_bytes, i); });
    }
}

// float i of a depunctured row, as its bit pattern: the transmitted value behind coded bit i, +0.0f where there is none
template <bool HARD, bool LDS>
__device__ __forceinline__ uint32_t unmatch_value(const UnmatchArgs& a, const int32_t* lds, int64_t r, int64_t i)
{
    if (i >= a.n_coded) return 0u;
    const int j = LDS ? lds[i] : a.inv[i];           // -1, or 0 <= j < n_tx <= in_stride, n_tx <= 8 in_row_bytes
    if (j < 0) return 0u;
    if constexpr (HARD) {
        const unsigned b = static_cast<const unsigned char*>(a.in)[r * a.in_width + (j >> 3)];
        return 0x3f800000u | (((b >> (7 - (j & 7))) & 1u) << 31);      // +1.0f for a 0 bit, -1.0f for a 1 bit
    } else {
        return static_cast<const uint32_t*>(a.in)[r * a.in_width + j];
    }
}

template <bool HARD, bool LDS>
__global__ __launch_bounds__(kLanes) void k_rm_unmatch(UnmatchArgs a)
{
    extern __shared__ int32_t lds_table[];
    stage_table<LDS>(lds_table, a.inv, a.n_coded);
    const int64_t n_live = live_rows(a.count, a.n_rows), os = a.out_stride;
    const StreamTiles tl(a.out, kVps, a.n_rows * os, kLanes);
    for (int64_t tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto t = tl.tile(tile);
        const int64_t w = t.v0 + threadIdx.x;
        if (w >= t.v1) continue;
        write_elems<uint32_t, kVps>(a.out, tl, t, RowCursor(t.i_lo, os), w, n_live,
                                    [&](int64_t r, int64_t i) { return unmatch_value<HARD, LDS>(a, lds_table, r, i); });
    }
}

// bits of a coded row of n_coded bits that the pattern keeps (arguments checked by the caller)
int64_t kept_of(int64_t n_coded, const uint8_t* keep, int period)
{
    int64_t per_period = 0, head = 0;
    const int64_t rest = n_coded % period;
    for (int i = 0; i < period; ++i) {
        if (!keep[i]) continue;
        ++per_period;
        if (i < rest) ++head;
    }
    return n_coded / period * per_period + head;
}

int pattern_check(int64_t n_coded, const uint8_t* keep, int period)
{
    if (n_coded < 1 || n_coded > kMaxCoded) return api_fail(GFDM_HIP_EINVAL, "n_coded must satisfy 1 <= n_coded <= 2^21");
    if (period < 1 || period > kMaxPeriod) return api_fail(GFDM_HIP_EINVAL, "the period of the puncturing pattern must satisfy 1 <= period <= 4096");
    if (!keep) return api_fail(GFDM_HIP_EINVAL, "NULL puncturing pattern");
    if (kept_of(n_coded, keep, period) < 1) return api_fail(GFDM_HIP_EINVAL, "the puncturing pattern keeps no bit of the row");
    return GFDM_HIP_OK;
}

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int matcher_check(int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm, int64_t n_rows)
{
    const int rc = pattern_check(n_coded, keep, period);
    if (rc != GFDM_HIP_OK) return rc;
    if (perm) {
        const int64_t n_tx = kept_of(n_coded, keep, period);
        if (n_perm != n_tx) return api_fail(GFDM_HIP_EINVAL, "perm must have one entry for every transmitted bit (gfdm_hip_rate_matcher_tx_bits_of)");
        std::vector<bool> seen((size_t)n_tx, false);
        for (int64_t j = 0; j < n_tx; ++j) {
            if (perm[j] < 0 || perm[j] >= n_tx || seen[(size_t)perm[j]]) return api_fail(GFDM_HIP_EINVAL, "perm is not a permutation of 0 .. n_tx - 1");
            seen[(size_t)perm[j]] = true;
        }
    }
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    const int64_t per = n_coded * (int64_t)sizeof(float);                             // the widest row: its LLRs
    if (n_rows > 0 && per > INT64_MAX / n_rows) return api_fail(GFDM_HIP_EINVAL, "the byte size of the rows overflows int64");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_rate_matcher {
    gfdm::DeviceCtx ctx;
    int64_t n_coded = 0, n_tx = 0;
    std::vector<int32_t> src, inv;                   // src[j]: the coded bit behind transmitted bit j; inv[i]: its inverse, -1 where punctured
    int32_t* d_tables = nullptr;                     // src, then inv
    const int32_t* d_src() const { return d_tables; }
    const int32_t* d_inv() const { return d_tables + n_tx; }
    ~gfdm_hip_rate_matcher()
    {
        if (!d_tables) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(d_tables);
    }
};

namespace {

enum Op { OP_MATCH, OP_SOFT, OP_HARD };

// the argument checks and the two tables: no device yet
int compose(gfdm_hip_rate_matcher& h, int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm)
{
    const int rc = matcher_check(n_coded, keep, period, perm, n_perm, 0);
    if (rc != GFDM_HIP_OK) return rc;
    h.n_coded = n_coded;
    h.n_tx = kept_of(n_coded, keep, period);
    std::vector<int32_t> kept;
    kept.reserve((size_t)h.n_tx);
    for (int64_t i = 0; i < n_coded; ++i)
        if (keep[i % period]) kept.push_back((int32_t)i);
    h.src.resize((size_t)h.n_tx);
    h.inv.assign((size_t)n_coded, -1);
    for (int64_t j = 0; j < h.n_tx; ++j) {
        h.src[(size_t)j] = kept[(size_t)(perm ? perm[j] : j)];
        h.inv[(size_t)h.src[(size_t)j]] = (int32_t)j;
    }
    return GFDM_HIP_OK;
}

// the tables on the handle's device (which is current)
int upload(gfdm_hip_rate_matcher& h)
{
    const size_t n_src = h.src.size() * sizeof(int32_t), n_inv = h.inv.size() * sizeof(int32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h.d_tables), n_src + n_inv);
    if (e == hipSuccess) e = hipMemcpy(h.d_tables, h.src.data(), n_src, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h.d_tables + h.src.size(), h.inv.data(), n_inv, hipMemcpyHostToDevice);
    return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "rate matcher table upload");
}

int64_t tx_bytes_of(const gfdm_hip_rate_matcher* h) { return (h->n_tx + 7) / 8; }

int check_call(const gfdm_hip_rate_matcher* h, Op op, const void* out, const void* in, int64_t in_width, int64_t out_width, int64_t n_rows)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    int rc;
    switch (op) {
    case OP_MATCH:
        rc = check_width(in_width, (h->n_coded + 7) / 8, 1, n_rows, "in_row_bytes");
        if (rc == GFDM_HIP_OK) rc = check_width(out_width, tx_bytes_of(h), 1, n_rows, "out_row_bytes");
        break;
    case OP_SOFT:
        rc = check_width(in_width, h->n_tx, sizeof(float), n_rows, "in_stride");
        if (rc == GFDM_HIP_OK) rc = check_width(out_width, h->n_coded, sizeof(float), n_rows, "out_stride");
        break;
    default:
        rc = check_width(in_width, tx_bytes_of(h), 1, n_rows, "in_row_bytes");
        if (rc == GFDM_HIP_OK) rc = check_width(out_width, h->n_coded, sizeof(float), n_rows, "out_stride");
        break;
    }
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows > 0 && (!out || !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

// the one launch of a call.  Everything is a device pointer.
int enqueue(const gfdm_hip_rate_matcher* h, Op op, void* out, const void* in, const void* count, int64_t in_width, int64_t out_width, int64_t n_rows,
            hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(count, sizeof(int64_t)) || (op != OP_MATCH && misaligned(out, sizeof(float))) || (op == OP_SOFT && misaligned(in, sizeof(float))))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const bool lds = h->n_coded <= GFDM_HIP_RM_LDS_BITS;
    const dim3 block(kLanes);
    if (op == OP_MATCH) {
        const MatchArgs a = { static_cast<const unsigned char*>(in), static_cast<unsigned char*>(out), static_cast<const int64_t*>(count), h->d_src(),
                              n_rows, in_width, out_width, (int)h->n_tx };
        const dim3 grid(row_grid(out, kVps, n_rows * out_width, kLanes, kMaxGrid, 4));
        if (lds) hipLaunchKernelGGL(k_rm_match<true>, grid, block, (size_t)h->n_tx * sizeof(int32_t), s, a);
        else hipLaunchKernelGGL(k_rm_match<false>, grid, block, 0, s, a);
    } else {
        const UnmatchArgs a = { in, static_cast<uint32_t*>(out), static_cast<const int64_t*>(count), h->d_inv(), n_rows, in_width, out_width, (int)h->n_coded };
        const dim3 grid(row_grid(out, kVps, n_rows * out_width, kLanes, kMaxGrid));
        const size_t bytes = lds ? (size_t)h->n_coded * sizeof(int32_t) : 0;
        if (op == OP_SOFT) {
            if (lds) hipLaunchKernelGGL((k_rm_unmatch<false, true>), grid, block, bytes, s, a);
            else hipLaunchKernelGGL((k_rm_unmatch<false, false>), grid, block, bytes, s, a);
        } else {
            if (lds) hipLaunchKernelGGL((k_rm_unmatch<true, true>), grid, block, bytes, s, a);
            else hipLaunchKernelGGL((k_rm_unmatch<true, false>), grid, block, bytes, s, a);
        }
    }
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// upload the rows (and the count), one enqueue on the handle's stream, download the result
int call_host(gfdm_hip_rate_matcher* h, Op op, void* out, const void* in, const int64_t* count, int64_t in_width, int64_t out_width, int64_t n_rows)
{
    const int rc = check_call(h, op, out, in, in_width, out_width, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows == 0) return GFDM_HIP_OK;
    const size_t n = (size_t)n_rows;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(in), n * (size_t)in_width * (op == OP_SOFT ? sizeof(float) : 1));
    const auto cnt = hc.in(count, 1);
    const auto y = hc.out(static_cast<unsigned char*>(out), n * (size_t)out_width * (op == OP_MATCH ? 1 : sizeof(float)));
    return hc.run([&](hipStream_t s) { return enqueue(h, op, y.dev(), x.dev(), cnt.dev(), in_width, out_width, n_rows, s); });
}

int call_device(gfdm_hip_rate_matcher* h, Op op, void* out, const void* in, const void* count, int64_t in_width, int64_t out_width, int64_t n_rows,
                void* stream)
{
    const int rc = check_call(h, op, out, in, in_width, out_width, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) { return enqueue(h, op, out, in, count, in_width, out_width, n_rows, s); });
}

}  // namespace

extern "C" {

int gfdm_hip_rate_matcher_create(gfdm_hip_rate_matcher** out, int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm,
                                 int device)
{
    return gfdm::create_handle(
        out, device, [&](gfdm_hip_rate_matcher& h) { return compose(h, n_coded, keep, period, perm, n_perm); },
        [](gfdm_hip_rate_matcher& h) { return upload(h); });
}

int gfdm_hip_rate_matcher_destroy(gfdm_hip_rate_matcher* r) { delete r; return GFDM_HIP_OK; }
int64_t gfdm_hip_rate_matcher_coded_bits(const gfdm_hip_rate_matcher* r) { return r ? r->n_coded : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_rate_matcher_tx_bits(const gfdm_hip_rate_matcher* r) { return r ? r->n_tx : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_rate_matcher_tx_bytes(const gfdm_hip_rate_matcher* r) { return r ? tx_bytes_of(r) : GFDM_HIP_EINVAL; }
int gfdm_hip_rate_matcher_source_index(const gfdm_hip_rate_matcher* r, int32_t* src)
{
    if (!r || !src) return api_fail(GFDM_HIP_EINVAL, "NULL handle or buffer");
    std::copy(r->src.begin(), r->src.end(), src);
    return GFDM_HIP_OK;
}
int64_t gfdm_hip_rate_matcher_tx_bits_of(int64_t n_coded, const uint8_t* keep, int period)
{
    const int rc = pattern_check(n_coded, keep, period);
    return rc != GFDM_HIP_OK ? rc : kept_of(n_coded, keep, period);
}
int gfdm_hip_rate_matcher_check(int64_t n_coded, const uint8_t* keep, int period, const int32_t* perm, int64_t n_perm, int64_t n_rows)
{
    return matcher_check(n_coded, keep, period, perm, n_perm, n_rows);
}

int gfdm_hip_rate_matcher_match_host(gfdm_hip_rate_matcher* r, uint8_t* out, const uint8_t* coded, const int64_t* count, int64_t in_row_bytes,
                                     int64_t out_row_bytes, int64_t n_rows)
{
    return call_host(r, OP_MATCH, out, coded, count, in_row_bytes, out_row_bytes, n_rows);
}
int gfdm_hip_rate_matcher_match_device(gfdm_hip_rate_matcher* r, void* out, const void* coded, const void* count, int64_t in_row_bytes,
                                       int64_t out_row_bytes, int64_t n_rows, void* stream)
{
    return call_device(r, OP_MATCH, out, coded, count, in_row_bytes, out_row_bytes, n_rows, stream);
}
int gfdm_hip_rate_matcher_unmatch_host(gfdm_hip_rate_matcher* r, float* out, const float* llr, const int64_t* count, int64_t in_stride, int64_t out_stride,
                                       int64_t n_rows)
{
    return call_host(r, OP_SOFT, out, llr, count, in_stride, out_stride, n_rows);
}
int gfdm_hip_rate_matcher_unmatch_device(gfdm_hip_rate_matcher* r, void* out, const void* llr, const void* count, int64_t in_stride, int64_t out_stride,
                                         int64_t n_rows, void* stream)
{
    return call_device(r, OP_SOFT, out, llr, count, in_stride, out_stride, n_rows, stream);
}
int gfdm_hip_rate_matcher_unmatch_hard_host(gfdm_hip_rate_matcher* r, float* out, const uint8_t* tx, const int64_t* count, int64_t in_row_bytes,
                                            int64_t out_stride, int64_t n_rows)
{
    return call_host(r, OP_HARD, out, tx, count, in_row_bytes, out_stride, n_rows);
}
int gfdm_hip_rate_matcher_unmatch_hard_device(gfdm_hip_rate_matcher* r, void* out, const void* tx, const void* count, int64_t in_row_bytes,
                                              int64_t out_stride, int64_t n_rows, void* stream)
{
    return call_device(r, OP_HARD, out, tx, count, in_row_bytes, out_stride, n_rows, stream);
}

}  // extern "C"
