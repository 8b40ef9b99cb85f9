// Convolutional code, constraint length 7, rate 1/2 (default generators 171 / 133 octal = GNU Radio's polys [109, 79]): the encoder in front
// of the symbol mapper's map and the soft- / hard-input Viterbi decoder behind its soft / decode.  The contract -- the code, the quantiser,
// the path metrics, the tie rule and the traceback, all in integers -- is written out in include/gfdm_hip.h.
//
// decode: ONE WAVEFRONT PER ROW, lane = trellis state (64 states, 64 lanes), four rows per 256-lane workgroup, rows strided over a bounded
//   grid.  The waves of a workgroup never meet: there is no __syncthreads anywhere.
//   forward:   the trellis goes by in chunks of 64 steps.  Lane l loads the two LLRs of step base + l (8 bytes a lane, 512 contiguous bytes
//              a wave; two 4-byte loads where the row's pairs are only 4-byte aligned), quantises them and keeps them packed in one
//              register; the next chunk's pair is loaded before this chunk's steps run.  The step loop is unrolled over the chunk, so the
//              pair of step j reaches every lane through a lane read with a compile-time index.  A step fetches PM[s >> 1] and
//              PM[(s >> 1) + 32] from the other lanes (two ds_bpermute), adds the two branch metrics (four per-lane signs computed from
//              the generators at kernel start, so generators with bit 0 or bit 6 clear need no special case), compares, selects, and
//              __ballot(m1 > m0) is the step's 64 survivor decisions.  Lane j keeps the word of step j; after the chunk every lane
//              stores its word: 512 contiguous bytes a wave, into LDS while the row has at most GFDM_HIP_CC_LDS_STEPS steps (16 KiB a
//              wave), else into this wave's slot of the caller's workspace.
//   traceback: lane l reads back the word IT stored (so neither LDS nor the workspace carries anything between lanes), and the serial walk
//              over the chunk selects bits from words broadcast by lane reads with compile-time indices: no dependent memory load per step.
//              The state is wave-uniform.  The 64 information bits of a chunk are assembled in one word and lanes 0 .. 7 store its bytes.
//   The hard flavour is the same kernel with the other fetch (template parameter): +1 / -1 from a packed coded row.
//   Deviation from the first sketch: the LDS of a launch is sized by the row (dynamic), not by the budget, so short rows keep the SIMDs full.
// encode: element-wise, on the row stages' tile skeleton (gfdm_rowtile.h).  Output byte o of a row needs the information bits 4 o - 6 ..
//   4 o + 3: two bytes, read through the cache.  The zero padding behind the 2 T coded bits and the spare rows are written by the same kernel.
// Not here: tail-biting and streaming modes, other constraint lengths or mother-code rates, int8 LLR input.  Puncturing and interleaving
// are gfdm_ratematch.hip's.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"
#include "gfdm_rowtile.h"

#include <algorithm>
#include <climits>
#include <cmath>

using gfdm::RowCursor;
using gfdm::StreamTiles;
using gfdm::write_elems;
using gfdm::api_fail;
using gfdm::check_width;
using gfdm::live_rows;
using gfdm::misaligned;

namespace {

constexpr int kLanes = 256;
constexpr int kWaves = kLanes / 64;                  // rows per workgroup
constexpr int kChunk = 64;                           // trellis steps per chunk: one decision word per lane
constexpr int kMaxSteps = 1 << 20;                   // 2^20 * 254 < 2^30 - 2^28: no metric leaves int32
constexpr int kMaxGrid = 2048;                       // decode workgroups per launch (LDS variant); the rows beyond are strided over
constexpr int kWsWaves = 2048;                       // decode waves per launch of the workspace variant: one workspace slot each
constexpr int kTileVec = kLanes;                     // encode: 16-byte vectors of output per tile (4 KiB): a byte costs two loads and eight parities, so one vector a lane
constexpr int kMaxTiles = 8192;
constexpr int kVps = 16;                             // encode: coded bytes per vector
static_assert(kVps * kTileVec - 1 <= gfdm::kMaxRowReach, "the in-tile distance of RowCursor::at");

struct DecodeArgs {
    const void* in;              // soft: float [n_rows][stride]; hard: uint8 [n_rows][stride]
    unsigned char* out;          // [n_rows][info_bytes]
    int32_t* path_metric;        // optional [n_rows]
    const int64_t* count;        // optional (device)
    unsigned long long* ws;      // workspace variant: [waves of the launch][tpad]
    int64_t n_rows, stride, info_bytes;
    int n_info, steps, tpad;     // tpad: steps rounded up to whole chunks
    int g0, g1, mode;
    float gain;
};

struct EncodeArgs {
    const unsigned char* in;     // [n_rows][info_bytes]
    unsigned char* out;          // [n_rows][out_row_bytes]
    const int64_t* count;
    int64_t n_rows, info_bytes, out_row_bytes;
    int n_info, steps;
    int g0, g1;
};

// c_i(R) = parity(R & |g|) ^ (g < 0)
__device__ __forceinline__ int coded_bit(int R, int g)
{
    const int mag = g < 0 ? -g : g;
    return (__popc((unsigned)(R & mag)) & 1) ^ (g < 0 ? 1 : 0);
}

// q = clamp(rintf(llr * gain), -127, 127); NaN gives 0
__device__ __forceinline__ int quantise(float llr, float gain)
{
    float v = rintf(llr * gain);
    if (!(v == v)) v = 0.f;
    return (int)fminf(fmaxf(v, -127.f), 127.f);
}

__device__ __forceinline__ int pack_pair(int q0, int q1) { return (q0 & 0xffff) | (q1 << 16); }

// the packed soft values of step t of a row (0 beyond the trellis: never read there)
template <bool HARD>
__device__ __forceinline__ int fetch_pair(const void* row, int t, int steps, float gain, bool pairs_aligned)
{
    if (t >= steps) return 0;
    if constexpr (HARD) {
        const unsigned b = static_cast<const unsigned char*>(row)[t >> 2];
        const unsigned pair = (b >> (6 - 2 * (t & 3))) & 3u;
        return pack_pair(1 - 2 * (int)(pair >> 1), 1 - 2 * (int)(pair & 1u));
    } else {
        const float* p = static_cast<const float*>(row) + 2 * (int64_t)t;
        float x0, x1;
        if (pairs_aligned) {
            const float2 v = *reinterpret_cast<const float2*>(p);
            x0 = v.x;
            x1 = v.y;
        } else {
            x0 = p[0];
            x1 = p[1];
        }
        return pack_pair(quantise(x0, gain), quantise(x1, gain));
    }
}

template <bool HARD, bool WS>
__global__ __launch_bounds__(kLanes) void k_cc_decode(DecodeArgs a)
{
    extern __shared__ unsigned long long lds_words[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* const dec = WS ? a.ws + ((int64_t)blockIdx.x * kWaves + wave) * a.tpad : lds_words + wave * a.tpad;
    // the signs 1 - 2 c_i(R) of this state's two incoming transitions, R = s | (b << 6)
    const int s00 = 1 - 2 * coded_bit(lane, a.g0), s01 = 1 - 2 * coded_bit(lane, a.g1);
    const int s10 = 1 - 2 * coded_bit(lane | 64, a.g0), s11 = 1 - 2 * coded_bit(lane | 64, a.g1);
    const int from0 = 4 * (lane >> 1), from1 = 4 * ((lane >> 1) + 32);            // ds_bpermute takes byte addresses
    const int64_t n_live = live_rows(a.count, a.n_rows);
    const int T = a.steps;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < a.n_rows; row += (int64_t)gridDim.x * kWaves) {
        unsigned char* const out = a.out + row * a.info_bytes;
        if (row >= n_live) {                         // a spare row: zeros, its input is never read
            for (int64_t b = lane; b < a.info_bytes; b += 64) out[b] = 0;
            if (a.path_metric && lane == 0) a.path_metric[row] = 0;
            continue;
        }
        const void* const in = HARD ? (const void*)(static_cast<const unsigned char*>(a.in) + row * a.stride)
                                    : (const void*)(static_cast<const float*>(a.in) + row * a.stride);
        const bool pairs_aligned = ((uintptr_t)in & 7) == 0;
        int pm = lane == 0 ? 0 : -(1 << 30);
        int cur = fetch_pair<HARD>(in, lane, T, a.gain, pairs_aligned);
        for (int base = 0; base < T; base += kChunk) {
            const int nxt = fetch_pair<HARD>(in, base + kChunk + lane, T, a.gain, pairs_aligned);
            const int n = std::min(kChunk, T - base);
            unsigned long long word = 0;
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                if (j < n) {                         // wave-uniform: only a row's last chunk is short
                    const int sq = __builtin_amdgcn_readlane(cur, j);
                    const int q0 = (short)(sq & 0xffff), q1 = sq >> 16;
                    const int p0 = __builtin_amdgcn_ds_bpermute(from0, pm), p1 = __builtin_amdgcn_ds_bpermute(from1, pm);
                    const int m0 = p0 + s00 * q0 + s01 * q1, m1 = p1 + s10 * q0 + s11 * q1;
                    const bool take = m1 > m0;       // strict: a tie keeps b = 0
                    const unsigned long long decisions = __ballot(take);
                    pm = take ? m1 : m0;
                    if (lane == j) word = decisions;
                }
            }
            dec[base + lane] = word;
            cur = nxt;
        }
        // start state and its metric
        int state = 0, metric = __builtin_amdgcn_readlane(pm, 0);
        if (a.mode == GFDM_HIP_CC_TRUNCATED) {
            int best = pm;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) best = std::max(best, __shfl_xor(best, d));
            const unsigned long long at = __ballot(pm == best);
            state = __ffsll((long long)at) - 1;      // the first state of maximal metric
            metric = best;
        }
        state = __builtin_amdgcn_readfirstlane(state);
        if (a.path_metric && lane == 0) a.path_metric[row] = metric;
        for (int base = (T - 1) / kChunk * kChunk; base >= 0; base -= kChunk) {
            const unsigned long long word = dec[base + lane];                      // the word this lane stored
            const unsigned lo = (unsigned)word, hi = (unsigned)(word >> 32);
            const int n = std::min(kChunk, T - base);
            unsigned long long bits = 0;             // u of step base + j at bit 63 - j: the chunk's 8 bytes, MSB first
#pragma unroll
            for (int j = kChunk - 1; j >= 0; --j) {
                if (j < n) {
                    const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, j) << 32) |
                                                 (unsigned)__builtin_amdgcn_readlane((int)lo, j);
                    bits |= (unsigned long long)(state & 1) << (63 - j);
                    state = (state >> 1) | ((int)((w >> state) & 1ull) << 5);
                }
            }
            const int valid = a.n_info - base;       // the tail bits and the spare bits of the last byte go out as 0
            if (valid <= 0) bits = 0;
            else if (valid < 64) bits &= ~0ull << (64 - valid);
            const int64_t b = base / 8 + lane;
            if (lane < 8 && b < a.info_bytes) out[b] = (unsigned char)(bits >> (56 - 8 * lane));
        }
    }
}

// byte i of a coded row: steps 4 i .. 4 i + 3, from the information bits 4 i - 6 .. 4 i + 3
__device__ __forceinline__ unsigned encode_byte(const EncodeArgs& a, const unsigned char* __restrict__ row, int64_t i)
{
    const int64_t t0 = 4 * i;
    if (t0 >= a.steps) return 0u;
    const int64_t b0 = (t0 - 6) >> 3;                // floor: -1 for the first byte
    unsigned w = 0;
    if (b0 >= 0 && b0 < a.info_bytes) w = (unsigned)row[b0] << 8;
    if (b0 + 1 < a.info_bytes) w |= row[b0 + 1];
    const int64_t keep = (int64_t)a.n_info - 8 * b0; // bits of the window that are information bits (>= 1 here)
    if (keep < 16) w &= ~(0xffffu >> (int)keep);
    unsigned byte = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t t = t0 + k;
        if (t >= a.steps) break;
        const int R = (int)((w >> (15 - (int)(t - 8 * b0))) & 127u);
        byte |= (unsigned)coded_bit(R, a.g0) << (7 - 2 * k);
        byte |= (unsigned)coded_bit(R, a.g1) << (6 - 2 * k);
    }
    return byte;
}

__global__ __launch_bounds__(kLanes) void k_cc_encode(EncodeArgs a)
{
    const int64_t n_live = live_rows(a.count, a.n_rows), orb = a.out_row_bytes;
    const StreamTiles tl(a.out, kVps, a.n_rows * orb, kTileVec);
    for (int64_t tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto t = tl.tile(tile);
        const RowCursor first(t.i_lo, orb);
#pragma unroll
        for (int u = 0; u < kTileVec / kLanes; ++u) {
            const int64_t w = t.v0 + u * kLanes + threadIdx.x;
            if (w < t.v1)
                write_elems<unsigned char, kVps>(a.out, tl, t, first, w, n_live, [&](int64_t r, int64_t i) { return encode_byte(a, a.in + r * a.info_bytes, i); });
        }
    }
}

int64_t steps_of(int mode, int64_t n_info) { return mode == GFDM_HIP_CC_TERMINATED ? n_info + 6 : n_info; }
int64_t tpad_of(int64_t steps) { return (steps + kChunk - 1) / kChunk * kChunk; }

// the argument table (include/gfdm_hip.h); needs no handle, so it is checked before any device is touched
int code_check(int poly0, int poly1, int mode, int64_t n_info, int64_t n_rows)
{
    for (int g : { poly0, poly1 })
        if (g == 0 || g > 127 || g < -127) return api_fail(GFDM_HIP_EINVAL, "a generator polynomial must satisfy 1 <= |g| <= 127");
    if (mode != GFDM_HIP_CC_TERMINATED && mode != GFDM_HIP_CC_TRUNCATED) return api_fail(GFDM_HIP_EINVAL, "unknown mode of the convolutional code");
    if (n_info < 1) return api_fail(GFDM_HIP_EINVAL, "n_info must be >= 1");
    if (n_info > kMaxSteps || steps_of(mode, n_info) > kMaxSteps) return api_fail(GFDM_HIP_EINVAL, "a row has more than 2^20 trellis steps");
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    const int64_t per = 2 * steps_of(mode, n_info) * (int64_t)sizeof(float);       // the widest row: its LLRs
    if (n_rows > 0 && per > INT64_MAX / n_rows) return api_fail(GFDM_HIP_EINVAL, "the byte size of the rows overflows int64");
    return GFDM_HIP_OK;
}

}  // namespace

struct gfdm_hip_conv_code {
    gfdm::DeviceCtx ctx;
    int g[2] = { 109, 79 };
    int mode = GFDM_HIP_CC_TERMINATED;
};

namespace {

enum Op { OP_SOFT, OP_HARD };

struct Geometry {
    int64_t steps, coded_bits, coded_bytes, info_bytes;
};

Geometry geometry_of(const gfdm_hip_conv_code* h, int64_t n_info)
{
    const int64_t t = steps_of(h->mode, n_info);
    return { t, 2 * t, (2 * t + 7) / 8, (n_info + 7) / 8 };
}

int64_t decode_waves(int64_t n_rows) { return std::min<int64_t>(std::max<int64_t>(n_rows, 1), kWsWaves); }

int64_t workspace_bytes_of(const gfdm_hip_conv_code* h, int64_t n_info, int64_t n_rows)
{
    const int64_t t = steps_of(h->mode, n_info);
    if (t <= GFDM_HIP_CC_LDS_STEPS || n_rows == 0) return 0;
    return decode_waves(n_rows) * tpad_of(t) * (int64_t)sizeof(unsigned long long);
}

int check_handle(const gfdm_hip_conv_code* h, int64_t n_info, int64_t n_rows)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    return code_check(h->g[0], h->g[1], h->mode, n_info, n_rows);
}

int check_encode(const gfdm_hip_conv_code* h, const void* out, const void* data, int64_t n_info, int64_t out_row_bytes, int64_t n_rows)
{
    int rc = check_handle(h, n_info, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    rc = check_width(out_row_bytes, geometry_of(h, n_info).coded_bytes, 1, n_rows, "out_row_bytes");
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows > 0 && (!out || !data)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

int check_decode(const gfdm_hip_conv_code* h, Op op, const void* out, const void* in, int64_t n_info, int64_t stride, float gain, int64_t n_rows)
{
    int rc = check_handle(h, n_info, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    const Geometry geo = geometry_of(h, n_info);
    rc = op == OP_SOFT ? check_width(stride, geo.coded_bits, sizeof(float), n_rows, "llr_stride") : check_width(stride, geo.coded_bytes, 1, n_rows, "in_row_bytes");
    if (rc != GFDM_HIP_OK) return rc;
    if (op == OP_SOFT && !(std::isfinite(gain) && gain > 0.f)) return api_fail(GFDM_HIP_EINVAL, "gain must be finite and > 0");
    if (n_rows > 0 && (!out || !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

// the one launch of an encode.  Everything is a device pointer.
int encode_enqueue(const gfdm_hip_conv_code* h, void* out, const void* data, const void* count, int64_t n_info, int64_t out_row_bytes, int64_t n_rows,
                   hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(count, sizeof(int64_t))) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const Geometry geo = geometry_of(h, n_info);
    const EncodeArgs a = { static_cast<const unsigned char*>(data), static_cast<unsigned char*>(out), static_cast<const int64_t*>(count), n_rows,
                           geo.info_bytes, out_row_bytes, (int)n_info, (int)geo.steps, h->g[0], h->g[1] };
    hipLaunchKernelGGL(k_cc_encode, dim3(gfdm::row_grid(out, kVps, n_rows * out_row_bytes, kTileVec, kMaxTiles)), dim3(kLanes), 0, s, a);
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

// the one launch of a decode
int decode_enqueue(const gfdm_hip_conv_code* h, Op op, void* out, void* path_metric, const void* in, const void* count, int64_t n_info, int64_t stride,
                   float gain, int64_t n_rows, void* workspace, hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(count, sizeof(int64_t)) || misaligned(path_metric, sizeof(int32_t)) || (op == OP_SOFT && misaligned(in, sizeof(float))))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    const Geometry geo = geometry_of(h, n_info);
    const bool ws = geo.steps > GFDM_HIP_CC_LDS_STEPS;
    if (ws && !workspace) return api_fail(GFDM_HIP_EINVAL, "rows of this length need a workspace (gfdm_hip_conv_code_decode_workspace_bytes)");
    if (ws && misaligned(workspace, 16)) return api_fail(GFDM_HIP_EINVAL, "the workspace must be 16-byte aligned");
    const int tpad = (int)tpad_of(geo.steps);
    const DecodeArgs a = { in, static_cast<unsigned char*>(out), static_cast<int32_t*>(path_metric), static_cast<const int64_t*>(count),
                           ws ? static_cast<unsigned long long*>(workspace) : nullptr, n_rows, stride, geo.info_bytes, (int)n_info, (int)geo.steps, tpad,
                           h->g[0], h->g[1], h->mode, gain };
    const int64_t groups = ws ? (decode_waves(n_rows) + kWaves - 1) / kWaves : std::min<int64_t>((n_rows + kWaves - 1) / kWaves, kMaxGrid);
    const dim3 grid((unsigned)groups), block(kLanes);
    const size_t lds = ws ? 0 : (size_t)kWaves * tpad * sizeof(unsigned long long);
    if (op == OP_SOFT) {
        if (ws) hipLaunchKernelGGL((k_cc_decode<false, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((k_cc_decode<false, false>), grid, block, lds, s, a);
    } else {
        if (ws) hipLaunchKernelGGL((k_cc_decode<true, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((k_cc_decode<true, false>), grid, block, lds, s, a);
    }
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int encode_host(gfdm_hip_conv_code* h, uint8_t* out, const uint8_t* data, const int64_t* count, int64_t n_info, int64_t out_row_bytes, int64_t n_rows)
{
    const int rc0 = check_encode(h, out, data, n_info, out_row_bytes, n_rows);
    if (rc0 != GFDM_HIP_OK) return rc0;
    if (n_rows == 0) return GFDM_HIP_OK;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(data, (size_t)n_rows * (size_t)geometry_of(h, n_info).info_bytes);
    const auto cnt = hc.in(count, 1);
    const auto y = hc.out(out, (size_t)n_rows * (size_t)out_row_bytes);
    return hc.run([&](hipStream_t s) { return encode_enqueue(h, y.dev(), x.dev(), cnt.dev(), n_info, out_row_bytes, n_rows, s); });
}

// upload the rows (and the count), one enqueue on the handle's stream with a workspace of the call's own, download the result
int decode_host(gfdm_hip_conv_code* h, Op op, uint8_t* out, int32_t* path_metric, const void* in, const int64_t* count, int64_t n_info, int64_t stride,
                float gain, int64_t n_rows)
{
    const int rc0 = check_decode(h, op, out, in, n_info, stride, gain, n_rows);
    if (rc0 != GFDM_HIP_OK) return rc0;
    if (n_rows == 0) return GFDM_HIP_OK;
    const size_t n = (size_t)n_rows;
    gfdm::HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const unsigned char*>(in), n * (size_t)stride * (op == OP_SOFT ? sizeof(float) : 1));
    const auto cnt = hc.in(count, 1);
    const auto y = hc.out(out, n * (size_t)geometry_of(h, n_info).info_bytes);
    const auto pm = hc.out(path_metric, n);
    const auto ws = hc.scratch<unsigned char>((size_t)workspace_bytes_of(h, n_info, n_rows));
    return hc.run([&](hipStream_t s) {
        return decode_enqueue(h, op, y.dev(), pm.dev(), x.dev(), cnt.dev(), n_info, stride, gain, n_rows, ws.dev(), s);
    });
}

int decode_device(gfdm_hip_conv_code* h, Op op, void* out, void* path_metric, const void* in, const void* count, int64_t n_info, int64_t stride, float gain,
                  int64_t n_rows, void* workspace, void* stream)
{
    const int rc = check_decode(h, op, out, in, n_info, stride, gain, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(h->ctx.device, stream, [&](hipStream_t s) {
        return decode_enqueue(h, op, out, path_metric, in, count, n_info, stride, gain, n_rows, workspace, s);
    });
}

// a size getter: the status code where the arguments are bad
template <class F>
int64_t size_of(const gfdm_hip_conv_code* c, int64_t n_info, int64_t n_rows, F f)
{
    const int rc = check_handle(c, n_info, n_rows);
    return rc != GFDM_HIP_OK ? rc : f();
}

}  // namespace

extern "C" {

int gfdm_hip_conv_code_create(gfdm_hip_conv_code** out, int poly0, int poly1, int mode, int device)
{
    return gfdm::create_handle(out, device, [&](gfdm_hip_conv_code& h) {
        h.g[0] = poly0;
        h.g[1] = poly1;
        h.mode = mode;
        return code_check(poly0, poly1, mode, 1, 0);
    });
}

int gfdm_hip_conv_code_destroy(gfdm_hip_conv_code* c) { delete c; return GFDM_HIP_OK; }
int gfdm_hip_conv_code_poly(const gfdm_hip_conv_code* c, int i) { return (c && (i == 0 || i == 1)) ? c->g[i] : 0; }
int gfdm_hip_conv_code_mode(const gfdm_hip_conv_code* c) { return c ? c->mode : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_conv_code_steps(const gfdm_hip_conv_code* c, int64_t n_info)
{
    return size_of(c, n_info, 0, [&] { return geometry_of(c, n_info).steps; });
}
int64_t gfdm_hip_conv_code_coded_bits(const gfdm_hip_conv_code* c, int64_t n_info)
{
    return size_of(c, n_info, 0, [&] { return geometry_of(c, n_info).coded_bits; });
}
int64_t gfdm_hip_conv_code_coded_bytes(const gfdm_hip_conv_code* c, int64_t n_info)
{
    return size_of(c, n_info, 0, [&] { return geometry_of(c, n_info).coded_bytes; });
}
int64_t gfdm_hip_conv_code_info_bytes(const gfdm_hip_conv_code* c, int64_t n_info)
{
    return size_of(c, n_info, 0, [&] { return geometry_of(c, n_info).info_bytes; });
}
int64_t gfdm_hip_conv_code_decode_workspace_bytes(const gfdm_hip_conv_code* c, int64_t n_info, int64_t n_rows)
{
    return size_of(c, n_info, n_rows, [&] { return workspace_bytes_of(c, n_info, n_rows); });
}
int gfdm_hip_conv_code_check(int poly0, int poly1, int mode, int64_t n_info, int64_t n_rows) { return code_check(poly0, poly1, mode, n_info, n_rows); }

int gfdm_hip_conv_code_encode_host(gfdm_hip_conv_code* c, uint8_t* out, const uint8_t* data, const int64_t* count, int64_t n_info, int64_t out_row_bytes,
                                   int64_t n_rows)
{
    return encode_host(c, out, data, count, n_info, out_row_bytes, n_rows);
}
int gfdm_hip_conv_code_encode_device(gfdm_hip_conv_code* c, void* out, const void* data, const void* count, int64_t n_info, int64_t out_row_bytes,
                                     int64_t n_rows, void* stream)
{
    const int rc = check_encode(c, out, data, n_info, out_row_bytes, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(c->ctx.device, stream, [&](hipStream_t s) { return encode_enqueue(c, out, data, count, n_info, out_row_bytes, n_rows, s); });
}
int gfdm_hip_conv_code_decode_host(gfdm_hip_conv_code* c, uint8_t* out, int32_t* path_metric, const float* llr, const int64_t* count, int64_t n_info,
                                   int64_t llr_stride, float gain, int64_t n_rows)
{
    return decode_host(c, OP_SOFT, out, path_metric, llr, count, n_info, llr_stride, gain, n_rows);
}
int gfdm_hip_conv_code_decode_device(gfdm_hip_conv_code* c, void* out, void* path_metric, const void* llr, const void* count, int64_t n_info,
                                     int64_t llr_stride, float gain, int64_t n_rows, void* workspace, void* stream)
{
    return decode_device(c, OP_SOFT, out, path_metric, llr, count, n_info, llr_stride, gain, n_rows, workspace, stream);
}
int gfdm_hip_conv_code_decode_hard_host(gfdm_hip_conv_code* c, uint8_t* out, int32_t* path_metric, const uint8_t* coded, const int64_t* count,
                                        int64_t n_info, int64_t in_row_bytes, int64_t n_rows)
{
    return decode_host(c, OP_HARD, out, path_metric, coded, count, n_info, in_row_bytes, 1.f, n_rows);
}
int gfdm_hip_conv_code_decode_hard_device(gfdm_hip_conv_code* c, void* out, void* path_metric, const void* coded, const void* count, int64_t n_info,
                                          int64_t in_row_bytes, int64_t n_rows, void* workspace, void* stream)
{
    return decode_device(c, OP_HARD, out, path_metric, coded, count, n_info, in_row_bytes, 1.f, n_rows, workspace, stream);
}

}  // extern "C"
