// Frame check: CRC-32 and whitening of payload rows, in front of the convolutional code's encode on the transmit side (attach) and behind
// its decode on the receive side (verify).  The contract -- the bitwise CRC, the LFSR of the whitening sequence, the row layouts, all
// integer arithmetic -- is written out in include/gfdm_hip.h.
//
// The CRC without its two XORs is linear over GF(2): with raw(m) the register after the bytes of m from a register of 0,
// raw(A || B) = raw(A) x^(8 |B|) + raw(B) mod P.  A row is cut into the 16-byte chunks of its memory layout, chunk c at bytes 16 c ..:
//   Group of lanes per row: G = min(64, next power of two >= ceil(frame_bytes / 16)) lanes own a row, a wavefront holds 64 / G rows, a
//   workgroup 256 / G; rows of more than 1024 bytes are walked in `steps` steps of 64 chunks.  The grid follows the number of rows and
//   is bounded by kMaxGrid; a workgroup walks the row groups beyond.
//   One lane, one chunk: a 16-byte load where the whole chunk belongs to the row (the address may be any: the target's unaligned
//   access mode), byte loads at the cut end; the whitening chunk from the handle's padded copy; raw(chunk) by slicing-by-4 from four
//   256-entry tables in LDS (16 reads in chains of four, not one chain of 16); the product with pos[c] = x^(8 (n - 16 c - 16)) mod P,
//   n the bytes the CRC runs over, as a 32-step shift-and-XOR.  The exponent of the cut chunk is negative -- it undoes the zeros the
//   chunk was padded with -- and taken modulo 2^32 - 1, the order of the multiplicative group (P is irreducible).  The group
//   XOR-reduces with __shfl_xor in log2 G steps.  Deviation from a running value shifted once per step: every chunk position has its
//   constant in the table (4 bytes per 16 of the row), so long rows take the same path as short ones and no lane waits for the last.
//   The initial 0xFFFFFFFF and the final XOR are one constant per handle (`fold`): attach's CRC is raw(payload) ^ crc(zeros); verify
//   compares raw(dewhitened frame) with the raw value of a good frame -- the residue, which by the bijection of the last four bytes
//   holds exactly when the stored CRC is the payload's.
//   Output in the same pass: verify writes the dewhitened payload chunk and ok from the registers it loaded; attach writes every chunk
//   as it goes except the one or two that carry CRC bytes, which their lanes hold until the reduction.  The bytes a row lacks to its
//   width are zeros from the lanes that own them; what lies behind the G * steps chunks of a wide row is written by the group, strided.
//   LDS banking: the table index is data dependent, 32 lanes over 32 banks (ds_read_b32).  Interleaved replicas leave as many lanes
//   as banks in every class, so they were not built; one lane one bank would take 64 KiB per table.
// good_row / n_good: a second, small kernel over ok (described above it): a workgroup per 4096 rows, up to 256 workgroups, each of which
// counts the flags in front of its rows itself instead of waiting for another workgroup, so there is no scratch and no third kernel.
// Not here: per-row seeds, other polynomials, moving the good rows to the front, fusing verify into decode's traceback.
#include "../../include/gfdm_hip.h"
#include "gfdm_decide.h"
#include "gfdm_hostcall.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

using gfdm::api_fail;
using gfdm::check_width;
using gfdm::live_rows;
using gfdm::misaligned;

namespace {

constexpr int kLanes = 256;
constexpr int kMaxGrid = 2048;                       // workgroups per launch: eight per CU, each walks the row groups beyond
constexpr int64_t kMaxPayload = ((int64_t)1 << 17) - 4;
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kScanLanes = 256, kScanPer = 16, kScanTile = kScanLanes * kScanPer, kScanMaxGrid = 256;        // the scan of ok: 16 flags a lane

// one zero bit through the register: a product with x (bit 31 is x^0)
__host__ __device__ __forceinline__ uint32_t times_x(uint32_t r) { return (r >> 1) ^ (kPoly & (0u - (r & 1u))); }

// a(x) b(x) mod P
__host__ __device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = times_x(b);
    }
    return p;
}

struct CheckArgs {
    const unsigned char* in;     // attach: payload [n_rows][in_w]; verify: frames [n_rows][in_w]
    unsigned char* out;          // attach: frames [n_rows][out_w]; verify: payload [n_rows][out_w] or NULL
    unsigned char* ok;           // verify: [n_rows]
    const int64_t* count;        // optional (device)
    const uint32_t* tables;      // [4][256]
    const uint4* seq;            // the whitening sequence, [G * steps] chunks, zeros behind frame_bytes
    const uint32_t* pos;         // [G * steps]
    int64_t n_rows, in_w, out_w;
    int n_in;                    // the bytes of a row that are read and that the CRC runs over: n_payload (attach), frame_bytes (verify)
    int n_payload;
    int lg, steps;               // log2 G; chunks of a row = G * steps
    uint32_t fold;
};

__device__ __forceinline__ uint4 operator^(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

// the k bytes at p (k <= 0: none; k >= 16: a whole chunk) as a little-endian chunk, zeros behind them
__device__ __forceinline__ uint4 load_chunk(const unsigned char* __restrict__ p, int k)
{
    uint32_t t[4] = { 0u, 0u, 0u, 0u };
    if (k >= 16) {
        __builtin_memcpy(t, p, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < k) t[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
    return make_uint4(t[0], t[1], t[2], t[3]);
}

// the first k bytes of chunk w to p (k <= 0: none)
__device__ __forceinline__ void store_chunk(unsigned char* __restrict__ p, uint4 w, int64_t k)
{
    const uint32_t t[4] = { w.x, w.y, w.z, w.w };
    if (k >= 16) {
        __builtin_memcpy(p, t, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < k) p[j] = (unsigned char)(t[j >> 2] >> (8 * (j & 3)));
    }
}

// word i of a chunk keeps its bytes below byte d of the chunk
__device__ __forceinline__ uint32_t keep_word(uint32_t w, int d)
{
    return d >= 4 ? w : d <= 0 ? 0u : w & ((1u << (8 * d)) - 1u);
}
__device__ __forceinline__ uint4 keep_low(uint4 w, int d)
{
    return make_uint4(keep_word(w.x, d), keep_word(w.y, d - 4), keep_word(w.z, d - 8), keep_word(w.w, d - 12));
}

// what a word sees of the four bytes of v, least significant first, that start d bytes behind the word's first
__device__ __forceinline__ uint32_t place_word(uint32_t v, int d)
{
    return (d <= -4 || d >= 4) ? 0u : d >= 0 ? v << (8 * d) : v >> (-8 * d);
}
__device__ __forceinline__ uint4 place(uint32_t v, int d)
{
    return make_uint4(place_word(v, d), place_word(v, d - 4), place_word(v, d - 8), place_word(v, d - 12));
}

// raw(chunk): slicing-by-4 over the workgroup's tables, tab[k][b] = raw of byte b followed by k zero bytes
__device__ __forceinline__ uint32_t raw_word(const uint32_t* tab, uint32_t r, uint32_t w)
{
    r ^= w;
    return tab[768 + (r & 255u)] ^ tab[512 + ((r >> 8) & 255u)] ^ tab[256 + ((r >> 16) & 255u)] ^ tab[r >> 24];
}
__device__ __forceinline__ uint32_t raw_chunk(const uint32_t* tab, uint4 w)
{
    return raw_word(tab, raw_word(tab, raw_word(tab, raw_word(tab, 0u, w.x), w.y), w.z), w.w);
}

template <bool VERIFY>
__global__ __launch_bounds__(kLanes) void k_fc_rows(CheckArgs a)
{
    __shared__ uint32_t tab[1024];
    reinterpret_cast<uint4*>(tab)[threadIdx.x] = reinterpret_cast<const uint4*>(a.tables)[threadIdx.x];
    __syncthreads();
    const int64_t n_live = live_rows(a.count, a.n_rows);
    const int G = 1 << a.lg, g = (int)threadIdx.x & (G - 1), rows_per_pass = kLanes >> a.lg;
    const int64_t npass = (a.n_rows + rows_per_pass - 1) / rows_per_pass;
    const int64_t covered = (int64_t)16 * G * a.steps;
    const bool store = !VERIFY || a.out != nullptr;
    for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {     // (uniform in the workgroup: every lane takes part in the shuffles)
        const int64_t r = pass * rows_per_pass + ((int)threadIdx.x >> a.lg);
        const bool exists = r < a.n_rows, live = r < n_live;
        const int64_t in_at = exists ? r * a.in_w : 0, out_at = exists ? r * a.out_w : 0;
        uint32_t acc = 0;
        uint4 held = make_uint4(0u, 0u, 0u, 0u);
        int held_base = -1;
        for (int s = 0; s < a.steps; ++s) {
            const int c = (s << a.lg) + g, base = 16 * c;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (live) {
                w = load_chunk(a.in + in_at + base, a.n_in - base);
                if constexpr (VERIFY) w = w ^ a.seq[c];
            }
            acc ^= mulmod(a.pos[c], raw_chunk(tab, w));
            if constexpr (VERIFY) {
                if (store && exists) store_chunk(a.out + out_at + base, keep_low(w, a.n_payload - base), a.out_w - base);
            } else {
                if (base + 16 > a.n_payload && base < a.n_payload + 4) {         // carries CRC bytes: written behind the reduction
                    held = w;
                    held_base = base;
                } else if (exists) {
                    if (live) w = w ^ a.seq[c];
                    store_chunk(a.out + out_at + base, w, a.out_w - base);
                }
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) acc ^= __shfl_xor(acc, m, 64);
        if constexpr (VERIFY) {
            if (g == 0 && exists) a.ok[r] = (unsigned char)(live && acc == a.fold);
        } else {
            if (held_base >= 0 && exists) {
                if (live) held = held ^ place(acc ^ a.fold, a.n_payload - held_base) ^ a.seq[held_base >> 4];
                store_chunk(a.out + out_at + held_base, held, a.out_w - held_base);
            }
        }
        if (store && exists)
            for (int64_t j = covered + g; j < a.out_w; j += G) a.out[out_at + j] = 0;
    }
}

// The flags of the 16 rows from i0 on (i0 a multiple of 16), little-endian, zeros behind n_rows.  ok was written by k_fc_rows: 0 or 1.
__device__ __forceinline__ uint4 flags16(const unsigned char* __restrict__ ok, int64_t i0, int64_t n_rows) { return load_chunk(ok + i0, (int)std::min<int64_t>(n_rows - i0, 16)); }
__device__ __forceinline__ int count16(uint4 w)
{
    return __popc(w.x & 0x01010101u) + __popc(w.y & 0x01010101u) + __popc(w.z & 0x01010101u) + __popc(w.w & 0x01010101u);
}

// the sum of v over the workgroup, in every lane (sums: one slot per wave; a barrier in front protects its reuse)
__device__ __forceinline__ int64_t workgroup_sum(int64_t v, int64_t* sums)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = v;
    __syncthreads();
    int64_t total = 0;
#pragma unroll
    for (int w = 0; w < kScanLanes / 64; ++w) total += sums[w];
    return total;
}

// good_row[0 .. n_good-1]: the rows with ok = 1 in ascending order; -1 behind them.  Workgroup k owns the rows [k tile, (k + 1) tile), tile a
// multiple of kScanTile, and waits for nobody: it counts the flags in front of its rows and all flags itself (n_rows bytes in 16-byte
// loads: the flags are a 64th of what verify read), writes the indices of its good rows from there on -- a lane takes 16 consecutive
// flags, a wave scan with __shfl_up and the wave sums through LDS give its place --, and the -1 of the places p >= n_good among ITS
// places p, so that every element of good_row is written once.
__global__ __launch_bounds__(kScanLanes) void k_fc_good(const unsigned char* __restrict__ ok, int64_t* __restrict__ good_row, int64_t* __restrict__ n_good,
                                                        int64_t n_rows, int64_t tile)
{
    __shared__ int64_t sums[kScanLanes / 64];
    __shared__ int wave_sum[kScanLanes / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t lo = (int64_t)blockIdx.x * tile, hi = std::min(lo + tile, n_rows);
    int64_t before = 0, all = 0;
#pragma unroll 4
    for (int64_t i0 = (int64_t)kScanPer * t; i0 < n_rows; i0 += kScanTile) {
        const int n = count16(flags16(ok, i0, n_rows));
        all += n;
        if (i0 < lo) before += n;
    }
    int64_t base = workgroup_sum(before, sums);
    const int64_t n_all = workgroup_sum(all, sums);
    for (int64_t t0 = lo; t0 < hi; t0 += kScanTile) {
        const int64_t i0 = t0 + (int64_t)kScanPer * t;
        const uint4 w = i0 < hi ? flags16(ok, i0, n_rows) : make_uint4(0u, 0u, 0u, 0u);
        const int mine = count16(w);
        int upto = mine;                                                   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(upto, d, 64);
            if (lane >= d) upto += v;
        }
        if (lane == 63) wave_sum[wave] = upto;
        __syncthreads();
        int in_front = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kScanLanes / 64; ++k) {
            const int n = wave_sum[k];
            if (k < wave) in_front += n;
            total += n;
        }
        int64_t o = base + in_front + upto - mine;
        const uint32_t word[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int e = 0; e < kScanPer; ++e)
            if ((word[e >> 2] >> (8 * (e & 3))) & 1u) good_row[o++] = i0 + e;
        base += total;
        __syncthreads();                                                   // wave_sum is written again by the next tile
    }
    for (int64_t p = std::max(lo, n_all) + t; p < hi; p += kScanLanes) good_row[p] = -1;
    if (blockIdx.x == 0 && t == 0) *n_good = n_all;
}

// ---- host: the argument table, the sequence and the constants ----

int table_check(int64_t n_payload, uint64_t mask, uint64_t seed, int degree, int64_t n_rows)
{
    if (n_payload < 1 || n_payload > kMaxPayload) return api_fail(GFDM_HIP_EINVAL, "n_payload must satisfy 1 <= n_payload <= 2^17 - 4");
    if (degree < 0 || degree > 32) return api_fail(GFDM_HIP_EINVAL, "degree must be 0 (no whitening) or 1 .. 32");
    if (degree > 0) {
        const uint64_t lim = (uint64_t)1 << degree;
        if (mask < 1 || mask >= lim) return api_fail(GFDM_HIP_EINVAL, "mask must satisfy 1 <= mask < 2^degree");
        if (seed < 1 || seed >= lim) return api_fail(GFDM_HIP_EINVAL, "seed must satisfy 1 <= seed < 2^degree");
    }
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    const int64_t per = std::max<int64_t>(n_payload + 4, (int64_t)sizeof(int64_t));      // the widest row, or its entry of good_row
    if (n_rows > 0 && per > INT64_MAX / n_rows) return api_fail(GFDM_HIP_EINVAL, "the byte size of the rows overflows int64");
    return GFDM_HIP_OK;
}

uint32_t byte_step(uint32_t r, unsigned b)
{
    r ^= b;
    for (int i = 0; i < 8; ++i) r = times_x(r);
    return r;
}

// x^e mod P for any integer e: the exponent modulo the group order 2^32 - 1
uint32_t x_to(int64_t e)
{
    const int64_t order = ((int64_t)1 << 32) - 1;
    uint64_t n = (uint64_t)(((e % order) + order) % order);
    uint32_t r = 0x80000000u, sq = 0x40000000u;      // x^0, x^1
    for (; n; n >>= 1) {
        if (n & 1) r = mulmod(r, sq);
        sq = mulmod(sq, sq);
    }
    return r;
}

}  // namespace

struct gfdm_hip_frame_check {
    gfdm::DeviceCtx ctx;
    int64_t n_payload = 0;
    int lg = 0, steps = 1;
    uint32_t fold_attach = 0, fold_verify = 0;
    std::vector<uint8_t> seq;                        // frame_bytes
    std::vector<uint32_t> image;                     // what the device keeps: tables [4][256], seq as chunks, pos of attach, pos of verify
    uint32_t* d_image = nullptr;
    int64_t frame_bytes() const { return n_payload + 4; }
    int chunks() const { return steps << lg; }
    const uint32_t* d_tables() const { return d_image; }
    const uint4* d_seq() const { return reinterpret_cast<const uint4*>(d_image + 1024); }
    const uint32_t* d_pos(bool verify) const { return d_image + 1024 + (size_t)chunks() * (verify ? 5 : 4); }
    ~gfdm_hip_frame_check()
    {
        if (!d_image) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(d_image);
    }
};

namespace {

// the argument checks, the sequence, the tables and the constants: no device yet
int compose(gfdm_hip_frame_check& h, int64_t n_payload, uint64_t mask, uint64_t seed, int degree)
{
    const int rc = table_check(n_payload, mask, seed, degree, 0);
    if (rc != GFDM_HIP_OK) return rc;
    h.n_payload = n_payload;
    const int64_t fb = h.frame_bytes();
    const int64_t need = (fb + 15) / 16;
    while ((1 << h.lg) < need && h.lg < 6) ++h.lg;
    h.steps = (int)((need + (1 << h.lg) - 1) >> h.lg);
    const size_t nch = (size_t)h.chunks();
    h.seq.assign((size_t)fb, 0);
    if (degree > 0) {
        uint64_t s = seed;
        for (int64_t i = 0; i < 8 * fb; ++i) {
            h.seq[(size_t)(i >> 3)] |= (uint8_t)((s & 1u) << (7 - (i & 7)));
            s = (s >> 1) | ((uint64_t)__builtin_parityll(s & mask) << (degree - 1));
        }
    }
    h.image.assign(1024 + 6 * nch, 0u);
    uint32_t* tab = h.image.data();
    for (unsigned b = 0; b < 256; ++b) tab[b] = byte_step(0u, b);
    for (int k = 1; k < 4; ++k)
        for (unsigned b = 0; b < 256; ++b) tab[256 * k + b] = (tab[256 * (k - 1) + b] >> 8) ^ tab[tab[256 * (k - 1) + b] & 255u];
    std::memcpy(h.image.data() + 1024, h.seq.data(), (size_t)fb);
    for (size_t c = 0; c < nch; ++c) {
        h.image[1024 + 4 * nch + c] = x_to(8 * (n_payload - 16 * (int64_t)c - 16));
        h.image[1024 + 5 * nch + c] = x_to(8 * (fb - 16 * (int64_t)c - 16));
    }
    uint32_t r = 0xFFFFFFFFu;                        // crc of n_payload zero bytes: crc(m) = raw(m) ^ crc(zeros)
    for (int64_t i = 0; i < n_payload; ++i) r = byte_step(r, 0u);
    h.fold_attach = r ^ 0xFFFFFFFFu;
    r = 0;                                           // raw of a good frame, the one of the all-zero payload: its leading zeros leave the register at 0
    for (int j = 0; j < 4; ++j) r = byte_step(r, (h.fold_attach >> (8 * j)) & 255u);
    h.fold_verify = r;
    return GFDM_HIP_OK;
}

// the image on the handle's device (which is current)
int upload(gfdm_hip_frame_check& h)
{
    const size_t bytes = h.image.size() * sizeof(uint32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h.d_image), bytes);
    if (e == hipSuccess) e = hipMemcpy(h.d_image, h.image.data(), bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? GFDM_HIP_OK : gfdm::api_fail_hip(e, "frame check table upload");
}

struct VerifyOut {
    void* payload;
    void* ok;
    void* good_row;
    void* n_good;
};

int check_attach(const gfdm_hip_frame_check* h, const void* out, const void* in, int64_t in_w, int64_t out_w, int64_t n_rows)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    int rc = check_width(in_w, h->n_payload, 1, n_rows, "in_row_bytes");
    if (rc == GFDM_HIP_OK) rc = check_width(out_w, h->frame_bytes(), 1, n_rows, "out_row_bytes");
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows > 0 && (!out || !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

int check_verify(const gfdm_hip_frame_check* h, const VerifyOut& o, const void* in, int64_t in_w, int64_t out_w, int64_t n_rows)
{
    if (!h) return api_fail(GFDM_HIP_EINVAL, "NULL handle");
    if (n_rows < 0) return api_fail(GFDM_HIP_EINVAL, "n_rows must be >= 0");
    int rc = check_width(in_w, h->frame_bytes(), 1, n_rows, "in_row_bytes");
    if (rc == GFDM_HIP_OK && o.payload) rc = check_width(out_w, h->n_payload, 1, n_rows, "out_row_bytes");
    if (rc == GFDM_HIP_OK) rc = check_width(1, 1, sizeof(int64_t), n_rows, "good_row");
    if (rc != GFDM_HIP_OK) return rc;
    if ((o.good_row == nullptr) != (o.n_good == nullptr)) return api_fail(GFDM_HIP_EINVAL, "good_row and n_good go together: both or neither");
    if (n_rows > 0 && (!o.ok || !in)) return api_fail(GFDM_HIP_EINVAL, "NULL buffer");
    return GFDM_HIP_OK;
}

unsigned grid_for(const gfdm_hip_frame_check* h, int64_t n_rows)
{
    const int64_t rows_per_pass = kLanes >> h->lg;
    return (unsigned)std::min<int64_t>((n_rows + rows_per_pass - 1) / rows_per_pass, kMaxGrid);
}

CheckArgs args_of(const gfdm_hip_frame_check* h, bool verify, void* out, void* ok, const void* in, const void* count, int64_t in_w, int64_t out_w,
                  int64_t n_rows)
{
    return { static_cast<const unsigned char*>(in), static_cast<unsigned char*>(out), static_cast<unsigned char*>(ok), static_cast<const int64_t*>(count),
             h->d_tables(), h->d_seq(), h->d_pos(verify), n_rows, in_w, out_w, (int)(verify ? h->frame_bytes() : h->n_payload), (int)h->n_payload,
             h->lg, h->steps, verify ? h->fold_verify : h->fold_attach };
}

// the launches of a call.  Everything is a device pointer.
int enqueue_attach(const gfdm_hip_frame_check* h, void* out, const void* in, const void* count, int64_t in_w, int64_t out_w, int64_t n_rows, hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(count, sizeof(int64_t))) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    hipLaunchKernelGGL(k_fc_rows<false>, dim3(grid_for(h, n_rows)), dim3(kLanes), 0, s, args_of(h, false, out, nullptr, in, count, in_w, out_w, n_rows));
    GFDM_TRY(hipGetLastError());
    return GFDM_HIP_OK;
}

int enqueue_verify(const gfdm_hip_frame_check* h, const VerifyOut& o, const void* in, const void* count, int64_t in_w, int64_t out_w, int64_t n_rows,
                   hipStream_t s)
{
    if (n_rows == 0) return GFDM_HIP_OK;
    if (misaligned(count, sizeof(int64_t)) || misaligned(o.good_row, sizeof(int64_t)) || misaligned(o.n_good, sizeof(int64_t)))
        return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
    hipLaunchKernelGGL(k_fc_rows<true>, dim3(grid_for(h, n_rows)), dim3(kLanes), 0, s, args_of(h, true, o.payload, o.ok, in, count, in_w, out_w, n_rows));
    GFDM_TRY(hipGetLastError());
    if (o.good_row) {
        const int64_t tile = kScanTile * ((n_rows + (int64_t)kScanTile * kScanMaxGrid - 1) / ((int64_t)kScanTile * kScanMaxGrid));
        hipLaunchKernelGGL(k_fc_good, dim3((unsigned)((n_rows + tile - 1) / tile)), dim3(kScanLanes), 0, s, static_cast<const unsigned char*>(o.ok),
                           static_cast<int64_t*>(o.good_row), static_cast<int64_t*>(o.n_good), n_rows, tile);
        GFDM_TRY(hipGetLastError());
    }
    return GFDM_HIP_OK;
}

}  // namespace

extern "C" {

int gfdm_hip_frame_check_create(gfdm_hip_frame_check** out, int64_t n_payload, uint64_t mask, uint64_t seed, int degree, int device)
{
    return gfdm::create_handle(
        out, device, [&](gfdm_hip_frame_check& h) { return compose(h, n_payload, mask, seed, degree); }, [](gfdm_hip_frame_check& h) { return upload(h); });
}

int gfdm_hip_frame_check_destroy(gfdm_hip_frame_check* c) { delete c; return GFDM_HIP_OK; }
int64_t gfdm_hip_frame_check_payload_bytes(const gfdm_hip_frame_check* c) { return c ? c->n_payload : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_frame_check_frame_bytes(const gfdm_hip_frame_check* c) { return c ? c->frame_bytes() : GFDM_HIP_EINVAL; }
int64_t gfdm_hip_frame_check_frame_bits(const gfdm_hip_frame_check* c) { return c ? 8 * c->frame_bytes() : GFDM_HIP_EINVAL; }
int gfdm_hip_frame_check_whitening(const gfdm_hip_frame_check* c, uint8_t* seq)
{
    if (!c || !seq) return api_fail(GFDM_HIP_EINVAL, "NULL handle or buffer");
    std::copy(c->seq.begin(), c->seq.end(), seq);
    return GFDM_HIP_OK;
}
int gfdm_hip_frame_check_check(int64_t n_payload, uint64_t mask, uint64_t seed, int degree, int64_t n_rows)
{
    return table_check(n_payload, mask, seed, degree, n_rows);
}

int gfdm_hip_frame_check_attach_host(gfdm_hip_frame_check* c, uint8_t* out, const uint8_t* payload, const int64_t* count, int64_t in_row_bytes,
                                     int64_t out_row_bytes, int64_t n_rows)
{
    const int rc = check_attach(c, out, payload, in_row_bytes, out_row_bytes, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows == 0) return GFDM_HIP_OK;
    gfdm::HostCall hc(c->ctx);
    const auto x = hc.in(payload, (size_t)n_rows * (size_t)in_row_bytes);
    const auto cnt = hc.in(count, 1);
    const auto y = hc.out(out, (size_t)n_rows * (size_t)out_row_bytes);
    return hc.run([&](hipStream_t s) { return enqueue_attach(c, y.dev(), x.dev(), cnt.dev(), in_row_bytes, out_row_bytes, n_rows, s); });
}
int gfdm_hip_frame_check_attach_device(gfdm_hip_frame_check* c, void* out, const void* payload, const void* count, int64_t in_row_bytes,
                                       int64_t out_row_bytes, int64_t n_rows, void* stream)
{
    const int rc = check_attach(c, out, payload, in_row_bytes, out_row_bytes, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(c->ctx.device, stream,
                           [&](hipStream_t s) { return enqueue_attach(c, out, payload, count, in_row_bytes, out_row_bytes, n_rows, s); });
}
int gfdm_hip_frame_check_verify_host(gfdm_hip_frame_check* c, uint8_t* payload, uint8_t* ok, int64_t* good_row, int64_t* n_good, const uint8_t* frames,
                                     const int64_t* count, int64_t in_row_bytes, int64_t out_row_bytes, int64_t n_rows)
{
    const int rc = check_verify(c, VerifyOut{ payload, ok, good_row, n_good }, frames, in_row_bytes, out_row_bytes, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    if (n_rows == 0) return GFDM_HIP_OK;
    gfdm::HostCall hc(c->ctx);
    const auto x = hc.in(frames, (size_t)n_rows * (size_t)in_row_bytes);
    const auto cnt = hc.in(count, 1);
    const auto y = hc.out(payload, (size_t)n_rows * (size_t)out_row_bytes);
    const auto k = hc.out(ok, (size_t)n_rows);
    const auto gr = hc.out(good_row, (size_t)n_rows);
    const auto ng = hc.out(n_good, 1);
    return hc.run([&](hipStream_t s) {
        return enqueue_verify(c, VerifyOut{ y.dev(), k.dev(), gr.dev(), ng.dev() }, x.dev(), cnt.dev(), in_row_bytes, out_row_bytes, n_rows, s);
    });
}
int gfdm_hip_frame_check_verify_device(gfdm_hip_frame_check* c, void* payload, void* ok, void* good_row, void* n_good, const void* frames,
                                       const void* count, int64_t in_row_bytes, int64_t out_row_bytes, int64_t n_rows, void* stream)
{
    const VerifyOut o = { payload, ok, good_row, n_good };
    const int rc = check_verify(c, o, frames, in_row_bytes, out_row_bytes, n_rows);
    if (rc != GFDM_HIP_OK) return rc;
    return gfdm::on_device(c->ctx.device, stream, [&](hipStream_t s) { return enqueue_verify(c, o, frames, count, in_row_bytes, out_row_bytes, n_rows, s); });
}

}  // extern "C"
