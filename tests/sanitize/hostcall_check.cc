// TEST-ONLY driver for the staged host call of gr-gfdm_amd/csrc/gfdm_hostcall.h (gfdm::HostCall) against the loop-back HIP layer, under
// AddressSanitizer + UBSan: no GPU, no Python.  The "kernel" is a host function enqueued on the call's stream (loopback::enqueue); device memory
// is malloc'ed memory of exactly the requested size, so a piece placed or sized wrong is an AddressSanitizer report.
//   round trip: every `in` piece holds the host bytes when the callable runs, every `out` array holds what the callable wrote, copied once; absent
//               operands are NULL inside the callable; empty ones have an address
//   extents:    every piece is on a 256-byte boundary (as an allocation of its own was), at least 16 bytes long and disjoint from the others; out and scratch pieces are written to their full
//               size with a pattern of their own, the in pieces are read again afterwards
//   failure:    every runtime call HostCall makes fails once, and so does the callable: a non-OK status, nothing left allocated, the next call succeeds
// ... and for the constructor skeleton (gfdm::create_handle) with a handle built like the symbol mapper's (DeviceCtx + Constellation):
//   refused:    a call whose arguments are refused makes NO runtime call, neither before the refusal nor when the handle it had built is deleted
//               (the layer counts every hip* call), so it does not initialise the runtime, select a device or swallow the caller's sticky error
//   failure:    the stream, the allocation and the upload failing once each: a non-OK status, no handle, nothing left allocated or open
#include <hip/hip_runtime.h>

#include "gfdm_hostcall.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
std::string g_last_error;
int g_failed = 0;
}
int gfdm::api_fail(int code, const std::string& msg) { g_last_error = msg; return code; }
int gfdm::api_fail_hip(hipError_t e, const char* what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return GFDM_HIP_EHIP;
}

#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                   \
            fprintf(stderr, "\n");                                          \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

namespace {

// a host array of exactly `bytes` bytes (so that AddressSanitizer sees a copy that runs past it), filled with a pattern of its own
struct HostArray {
    unsigned char* p;
    size_t bytes;
    HostArray(size_t n, unsigned seed) : p(static_cast<unsigned char*>(malloc(n ? n : 1))), bytes(n) { fill(p, n, seed); }
    HostArray(const HostArray&) = delete;
    ~HostArray() { free(p); }
    static unsigned char at(size_t i, unsigned seed) { return (unsigned char)(seed * 37u + i * 11u + (i >> 8)); }
    static void fill(unsigned char* q, size_t n, unsigned seed) { for (size_t i = 0; i < n; ++i) q[i] = at(i, seed); }
    static bool holds(const unsigned char* q, size_t n, unsigned seed)
    {
        for (size_t i = 0; i < n; ++i)
            if (q[i] != at(i, seed)) return false;
        return true;
    }
};

struct Range { const unsigned char* p; size_t bytes; };

// what the callable found wrong (it runs on the stream's thread)
std::atomic<int> g_kernel_errors{ 0 };
#define KCHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED in the callable, line %d: %s\n", __LINE__, #cond); g_kernel_errors.fetch_add(1); } } while (0)

enum Fault { NONE, SET_DEVICE, MALLOC, UPLOAD, DOWNLOAD, SYNCHRONIZE, LAUNCH, CALLABLE, N_FAULTS };
const char* const kFaultName[] = { "none", "hipSetDevice", "hipMalloc", "hipMemcpyAsync (up)", "hipMemcpyAsync (down)", "hipStreamSynchronize", "launch", "callable" };

constexpr size_t kSmall[] = { 1, 7, 8, 20 };      // not multiples of 16
constexpr size_t kBigIn = 100003, kBigOut = 70001 * sizeof(float), kBigScratch = 4099, kHistory = 5, kSpanFirst = 3;
constexpr int kUploads = 7, kDownloads = 5;        // the non-empty present operands below

// one staged call with every kind of operand; returns its status
int staged_call(const gfdm::DeviceCtx& ctx, Fault fault)
{
    // host side: inputs keep their pattern, outputs start with another one and must come back with the callable's
    HostArray in_small[4] = { { kSmall[0], 1 }, { kSmall[1], 2 }, { kSmall[2], 3 }, { kSmall[3], 4 } };
    HostArray in_big(kBigIn, 5), in_hist(kHistory * 8 + 64, 6), in_span(kSpanFirst + 33, 7), in_empty(0, 8);
    HostArray out_small[4] = { { kSmall[0], 101 }, { kSmall[1], 102 }, { kSmall[2], 103 }, { kSmall[3], 104 } };
    HostArray out_big(kBigOut, 105), out_empty(0, 106);
    const loopback::Stats before = loopback::stats();
    int rc;
    loopback::clear_failures();
    if (fault == SET_DEVICE) loopback::fail_next("hipSetDevice", 0, 1, hipErrorInvalidDevice);
    if (fault == MALLOC) loopback::fail_next("hipMalloc", 0, 1, hipErrorOutOfMemory);
    if (fault == UPLOAD) loopback::fail_next("hipMemcpyAsync", kUploads - 1, 1, hipErrorUnknown);
    if (fault == DOWNLOAD) loopback::fail_next("hipMemcpyAsync", kUploads + 1, 1, hipErrorUnknown);
    if (fault == SYNCHRONIZE) loopback::fail_next("hipStreamSynchronize", 0, 1, hipErrorUnknown);
    if (fault == LAUNCH) loopback::fail_next("launch", 0, 1, hipErrorLaunchFailure);
    loopback::arm(true);
    {
        gfdm::HostCall hc(ctx);
        const auto a0 = hc.in(in_small[0].p, kSmall[0]);
        const auto a1 = hc.in(in_small[1].p, kSmall[1]);
        const auto a2 = hc.in(reinterpret_cast<const int64_t*>(in_small[2].p), 1);
        const auto a3 = hc.in(reinterpret_cast<const float*>(in_small[3].p), 5);
        const auto big = hc.in(in_big.p, kBigIn);
        const auto absent_in = hc.in(static_cast<const float*>(nullptr), 9);
        const auto hist = hc.in(reinterpret_cast<const float2*>(in_hist.p + 64) - kHistory, kHistory + 0);      // [in - history, in + 0): the channel model's operand
        const auto span = hc.in(in_span.p + kSpanFirst, 33);                                                     // a sub-span: the synchroniser's
        const auto empty_in = hc.in(in_empty.p, 0);
        const auto o0 = hc.out(out_small[0].p, kSmall[0]);
        const auto absent_out = hc.out(static_cast<int32_t*>(nullptr), 9);
        const auto o1 = hc.out(out_small[1].p, kSmall[1]);
        const auto s0 = hc.scratch<unsigned char>(1);
        const auto o2 = hc.out(reinterpret_cast<int64_t*>(out_small[2].p), 1);
        const auto o3 = hc.out(reinterpret_cast<float*>(out_small[3].p), 5);
        const auto s1 = hc.scratch<unsigned char>(kBigScratch);
        const auto obig = hc.out(reinterpret_cast<float*>(out_big.p), kBigOut / sizeof(float));
        const auto empty_out = hc.out(out_empty.p, 0);
        const auto s_empty = hc.scratch<uint64_t>(0);
        const auto s_last = hc.scratch<unsigned char>(32);      // the last piece ends where the allocation ends: one written to its last byte
        rc = hc.run([&](hipStream_t s) -> int {
            if (fault == CALLABLE) return gfdm::api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one element");
            // everything the "kernel" needs, by value: it runs later, on the stream's thread
            const Range ins[] = { { a0.dev(), kSmall[0] }, { a1.dev(), kSmall[1] }, { (const unsigned char*)a2.dev(), kSmall[2] }, { (const unsigned char*)a3.dev(), kSmall[3] },
                                  { big.dev(), kBigIn }, { (const unsigned char*)hist.dev(), kHistory * 8 }, { span.dev(), 33 }, { empty_in.dev(), 0 } };
            const unsigned char* in_host[] = { in_small[0].p, in_small[1].p, in_small[2].p, in_small[3].p, in_big.p, in_hist.p + 64 - kHistory * 8, in_span.p + kSpanFirst, in_empty.p };
            const Range outs[] = { { o0.dev(), kSmall[0] }, { o1.dev(), kSmall[1] }, { (unsigned char*)o2.dev(), kSmall[2] }, { (unsigned char*)o3.dev(), kSmall[3] },
                                   { (unsigned char*)obig.dev(), kBigOut }, { empty_out.dev(), 0 }, { s0.dev(), 1 }, { s1.dev(), kBigScratch }, { (unsigned char*)s_empty.dev(), 0 }, { s_last.dev(), 32 } };
            const void* absent[] = { absent_in.dev(), absent_out.dev() };
            std::vector<Range> vi(ins, ins + 8), vo(outs, outs + 10);
            std::vector<const unsigned char*> vh(in_host, in_host + 8);
            const bool absent_null = !absent[0] && !absent[1];
            const hipError_t e = loopback::enqueue(s, [vi, vo, vh, absent_null] {
                KCHECK(absent_null);
                std::vector<Range> all(vi);
                all.insert(all.end(), vo.begin(), vo.end());
                for (size_t i = 0; i < all.size(); ++i) {
                    KCHECK(all[i].p != nullptr);
                    KCHECK((uintptr_t)all[i].p % 256 == 0);          // as an allocation of its own was
                    for (size_t j = 0; j < i; ++j) {              // extents of at least 16 bytes, no two overlap
                        const size_t ei = all[i].bytes > 16 ? all[i].bytes : 16, ej = all[j].bytes > 16 ? all[j].bytes : 16;
                        KCHECK(all[i].p + ei <= all[j].p || all[j].p + ej <= all[i].p);
                    }
                }
                for (size_t i = 0; i < vi.size(); ++i) KCHECK(memcmp(vi[i].p, vh[i], vi[i].bytes) == 0);
                for (size_t i = 0; i < vo.size(); ++i) HostArray::fill(const_cast<unsigned char*>(vo[i].p), vo[i].bytes, 200 + (unsigned)i);
                for (size_t i = 0; i < vi.size(); ++i) KCHECK(memcmp(vi[i].p, vh[i], vi[i].bytes) == 0);      // ... and nothing of that landed in an input
                for (size_t i = 0; i < vo.size(); ++i) KCHECK(HostArray::holds(vo[i].p, vo[i].bytes, 200 + (unsigned)i));
            });
            return e == hipSuccess ? (int)GFDM_HIP_OK : gfdm::api_fail_hip(e, "launch");
        });
    }
    loopback::arm(false);
    loopback::clear_failures();
    const loopback::Stats after = loopback::stats();
    CHECK(loopback::live_allocations() == 0, "%ld allocations live after a call (%s)", loopback::live_allocations(), kFaultName[fault]);
    CHECK(after.dev_allocs - before.dev_allocs == (fault == SET_DEVICE || fault == MALLOC ? 0 : 1), "%ld device allocations in one call (%s)",
          after.dev_allocs - before.dev_allocs, kFaultName[fault]);
    // the inputs are the caller's: never written
    for (int i = 0; i < 4; ++i) CHECK(HostArray::holds(in_small[i].p, kSmall[i], 1 + (unsigned)i), "input %d was written", i);
    CHECK(HostArray::holds(in_big.p, kBigIn, 5) && HostArray::holds(in_hist.p, in_hist.bytes, 6) && HostArray::holds(in_span.p, in_span.bytes, 7), "an input was written");
    if (rc == GFDM_HIP_OK) {
        CHECK(fault == NONE, "the call succeeded although %s failed", kFaultName[fault]);
        CHECK(after.async_copies - before.async_copies == kUploads + kDownloads, "%ld copies, expected %d: an operand was copied twice or not at all",
              after.async_copies - before.async_copies, kUploads + kDownloads);
        CHECK(after.launches - before.launches == 1, "%ld launches", after.launches - before.launches);
        for (int i = 0; i < 4; ++i) CHECK(HostArray::holds(out_small[i].p, kSmall[i], 200 + (unsigned)i), "output %d (%zu bytes) does not hold what the callable wrote", i, kSmall[i]);
        CHECK(HostArray::holds(out_big.p, kBigOut, 204), "the large output does not hold what the callable wrote");
    } else {
        CHECK(fault != NONE, "status %d: %s", rc, g_last_error.c_str());
        if (fault == SET_DEVICE) CHECK(rc == GFDM_HIP_ENODEV && g_last_error == "hipSetDevice failed", "status %d: %s", rc, g_last_error.c_str());
        if (fault == CALLABLE) CHECK(rc == GFDM_HIP_EINVAL && g_last_error == "a buffer lacks the alignment of one element", "status %d: %s", rc, g_last_error.c_str());
        if (fault == CALLABLE || fault == LAUNCH || fault == UPLOAD || fault == MALLOC || fault == SET_DEVICE)      // nothing came back
            for (int i = 0; i < 4; ++i) CHECK(HostArray::holds(out_small[i].p, kSmall[i], 101 + (unsigned)i), "output %d was written by a call that failed before its enqueue", i);
    }
    return rc;
}

// a handle as the device modules build theirs (gfdm_symbols.hip): the destructor builds a guard only when there is device memory to free
struct TestHandle {
    gfdm::DeviceCtx ctx;
    gfdm::Constellation c;
    ~TestHandle()
    {
        if (!c.d_points) return;
        gfdm::DeviceGuard guard(ctx.device);
        (void)hipFree(c.d_points);
    }
};

int create(TestHandle** out, const float* points, int n_points, int decision)
{
    return gfdm::create_handle(
        out, 0, [&](TestHandle& h) { return h.c.set(points, n_points, decision); }, [](TestHandle& h) { return h.c.upload(); });
}

void constructor_checks()
{
    const float qpsk[8] = { -1, -1, 1, -1, -1, 1, 1, 1 };
    TestHandle* const stale = reinterpret_cast<TestHandle*>(sizeof(TestHandle));      // never dereferenced: a refused call must reset *out
    struct { const float* pts; int n, decision; const char* what; } refused[] = {
        { qpsk, 3, GFDM_HIP_DECIDE_AUTO, "3 points" }, { nullptr, 4, GFDM_HIP_DECIDE_AUTO, "NULL points" }, { qpsk, 4, 17, "bad decision" },
        { qpsk, 4, GFDM_HIP_DECIDE_BPSK, "BPSK rule over 4 points" } };
    (void)hipSetDevice(1);                                   // the caller's state: another device current, a sticky error pending
    (void)hipSetDevice(99);
    for (const auto& r : refused) {
        TestHandle* h = stale;
        const long before = loopback::runtime_calls();
        const int rc = create(&h, r.pts, r.n, r.decision);
        CHECK(rc == GFDM_HIP_EINVAL && h == nullptr, "%s: status %d", r.what, rc);
        CHECK(loopback::runtime_calls() == before, "%s: a refused constructor made %ld runtime calls", r.what, loopback::runtime_calls() - before);
    }
    const long before = loopback::runtime_calls();
    CHECK(create(nullptr, qpsk, 4, GFDM_HIP_DECIDE_AUTO) == GFDM_HIP_EINVAL && loopback::runtime_calls() == before, "NULL handle pointer");
    int dev = -1;
    CHECK(hipGetDevice(&dev) == hipSuccess && dev == 1, "the current device changed to %d", dev);
    CHECK(hipGetLastError() == hipErrorInvalidDevice, "the caller's pending error was swallowed");
    (void)hipSetDevice(0);

    // every runtime call of an accepted constructor failing once, then the call that succeeds
    const char* const apis[] = { "hipGetDeviceCount", "hipSetDevice", "hipStreamCreateWithFlags", "hipMalloc", "hipMemcpy" };
    for (const char* api : apis) {
        const loopback::Stats s0 = loopback::stats();
        TestHandle* h = stale;
        loopback::fail_next(api, 0, 1, hipErrorUnknown);
        loopback::arm(true);
        const int rc = create(&h, qpsk, 4, GFDM_HIP_DECIDE_AUTO);
        loopback::arm(false);
        loopback::clear_failures();
        const loopback::Stats s1 = loopback::stats();
        CHECK(rc != GFDM_HIP_OK && h == nullptr, "%s failed and the constructor returned %d", api, rc);
        CHECK(loopback::live_allocations() == 0 && s1.streams_created - s0.streams_created == s1.streams_destroyed - s0.streams_destroyed,
              "%s failed: %ld allocations live, %ld streams open", api, loopback::live_allocations(),
              (s1.streams_created - s0.streams_created) - (s1.streams_destroyed - s0.streams_destroyed));
    }
    const loopback::Stats s0 = loopback::stats();
    TestHandle* h = nullptr;
    CHECK(create(&h, qpsk, 4, GFDM_HIP_DECIDE_AUTO) == GFDM_HIP_OK && h != nullptr, "constructor: %s", g_last_error.c_str());
    if (h) {
        CHECK(h->c.k == 2 && h->c.rule == GFDM_HIP_DECIDE_NEAREST && h->ctx.stream && h->c.d_points && memcmp(h->c.d_points, qpsk, sizeof qpsk) == 0,
              "the handle's constellation");
        delete h;
    }
    const loopback::Stats s1 = loopback::stats();
    CHECK(loopback::live_allocations() == 0 && s1.streams_created - s0.streams_created == 1 && s1.streams_destroyed - s0.streams_destroyed == 1,
          "a destroyed handle left something behind");
}

}  // namespace

// the argument table of the constellation (defined beside the kernels in gfdm_symbols.hip, which this program cannot compile)
extern "C" int gfdm_hip_symbol_mapper_check(int n_points, int64_t, int64_t)
{
    return gfdm::bits_of(n_points) ? (int)GFDM_HIP_OK : gfdm::api_fail(GFDM_HIP_EINVAL, "a constellation needs 2, 4, 8, ..., 256 points");
}

int main()
{
    {
        gfdm::DeviceCtx ctx;
        CHECK(ctx.open(0) == GFDM_HIP_OK, "DeviceCtx::open: %s", g_last_error.c_str());
        CHECK(staged_call(ctx, NONE) == GFDM_HIP_OK, "round trip: %s", g_last_error.c_str());
        for (int f = SET_DEVICE; f < N_FAULTS; ++f) {
            CHECK(staged_call(ctx, (Fault)f) != GFDM_HIP_OK, "%s failed and the call did not", kFaultName[f]);
            CHECK(staged_call(ctx, NONE) == GFDM_HIP_OK, "the call after a failed %s: %s", kFaultName[f], g_last_error.c_str());
        }
        CHECK(hipStreamSynchronize(ctx.stream) == hipSuccess, "final synchronise");
    }
    constructor_checks();
    CHECK(g_kernel_errors.load() == 0, "%d checks failed inside the callable", g_kernel_errors.load());
    CHECK(loopback::live_allocations() == 0, "%ld loop-back allocations still live", loopback::live_allocations());
    if (g_failed) {
        fprintf(stderr, "hostcall check: %d FAILED\n", g_failed);
        return 1;
    }
    printf("hostcall check OK: round trip, extents, %d injected failures, constructors\n", N_FAULTS - 1);
    return 0;
}
