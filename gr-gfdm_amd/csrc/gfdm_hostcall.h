// Internal, host only: what every translation unit of the C-ABI needs around a runtime call -- error reporting, the device guard, the device
// check, a handle's device + private stream, the skeletons of a constructor (create_handle) and of a *_device call (on_device), the staged
// *_host call (HostCall: one allocation, uploads, the enqueue, downloads, one synchronise), the checks and the call pair of the stream stages
// and the constellation the symbol mapper and the link meter share.  Compiled as plain C++ by tests/sanitize (hostcall_check.cc).  Never seen by hiprtc (not in JIT_HDRS).
#pragma once
#include "../../include/gfdm_hip.h"
#include "gfdm_plan.h"

#include <cfloat>
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

namespace gfdm {

// The decision rule a handle RUNS over `pts` (a gfdm_hip_decision, never AUTO) when the caller asked for `decision`, or -1 where the rule
// asked for does not fit n_points.  Shared by every constructor that takes a constellation.
// "Is this GNU Radio's unit constellation": every component within 6 * FLT_EPSILON * |component| (5.1e-7 at 1 / sqrt 2 = 8.5 f32 ulps there) of the unit
// point's.  Points that went through a double -> float conversion or a product with 1 / sqrt 2 in float land within one ulp; gr::digital's
// constellation_qpsk is built from the LITERAL SQRT_TWO = 0.707107 (gr-digital/lib/constellation.cc), which as a float sits 2.3e-7 = 3.8 ulps
// away from 1 / sqrt 2 and must still get the sign tests (tests/test_parity_gpu.py test_decision_rule_a_handle_runs_is_reported).
// The sign-test kernels of the receivers then cancel with 0.70710678f: 3.2e-7 relative to the literal's points, far inside the 1e-5 of the parity statement.
// AUTO picks the sign tests for those points alone.  An explicit QPSK / BPSK rule over other points (scaled, rotated) keeps its decision REGIONS
// only if it is the nearest-point rule of those points; it is then run as that, on the points as given.
inline int resolve_decision(const cf* pts, int n_points, int decision)
{
    auto near = [](cf p, float re, float im) {
        const float tr = 6.f * FLT_EPSILON * (std::fabs(re) > 0.f ? std::fabs(re) : 1.f), ti = 6.f * FLT_EPSILON * (std::fabs(im) > 0.f ? std::fabs(im) : 1.f);
        return std::fabs(p.x - re) <= tr && std::fabs(p.y - im) <= ti;
    };
    const float s = 0.70710678118654752f;
    const bool unit_qpsk = n_points == 4 && near(pts[0], -s, -s) && near(pts[1], s, -s) && near(pts[2], -s, s) && near(pts[3], s, s);
    const bool unit_bpsk = n_points == 2 && near(pts[0], -1.f, 0.f) && near(pts[1], 1.f, 0.f);
    if (decision == GFDM_HIP_DECIDE_AUTO) return unit_qpsk ? GFDM_HIP_DECIDE_QPSK : unit_bpsk ? GFDM_HIP_DECIDE_BPSK : GFDM_HIP_DECIDE_NEAREST;
    if ((decision == GFDM_HIP_DECIDE_QPSK && n_points != 4) || (decision == GFDM_HIP_DECIDE_BPSK && n_points != 2)) return -1;
    if (decision == GFDM_HIP_DECIDE_QPSK && !unit_qpsk) return GFDM_HIP_DECIDE_NEAREST;
    if (decision == GFDM_HIP_DECIDE_BPSK && !unit_bpsk) return GFDM_HIP_DECIDE_NEAREST;
    return decision;
}

// error reporting shared by the translation units of the C-ABI (thread-local message behind gfdm_hip_last_error; defined in gfdm_hip_api.hip)
int api_fail(int code, const std::string& msg);
int api_fail_hip(hipError_t e, const char* what);

#define GFDM_TRY(expr)                                                 \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return gfdm::api_fail_hip(_e, #expr);    \
    } while (0)

// RAII: make the handle's device current for the duration of a call.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        // hipGetLastError() is sticky: it keeps the error of ANY earlier failed runtime call of this thread (ours or the application's) until somebody reads
        // it, and the launchers check their launches with it -- a call must not fail on somebody else's stale error (found by tests/sanitize: an allocation
        // failure in one constructor failed the next handle's first launch).  Every entry point that launches builds a DeviceGuard first.
        (void)hipGetLastError();
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// is there a device, is the ordinal in range
inline int check_device(int dev)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return api_fail(GFDM_HIP_ENODEV, "no HIP device available (this library has no CPU path)");
    if (dev < 0 || dev >= count) return api_fail(GFDM_HIP_ENODEV, "HIP device ordinal out of range");
    return GFDM_HIP_OK;
}

// what a handle owns of the device: its ordinal and a private non-blocking stream for the *_host entry points
struct DeviceCtx {
    int device = 0;
    hipStream_t stream = nullptr;

    DeviceCtx() = default;
    DeviceCtx(const DeviceCtx&) = delete;
    DeviceCtx& operator=(const DeviceCtx&) = delete;
    int open(int dev)
    {
        const int rc = check_device(dev);
        if (rc != GFDM_HIP_OK) return rc;
        device = dev;
        DeviceGuard guard(dev);
        if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
        GFDM_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return GFDM_HIP_OK;
    }
    ~DeviceCtx()
    {
        if (!stream) return;         // never opened (a constructor that refused its arguments): no runtime call
        DeviceGuard guard(device);
        (void)hipStreamDestroy(stream);
    }
};

// bytes of one sample of a capture (SampleFormat): the host flavours upload it in the caller's format
inline size_t sample_bytes(int fmt) { return fmt == SAMPLES_SC16 ? 2 * sizeof(int16_t) : sizeof(cf); }

inline bool misaligned(const void* p, size_t to) { return ((uintptr_t)p % to) != 0; }

// a row width in elements of `elem` bytes: at least `least`, and n_rows rows of it inside int64
inline int check_width(int64_t width, int64_t least, int64_t elem, int64_t n_rows, const char* what)
{
    if (width < least) return api_fail(GFDM_HIP_EINVAL, std::string(what) + " is below the row's minimum");
    if (width > INT64_MAX / elem || (n_rows > 0 && width * elem > INT64_MAX / n_rows))
        return api_fail(GFDM_HIP_EINVAL, "the byte size of the rows overflows int64");
    return GFDM_HIP_OK;
}

// ---- the checks the stream stages share (channel model, fading model, resampler, burst shaper) ----
// n output samples with absolute indices offset .. offset + n - 1 from history + n complex64 input samples
inline int check_stream_span(int64_t n, int64_t history, int64_t offset)
{
    constexpr int64_t kMaxIndex = (int64_t)1 << 62;
    if (n < 0) return api_fail(GFDM_HIP_EINVAL, "n must be >= 0");
    if (history < 0) return api_fail(GFDM_HIP_EINVAL, "history must be >= 0");
    if (offset < 0) return api_fail(GFDM_HIP_EINVAL, "offset must be >= 0");
    if (n > kMaxIndex || offset > kMaxIndex - n) return api_fail(GFDM_HIP_EINVAL, "offset + n must not exceed 2^62");
    const int64_t lim = INT64_MAX / (int64_t)sizeof(cf);
    if (n > lim || history > lim - n) return api_fail(GFDM_HIP_EINVAL, "the byte size of the input overflows int64");
    return GFDM_HIP_OK;
}

// a stage that reads neighbours has no in-place call: n_out samples of out_bytes each at `out` against [in - history, in + n_in) of in_bytes
// each; `count` is the name of n_in in the caller's contract, `who` the module
inline int check_no_overlap(const void* out, size_t out_bytes, int64_t n_out, const void* in, size_t in_bytes, int64_t n_in, int64_t history,
                            const char* count, const char* who)
{
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n_out * out_bytes;
    const uintptr_t i0 = (uintptr_t)in - (uintptr_t)history * in_bytes, i1 = (uintptr_t)in + (uintptr_t)n_in * in_bytes;
    if (o0 < i1 && i0 < o1) return api_fail(GFDM_HIP_EINVAL, std::string("out overlaps [in - history, in + ") + count + "): " + who + " has no in-place call");
    return GFDM_HIP_OK;
}

inline int check_sample_alignment(const void* out, size_t out_bytes, const void* in, size_t in_bytes)
{
    if (misaligned(out, out_bytes) || misaligned(in, in_bytes)) return api_fail(GFDM_HIP_EINVAL, "a buffer lacks the alignment of one sample");
    return GFDM_HIP_OK;
}

// The *_device flavour of an entry point, after its checks: make the handle's device current, refuse if that failed, enqueue on the caller's stream.
template <class F>
int on_device(int device, void* stream, F enqueue)
{
    DeviceGuard guard(device);
    if (!guard.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
    return enqueue((hipStream_t)stream);
}

// The skeleton of a constructor.  `init` checks the arguments and fills the handle's host fields; `on_dev` runs with the device current and
// the context open, for what the handle keeps on the device.  Any failure deletes the handle.  A call that `init` refuses makes no runtime
// call at all, as when the checks ran before the handle existed: the destructor of a handle (and of its DeviceCtx) builds its DeviceGuard
// only when there is a stream or device memory to release (tests/sanitize/hostcall_check.cc counts the calls).
template <class H, class Init, class OnDev>
int create_handle(H** out, int device, Init init, OnDev on_dev)
{
    if (!out) return api_fail(GFDM_HIP_EINVAL, "NULL handle pointer");
    *out = nullptr;
    H* h = new (std::nothrow) H();
    if (!h) return api_fail(GFDM_HIP_ENOMEM, "out of host memory");
    int rc = init(*h);
    if (rc == GFDM_HIP_OK) rc = h->ctx.open(device);
    if (rc == GFDM_HIP_OK) {
        DeviceGuard guard(device);
        rc = on_dev(*h);
    }
    if (rc != GFDM_HIP_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return GFDM_HIP_OK;
}
template <class H, class Init>
int create_handle(H** out, int device, Init init)
{
    return create_handle(out, device, init, [](H&) { return GFDM_HIP_OK; });
}

// One convenience *_host call (a convenience, not a pipeline): everything around the enqueue of the *_device flavour.  The caller declares
// its operands -- in: a host array that goes up, out: one that comes back, scratch: device only -- and run() does the rest on the handle's
// private stream: ONE device allocation for all pieces, the uploads, the callable, the downloads, ONE synchronise; the allocation is freed
// with the object.  The pieces lie in the order of declaration, each at least 16 bytes long and on a 256-byte boundary, and the allocation
// ends with the last piece.  256 is what hipMalloc guarantees, so every piece keeps the alignment it had as an allocation of its own: the
// kernels take the same aligned / unaligned (`mis`) paths, and memsets and copies see the same addresses modulo 256, as before.  An operand whose
// host pointer is NULL takes no room, is not copied and is NULL to the enqueue; an empty one with a host pointer has a valid device address.
// A failing runtime call or a non-OK status of the callable ends the call with that status (no synchronise after a failed enqueue).
class HostCall {
public:
    template <class T>
    class Piece {
    public:
        T* dev() const { return present_ ? reinterpret_cast<T*>(hc_->base_ + off_) : nullptr; }      // valid inside run()'s callable

    private:
        friend class HostCall;
        const HostCall* hc_;
        size_t off_;
        bool present_;
    };

    HostCall(int device, hipStream_t stream) : guard_(device), stream_(stream) {}
    explicit HostCall(const DeviceCtx& ctx) : HostCall(ctx.device, ctx.stream) {}
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    ~HostCall() { if (base_) (void)hipFree(base_); }

    template <class T> Piece<const T> in(const T* host, size_t count)
    {
        const Piece<const T> p = place<const T>(host != nullptr, count * sizeof(T));
        if (host && count) up_.push_back(Copy{ p.off_, const_cast<T*>(host), count * sizeof(T) });
        return p;
    }
    template <class T> Piece<T> out(T* host, size_t count)
    {
        const Piece<T> p = place<T>(host != nullptr, count * sizeof(T));
        if (host && count) down_.push_back(Copy{ p.off_, host, count * sizeof(T) });
        return p;
    }
    template <class T> Piece<T> scratch(size_t count) { return place<T>(true, count * sizeof(T)); }

    template <class F>
    int run(F enqueue)
    {
        if (!guard_.ok) return api_fail(GFDM_HIP_ENODEV, "hipSetDevice failed");
        if (size_) GFDM_TRY(hipMalloc(&base_, size_));
        for (const Copy& c : up_) GFDM_TRY(hipMemcpyAsync(base_ + c.off, c.host, c.bytes, hipMemcpyHostToDevice, stream_));
        const int rc = enqueue(stream_);
        if (rc != GFDM_HIP_OK) return rc;
        for (const Copy& c : down_) GFDM_TRY(hipMemcpyAsync(c.host, base_ + c.off, c.bytes, hipMemcpyDeviceToHost, stream_));
        GFDM_TRY(hipStreamSynchronize(stream_));
        return GFDM_HIP_OK;
    }

private:
    struct Copy { size_t off; void* host; size_t bytes; };
    static constexpr size_t kAlign = 256;      // hipMalloc's own guarantee: a piece is aligned as it was when it had an allocation to itself

    template <class T> Piece<T> place(bool present, size_t bytes)
    {
        Piece<T> p;
        p.hc_ = this;
        p.off_ = (size_ + kAlign - 1) / kAlign * kAlign;
        p.present_ = present;
        if (present) size_ = p.off_ + (bytes > 16 ? bytes : 16);
        return p;
    }

    DeviceGuard guard_;              // first: the device stays current until the allocation is freed
    hipStream_t stream_;
    unsigned char* base_ = nullptr;
    size_t size_ = 0;
    std::vector<Copy> up_, down_;
};

// Both flavours of a stream stage's call that maps history + n complex64 samples to n samples, complex64 or sc16 (channel model, fading
// model): `check` is the module's check_call, `enqueue` its one launch.  host: upload history + n samples, the enqueue on the handle's
// stream, download n; else the enqueue on the caller's stream.
template <class H, class Check, class Enqueue>
int stream_call(H* h, bool host, int sc16, void* out, const void* in, int64_t n, int64_t history, int64_t offset, double gain, void* stream, Check check, Enqueue enqueue)
{
    const int rc = check(h, out, in, sc16, n, history, offset, gain);
    if (rc != GFDM_HIP_OK || n == 0) return rc;
    if (!host) return on_device(h->ctx.device, stream, [&](hipStream_t s) { return enqueue(h, sc16, out, static_cast<const cf*>(in), n, history, offset, gain, s); });
    HostCall hc(h->ctx);
    const auto x = hc.in(static_cast<const cf*>(in) - history, (size_t)(history + n));
    const auto y = hc.out(static_cast<unsigned char*>(out), (size_t)n * (sc16 ? 2 * sizeof(int16_t) : sizeof(cf)));
    return hc.run([&](hipStream_t s) { return enqueue(h, sc16, y.dev(), x.dev() + history, n, history, offset, gain, s); });
}

// ---- the constellation of a handle: the symbol mapper and the link meter decide with the same points and the same rule ----
inline int bits_of(int n_points)
{
    for (int k = 1; k <= 8; ++k)
        if (n_points == (1 << k)) return k;
    return 0;
}

inline int64_t row_bytes_of(int k, int64_t n_sym) { return (n_sym * k + 7) / 8; }

struct Constellation {
    int k = 0, rule = GFDM_HIP_DECIDE_NEAREST;
    cf points[256];
    cf* d_points = nullptr;          // freed by the owning handle's destructor, under the guard it builds for its own device memory

    Constellation() = default;
    Constellation(const Constellation&) = delete;
    Constellation& operator=(const Constellation&) = delete;
    // the argument checks and the host copy: no device yet
    int set(const float* pts, int n_points, int decision)
    {
        const int rc = gfdm_hip_symbol_mapper_check(n_points, 1, 0);
        if (rc != GFDM_HIP_OK) return rc;
        if (!pts) return api_fail(GFDM_HIP_EINVAL, "NULL constellation points");
        if (decision < GFDM_HIP_DECIDE_AUTO || decision > GFDM_HIP_DECIDE_BPSK) return api_fail(GFDM_HIP_EINVAL, "bad decision rule");
        rule = resolve_decision(reinterpret_cast<const cf*>(pts), n_points, decision);
        if (rule < 0) return api_fail(GFDM_HIP_EINVAL, "decision rule does not match the number of constellation points");
        k = bits_of(n_points);
        std::copy(reinterpret_cast<const cf*>(pts), reinterpret_cast<const cf*>(pts) + n_points, points);
        return GFDM_HIP_OK;
    }
    // the points on the handle's device (which is current)
    int upload()
    {
        const size_t bytes = ((size_t)1 << k) * sizeof(cf);
        hipError_t e = hipMalloc(&d_points, bytes);
        if (e == hipSuccess) e = hipMemcpy(d_points, points, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? GFDM_HIP_OK : api_fail_hip(e, "constellation upload");
    }
};

// f(std::integral_constant<int, K>) for the run-time k = 1 .. 8
template <class F>
void dispatch_bits(int k, F f)
{
    switch (k) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 8>()); break;
    }
}

// f(K, RULE) as integral constants for the rule a handle runs: the sign tests exist for the unit QPSK and BPSK points alone
template <int K, class F>
void with_rule(int rule, F f)
{
    if (K == 2 && rule == GFDM_HIP_DECIDE_QPSK) f(std::integral_constant<int, 2>(), std::integral_constant<int, GFDM_HIP_DECIDE_QPSK>());
    else if (K == 1 && rule == GFDM_HIP_DECIDE_BPSK) f(std::integral_constant<int, 1>(), std::integral_constant<int, GFDM_HIP_DECIDE_BPSK>());
    else f(std::integral_constant<int, K>(), std::integral_constant<int, GFDM_HIP_DECIDE_NEAREST>());
}

}  // namespace gfdm
