// Internal, host only: what every translation unit of the C-ABI needs around a runtime call -- error reporting, the device guard, the device
// check, a handle's device + private stream, and the device memory of one convenience host call.  Never seen by hiprtc (not in JIT_HDRS).
#pragma once
#include "../../include/gfdm_hip.h"
#include "gfdm_plan.h"

#include <cfloat>
#include <cmath>
#include <string>

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
        DeviceGuard guard(device);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// bytes of one sample of a capture (SampleFormat): the host flavours upload it in the caller's format
inline size_t sample_bytes(int fmt) { return fmt == SAMPLES_SC16 ? 2 * sizeof(int16_t) : sizeof(cf); }

// Device memory that lives for one host call (upload, ONE enqueue, download, synchronise: a convenience, not a pipeline).  A buffer is
// handed out whole (as) or piece by piece (take; pieces in descending order of alignment, the caller sizes the buffer for their sum).
struct DevBuf {
    void* p = nullptr;
    size_t taken = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }          // a zero-length request still yields a pointer
    template <class T> T* as() const { return static_cast<T*>(p); }
    template <class T> T* take(size_t count)
    {
        T* piece = reinterpret_cast<T*>(static_cast<unsigned char*>(p) + taken);
        taken += count * sizeof(T);
        return piece;
    }
};

// host array -> device piece / device piece -> host array on the call's stream; an absent (NULL) host array or an empty one is skipped
inline hipError_t upload(void* dev, const void* host, size_t bytes, hipStream_t s)
{
    return (host && bytes) ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}
inline hipError_t download(void* host, const void* dev, size_t bytes, hipStream_t s)
{
    return (host && bytes) ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
}

}  // namespace gfdm
