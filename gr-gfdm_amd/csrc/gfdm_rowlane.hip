// Row-lane kernel family: dispatch over the shapes compiled into the library (gfdm_row_shapes.h).  The kernels live in
// gfdm_rowlane_impl.h; gfdm_rowlane_shape.hip instantiates the kernels of one part of one shape (the library is linked with
// --no-undefined, so a shape the Makefile did not build fails the link).  Which kernel a call runs and its launch geometry:
// gfdm_rowvariants.h, shared with the run-time instantiation (gfdm_jit.hip).
#include "gfdm_rowvariants.h"
#include "gfdm_row_shapes.h"

#include <array>

namespace gfdm {

typedef const void* const* KernelList;        // the kernels of one part of a shape, in rowvar::part_variants order
#define GFDM_ROWLANE_PART(K_, M_, L_, P_) rowlane_##K_##_##M_##_##L_##_p##P_
#define X(K_, M_, L_)                                                                                                                  \
    extern const KernelList GFDM_ROWLANE_PART(K_, M_, L_, 0), GFDM_ROWLANE_PART(K_, M_, L_, 1), GFDM_ROWLANE_PART(K_, M_, L_, 2),       \
        GFDM_ROWLANE_PART(K_, M_, L_, 3), GFDM_ROWLANE_PART(K_, M_, L_, 4), GFDM_ROWLANE_PART(K_, M_, L_, 5);
GFDM_ROW_SHAPES(X)
#undef X

namespace {

// L < 0: the first shape with this (K, M) (the estimator does not depend on the overlap); nullptr: not compiled
KernelList compiled_part(int K, int M, int L, int part)
{
#define X(K_, M_, L_)                                                                                                                  \
    if (K == K_ && M == M_ && (L < 0 || L == L_))                                                                                      \
        return std::array<KernelList, JIT_NUM_PARTS>{ GFDM_ROWLANE_PART(K_, M_, L_, 0), GFDM_ROWLANE_PART(K_, M_, L_, 1),              \
                                                      GFDM_ROWLANE_PART(K_, M_, L_, 2), GFDM_ROWLANE_PART(K_, M_, L_, 3),              \
                                                      GFDM_ROWLANE_PART(K_, M_, L_, 4), GFDM_ROWLANE_PART(K_, M_, L_, 5) }[part];
    GFDM_ROW_SHAPES(X)
#undef X
    return nullptr;
}

hipError_t launch(KernelList kernels, const rowvar::Choice& c, int K, int M, int64_t nblocks, hipStream_t s, void** args)
{
    if (!kernels || c.index < 0) return hipErrorInvalidValue;
    const void* f = kernels[c.index];
    const rowvar::Geometry g = rowvar::geometry(K, M, c.v, nblocks);
    const hipError_t e = rowvar::allow_lds(f, g.lds);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(f, dim3(g.grid), dim3(g.block), args, g.lds, s);
}

}  // namespace

bool rowlane_supports(int M, int K, int L) { return compiled_part(K, M, L, JIT_PART_RX) != nullptr; }

bool rowlane_supports_estimate(int M, int K) { return compiled_part(K, M, -1, JIT_PART_EST) != nullptr; }

hipError_t launch_rowlane_estimate(const EstPlan& e, cf* out, const cf* in, int64_t nframes, hipStream_t s)
{
    if (nframes <= 0) return hipSuccess;
    EstPlan a_e = e;
    void* args[] = { &a_e, &out, &in, &nframes };
    return launch(compiled_part(e.K, e.M, -1, JIT_PART_EST), rowvar::select_estimate(e), e.K, e.M, nframes, s, args);
}

hipError_t launch_rowlane_modulate(const DevicePlan& p, const TxParams& tx, const cf* twT, cf* out, const cf* in, int64_t nblocks,
                                   hipStream_t s)
{
    if (nblocks <= 0) return hipSuccess;
    DevicePlan a_p = p;
    TxParams a_tx = tx;
    a_p.taps_real = rowvar::plan_flags_modulate(p, tx, out, in);
    a_p.wK = rowvar::plan_roots(p, twT);
    void* args[] = { &a_p, &a_tx, &twT, &out, &in, &nblocks };
    return launch(compiled_part(p.K, p.M, p.L, JIT_PART_MOD), rowvar::select_modulate(p, tx), p.K, p.M, nblocks, s, args);
}

hipError_t launch_rowlane_receive(const DevicePlan& p, const IcParams& ic, const EstPlan* est, const cf* twT, int mode, cf* out, const cf* in,
                                  const cf* f_eq, int64_t nblocks, hipStream_t s)
{
    if (nblocks <= 0) return hipSuccess;
    const rowvar::Choice c = rowvar::select_receive(p, ic, est, mode, f_eq);
    static const EstPlan kNoEst = {};
    DevicePlan a_p = p;
    IcParams a_ic = ic;
    a_p.taps_real = rowvar::plan_flags_receive(p, ic, est, out, in, f_eq);
    a_p.wK = rowvar::plan_roots(p, twT);
    EstPlan a_est = est ? *est : kNoEst;
    BurstIo a_bio = burst_io(est) ? *burst_io(est) : BurstIo{};
    void* args8[] = { &a_p, &a_ic, &a_est, &twT, &out, &in, &f_eq, &nblocks };
    void* args9[] = { &a_p, &a_ic, &a_est, &twT, &out, &in, &f_eq, &nblocks, &a_bio };      // k_row_receive_burst: BurstIo is its last argument
    void** args = burst_io(est) ? args9 : args8;
    return launch(compiled_part(p.K, p.M, p.L, c.v.part), c, p.K, p.M, nblocks, s, args);
}

}  // namespace gfdm
