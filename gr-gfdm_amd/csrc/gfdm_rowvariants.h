// Row-lane kernel variants: which kernels each part of a shape holds, which one a call runs, and its launch geometry.  ONE definition
// for the shapes compiled into the library (gfdm_rowlane_shape.hip, gfdm_rowlane.hip) and those instantiated at run time (gfdm_jit.hip);
// the two routes differ only in how a variant becomes a function and in the launch call.  Host side only.
#pragma once
#include "gfdm_plan.h"
#include "gfdm_tx.h"
#include "gfdm_rowgeom.h"

#include <atomic>
#include <cstdint>
#include <cstdlib>

namespace gfdm {
namespace rowvar {

// One kernel of a part (JIT_PART_*, gfdm_plan.h):
//   JIT_PART_RX, JIT_PART_RX_IC, JIT_PART_RX_PREAMBLE   k_row_receive<K, M, L, mode, eq, ick>
//   JIT_PART_RX_BURST                                   k_row_receive_burst<K, M, L, mode, ick>
//   JIT_PART_MOD                                        k_row_modulate<K, M, L, tx>
//   JIT_PART_EST                                        k_row_estimate<K, M>
struct Variant { int part, mode, eq, ick, tx; };

constexpr int kMaxVariants = 6;
struct PartVariants {
    int part = 0, n = 0;
    Variant v[kMaxVariants] = {};
    constexpr void add(int mode, int eq, int ick, int tx = 0) { v[n++] = Variant{ part, mode, eq, ick, tx }; }
};

// The kernels of a part in the order the launches index them.  The run-time route lists them in this order in its code-object cache
// (the .names files), so the order of the existing entries stays.  The matrix-core rounds exist only where rowgeom::ic_mfma(K, M).
constexpr PartVariants part_variants(int K, int M, int part)
{
    PartVariants t{ part };
    const bool mx = rowgeom::ic_mfma(K, M);
    switch (part) {
    case JIT_PART_RX:              // frequency-domain output and plain demodulation, equaliser none / vector
        t.add(RX_FD, EQ_NONE, ICK_GENERAL); t.add(RX_FD, EQ_VECTOR, ICK_GENERAL);
        t.add(RX_DEMOD, EQ_NONE, ICK_GENERAL); t.add(RX_DEMOD, EQ_VECTOR, ICK_GENERAL);
        break;
    case JIT_PART_RX_IC:           // interference cancellation, equaliser none / vector
        t.add(RX_IC, EQ_NONE, ICK_GENERAL); t.add(RX_IC, EQ_NONE, ICK_REALSYM);
        t.add(RX_IC, EQ_VECTOR, ICK_GENERAL); t.add(RX_IC, EQ_VECTOR, ICK_REALSYM);
        if (mx) { t.add(RX_IC, EQ_NONE, ICK_MFMA); t.add(RX_IC, EQ_VECTOR, ICK_MFMA); }
        break;
    case JIT_PART_RX_PREAMBLE:     // every mode with the equaliser estimated from the preamble inside the kernel
        t.add(RX_FD, EQ_PREAMBLE, ICK_GENERAL); t.add(RX_DEMOD, EQ_PREAMBLE, ICK_GENERAL);
        t.add(RX_IC, EQ_PREAMBLE, ICK_GENERAL); t.add(RX_IC, EQ_PREAMBLE, ICK_REALSYM);
        if (mx) t.add(RX_IC, EQ_PREAMBLE, ICK_MFMA);
        break;
    case JIT_PART_RX_BURST:        // the same with block and preamble gathered from a capture (BurstIo)
        t.add(RX_FD, EQ_BURST, ICK_GENERAL); t.add(RX_DEMOD, EQ_BURST, ICK_GENERAL);
        t.add(RX_IC, EQ_BURST, ICK_GENERAL); t.add(RX_IC, EQ_BURST, ICK_REALSYM);
        if (mx) t.add(RX_IC, EQ_BURST, ICK_MFMA);
        break;
    case JIT_PART_MOD:             // plain, behind the resource mapper, framed (TxParams)
        for (int tx = 0; tx < 3; ++tx) t.add(0, EQ_NONE, ICK_GENERAL, tx);
        break;
    case JIT_PART_EST:
        t.add(0, EQ_NONE, ICK_GENERAL);
        break;
    }
    return t;
}

// a variant and its position in its part's list; index -1: the shape has no such kernel
struct Choice { Variant v; int index; };

inline Choice find(int K, int M, const Variant& want)
{
    const PartVariants t = part_variants(K, M, want.part);
    for (int i = 0; i < t.n; ++i)
        if (t.v[i].mode == want.mode && t.v[i].eq == want.eq && t.v[i].ick == want.ick && t.v[i].tx == want.tx) return Choice{ want, i };
    return Choice{ want, -1 };
}

// The receive kernel of a call.  Without cancellation rounds (ic_iter = 0) RX_IC runs the plain demodulator; the rounds go to the matrix
// cores where the handle and the shape allow it (ic_mfma_applies, rowgeom::ic_mfma), else to the vector ALU.
inline Choice select_receive(const DevicePlan& p, const IcParams& ic, const EstPlan* est, int mode, const cf* f_eq)
{
    const bool rounds = (mode == RX_IC && ic.ic_iter > 0);
    const int ick = !rounds ? ICK_GENERAL : (ic_mfma_applies(p, ic) && rowgeom::ic_mfma(p.K, p.M)) ? ICK_MFMA : p.ic_real_sym ? ICK_REALSYM : ICK_GENERAL;
    const bool gather = burst_io(est) != nullptr;
    return find(p.K, p.M, Variant{ gather ? JIT_PART_RX_BURST : est ? JIT_PART_RX_PREAMBLE : rounds ? JIT_PART_RX_IC : JIT_PART_RX,
                                   mode == RX_FD ? RX_FD : rounds ? RX_IC : RX_DEMOD, gather ? EQ_BURST : est ? EQ_PREAMBLE : f_eq ? EQ_VECTOR : EQ_NONE, ick, 0 });
}

inline Choice select_modulate(const DevicePlan& p, const TxParams& tx)
{
    return find(p.K, p.M, Variant{ JIT_PART_MOD, 0, EQ_NONE, ICK_GENERAL, (tx.mapped && tx.framed) ? 2 : tx.mapped ? 1 : 0 });
}

// 16-byte sample accesses of the K = 64 kernels (gfdm_rowlane_impl.h): the launch-uniform flag PLAN_WIDE_IO a launch carries in its own
// copy of the plan.  complex64 pointers may be only 8-byte aligned, so the wide form is chosen per call: every pointer of the call on a
// 16-byte boundary (a block is 8 K M bytes, a multiple of 16 at K = 64) and plain packed blocks on both sides -- the mapper, frame,
// demapper-with-offset and burst paths keep the 8-byte code.  wide_access(): process-wide switch (gfdm_hip_set_wide_access; tests and
// A/B runs turn it off to get the 8-byte route on the same input); GFDM_HIP_WIDE_ACCESS=0 in the environment starts a process with it off.
inline std::atomic<int>& wide_access()
{
    static std::atomic<int> on{ [] { const char* e = getenv("GFDM_HIP_WIDE_ACCESS"); return (e && e[0] == '0' && !e[1]) ? 0 : 1; }() };
    return on;
}

inline bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15u) == 0; }       // (a null pointer is not an operand of the call)

inline int plan_flags_modulate(const DevicePlan& p, const TxParams& tx, const cf* out, const cf* in)
{
    const bool wide = p.K == 64 && !tx.mapped && !tx.framed && aligned16(out) && aligned16(in) && wide_access().load(std::memory_order_relaxed) != 0;
    return p.taps_real | (wide ? (int)PLAN_WIDE_IO : 0);
}

inline int plan_flags_receive(const DevicePlan& p, const IcParams& ic, const EstPlan* est, const cf* out, const cf* in, const cf* f_eq)
{
    const bool wide = p.K == 64 && !burst_io(est) && ic.io.in_stride == 0 && ic.io.in_offset == 0 && aligned16(out) && aligned16(in) && aligned16(f_eq) &&
                      wide_access().load(std::memory_order_relaxed) != 0;
    return p.taps_real | (wide ? (int)PLAN_WIDE_IO : 0);
}

// The subcarrier-FFT roots of a modulate / receive launch: pair-packed per lane behind the table twT points at (gfdm_packed_tables.h)
// where that stage is compiled in for the shape, else the plan's plain wK.  Set in the launch's own copy of the plan, as the flags above;
// the handle's plan keeps the plain table, which the generic family and the estimator kernel read.
inline const cf* plan_roots(const DevicePlan& p, const cf* twT)
{
    return rowgeom::packed_roots(p.K, p.M) ? twT + rowgeom::packed_roots_offset(p.K, p.M) : p.wK;
}

inline Choice select_estimate(const EstPlan& e) { return find(e.K, e.M, Variant{ JIT_PART_EST, 0, EQ_NONE, ICK_GENERAL, 0 }); }

struct Geometry { unsigned grid, block; size_t lds; };       // lds: dynamic LDS bytes

constexpr Geometry geometry(int K, int M, const Variant& v, int64_t nblocks)
{
    const bool pre = (v.eq == EQ_PREAMBLE || v.eq == EQ_BURST);
    size_t lds = rowgeom::lds_bytes(K, pre ? M + 2 : M);                // EQ_PREAMBLE: two more tile columns for the preamble halves
    if (pre || v.part == JIT_PART_EST) lds += rowgeom::est_bytes(K);    // the estimate behind the tiles
    if (v.ick == ICK_MFMA) lds += rowgeom::ic_mfma_edge_bytes(K);       // behind everything else: the wavefronts' edge rows of the IcMfma rounds
    return Geometry{ (unsigned)((nblocks + rowgeom::bpw(K) - 1) / rowgeom::bpw(K)), (unsigned)rowgeom::wg(K), lds };
}

// above the default 64 KiB of dynamic LDS (the largest tiles with the preamble columns and the estimate) a kernel has to opt in
inline hipError_t allow_lds(const void* f, size_t lds)
{
    return lds > 64 * 1024 ? hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

}  // namespace rowvar
}  // namespace gfdm
