// Row-lane kernels of ONE shape and ONE part (gfdm_rowlane_impl.h): compiled by the Makefile once per entry of gfdm_row_shapes.h and
// per part with -DGFDM_SHAPE_K= -DGFDM_SHAPE_M= -DGFDM_SHAPE_L= -DGFDM_SHAPE_PART= (JIT_PART_*: the kernels of rowvar::part_variants).
#include "gfdm_rowlane_impl.h"
#include "gfdm_rowvariants.h"

#include <array>
#include <utility>

#if !defined(GFDM_SHAPE_K) || !defined(GFDM_SHAPE_M) || !defined(GFDM_SHAPE_L) || !defined(GFDM_SHAPE_PART)
#error "compile with -DGFDM_SHAPE_K=.. -DGFDM_SHAPE_M=.. -DGFDM_SHAPE_L=.. -DGFDM_SHAPE_PART=.."
#endif

namespace gfdm {
namespace {

constexpr int K = GFDM_SHAPE_K, M = GFDM_SHAPE_M, L = GFDM_SHAPE_L, PART = GFDM_SHAPE_PART;
static_assert(rowgeom::lds_bytes(K, M) <= 64 * 1024, "row-lane tile exceeds the default dynamic LDS limit");
constexpr rowvar::PartVariants kPart = rowvar::part_variants(K, M, PART);

template <int I> const void* kernel()
{
    constexpr rowvar::Variant v = kPart.v[I];
    if constexpr (PART == JIT_PART_MOD) return reinterpret_cast<const void*>(k_row_modulate<K, M, L, v.tx>);
    else if constexpr (PART == JIT_PART_EST) return reinterpret_cast<const void*>(k_row_estimate<K, M>);
    else if constexpr (PART == JIT_PART_RX_BURST) return reinterpret_cast<const void*>(k_row_receive_burst<K, M, L, v.mode, v.ick>);
    else return reinterpret_cast<const void*>(k_row_receive<K, M, L, v.mode, v.eq, v.ick>);
}

template <int... I> std::array<const void*, sizeof...(I)> kernels(std::integer_sequence<int, I...>) { return { kernel<I>()... }; }
const auto kKernels = kernels(std::make_integer_sequence<int, kPart.n>());

}  // namespace

// the part's kernels in table order, rowlane_<K>_<M>_<L>_p<part> (gfdm_rowlane.hip); the -D values are expanded before they are pasted
#define GFDM_ROWLANE_EXPORT_I(K_, M_, L_, P_) extern const void* const* const rowlane_##K_##_##M_##_##L_##_p##P_ = kKernels.data();
#define GFDM_ROWLANE_EXPORT(K_, M_, L_, P_) GFDM_ROWLANE_EXPORT_I(K_, M_, L_, P_)
GFDM_ROWLANE_EXPORT(GFDM_SHAPE_K, GFDM_SHAPE_M, GFDM_SHAPE_L, GFDM_SHAPE_PART)

}  // namespace gfdm

#if defined(GFDM_STAMPS)      /* diagnostic build only (scratch/stamps.py): one setter per translation unit, each has its own g_stamp_buf */
#define GFDM_STAMP_SETTER_I(K_, M_, L_, P_) extern "C" int gfdm_debug_set_stamp_buffer_##K_##_##M_##_##L_##_p##P_(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(gfdm::g_stamp_buf), &p, sizeof(p)); }
#define GFDM_STAMP_SETTER(K_, M_, L_, P_) GFDM_STAMP_SETTER_I(K_, M_, L_, P_)
GFDM_STAMP_SETTER(GFDM_SHAPE_K, GFDM_SHAPE_M, GFDM_SHAPE_L, GFDM_SHAPE_PART)
#endif
