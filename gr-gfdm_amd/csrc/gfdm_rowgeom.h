// Launch geometry of the row-lane kernels as plain constexpr functions of the shape: ONE definition for the kernels
// (gfdm_rowlane_impl.h) and for the host code that launches them, compiled or instantiated at run time (gfdm_rowvariants.h).
#pragma once
#ifndef __HIPCC_RTC__
#include <stddef.h>
#endif

#ifndef GFDM_ROW_WG
#define GFDM_ROW_WG 256
#endif

namespace gfdm {
namespace rowgeom {

// Subcarrier counts the family covers: powers of two 4 .. 1024 (radix-4 / wide passes, gfdm_rowlane_impl.h), and every other K <= 1024
// that splits into two or three factors the butterfly codelets hold in registers -- Dft<R> for R <= 16 where such a plan exists
// (96 = 6 x 16, 12, 48, 240; 200 = 2 x 10 x 10, 384, 600, 1000), else R <= 32 (34 = 2 x 17, 62 = 2 x 31, 51, 93, 589 = 19 x 31, a prime
// K <= 31 itself).  Two passes are preferred to three; two-pass plans with factors <= 16 stay below K = 256.
//   the LAST pass takes the largest divisor <= lim, the pass(es) in front the same rule on the quotient; R0 = 1: a single pass
constexpr bool pow2(int K) { return K > 0 && (K & (K - 1)) == 0; }
constexpr int ldiv(int K, int lim)                                           // the largest divisor of K that is <= lim
{
    int r = 1;
    for (int d = 2; d <= lim && d <= K; ++d)
        if (K % d == 0) r = d;
    return r;
}
constexpr bool plan2(int K, int lim) { return K / ldiv(K, lim) <= lim; }
constexpr bool plan3(int K, int lim) { return ldiv(K, lim) > 1 && ldiv(K / ldiv(K, lim), lim) > 1 && plan2(K / ldiv(K, lim), lim); }
// radix limit of K's plan: 16 if a two- or three-pass plan with factors <= 16 exists, else 32
constexpr int plan_lim(int K) { return ((K <= 256 && plan2(K, 16)) || plan3(K, 16)) ? 16 : 32; }
constexpr bool mixed(int K)                                                   // two passes
{
    return !pow2(K) && K >= 3 && K <= 1024 && ((K <= 256 && plan2(K, 16)) || (!plan3(K, 16) && plan2(K, 32)));
}
constexpr int mixed_r1(int K) { return ldiv(K, plan_lim(K)); }
constexpr int mixed_r0(int K) { return K / mixed_r1(K); }
constexpr bool mixed3(int K)                                                  // three passes
{
    return !pow2(K) && !mixed(K) && K >= 3 && K <= 1024 && (plan3(K, 16) || plan3(K, 32));
}
constexpr int mixed3_r2(int K) { return ldiv(K, plan_lim(K)); }
constexpr int mixed3_r1(int K) { return ldiv(K / mixed3_r2(K), plan_lim(K)); }
constexpr int mixed3_r0(int K) { return K / mixed3_r2(K) / mixed3_r1(K); }
constexpr bool supported(int K) { return (pow2(K) && K >= 4 && K <= 1024) || mixed(K) || mixed3(K); }

// threads per workgroup: whole blocks only (a block never straddles two workgroups)
constexpr int wg(int K) { return K >= 128 ? K : pow2(K) ? GFDM_ROW_WG : (GFDM_ROW_WG / K) * K; }
// blocks of K lanes that sit inside ONE wavefront are ordered by the wave's program order; others need the workgroup barrier
constexpr bool wave_local(int K) { return K <= 64 && 64 % K == 0; }
constexpr int bpw(int K) { return wg(K) / K; }                               // blocks per workgroup
constexpr int tile_stride(int K, int M) { return K * M + (bpw(K) > 1 ? 16 : 0); }   // complex elements between the tiles of a workgroup
constexpr size_t lds_bytes(int K, int M) { return (size_t)bpw(K) * (size_t)tile_stride(K, M) * 8 + 64; }
// Matrix-core form of the interference-cancellation rounds (IcMfma in gfdm_rowlane_impl.h): 64-row aligned wavefronts of whole 16-row
// groups and a timeslot row within the 16 x 16 tile of v_mfma_f32_16x16x32_f16.  Since round 4 the rounds keep everything in registers
// (lane-row transposes, DPP row shifts); only blocks that span several wavefronts pass each wavefront's two edge rows through LDS:
// [2 buffers][wavefront][first | last row][component][lane row] x 8 bytes behind the tiles.
constexpr bool ic_mfma(int K, int M) { return pow2(K) && K >= 16 && M >= 4 && M <= 16; }
// ... and where it is the default (measured, profiles/README.md)
constexpr bool ic_mfma_preferred(int K, int M) { return ic_mfma(K, M) && K >= 128; }
constexpr size_t ic_mfma_pad_bytes(int K) { return wave_local(K) ? 0 : (size_t)(K / 4) * 8; }      // padding of the rounds' tile layout (one element per 4 rows)
constexpr size_t ic_mfma_edge_bytes(int K) { return wave_local(K) ? 0 : (size_t)2 * (K / 64) * 2 * 2 * 4 * 8 + ic_mfma_pad_bytes(K); }
constexpr int est_stride(int K) { return K + 10; }                           // EQ_PREAMBLE: edge-extended estimate bins per block
constexpr size_t est_bytes(int K) { return (size_t)bpw(K) * (size_t)est_stride(K) * 8; }

// ---- per-lane tables fetched in 16-byte pairs (gfdm_packed_tables.h, "Per-lane tables in 16-byte pairs" in gfdm_rowlane_impl.h) ----
// Both knobs are read by the kernels AND by the host code that builds the tables and launches (compiled and run-time route): 0 compiles a
// stage out everywhere and leaves the [m][K] twiddle table and the plain wK roots.
// Measured defaults (profiles/r14/packed_tables_ab.csv, profiles/EXPERIMENTS.md "Per-lane tables in 16-byte pairs"; K=64 M=9 L=2, 4096 blocks, builds in
// alternating processes on one MI355X, three visits of three rounds; kernel = steady-state duration alone on its stream, step = modulate + MF demodulate
// pipelined over three streams as bench.py runs it; repeats of one build spread by 0.01 us resp. 0.5-0.9 % sustained and 2-3 % over the 200-step burst):
//   TWT   = 1   modulate 9.08 -> 8.39 us, demodulate 9.23 -> 8.61 us, sustained step rate +3.2 ... +4.3 % in every round of all visits (3.08-3.15e8 -> 3.18-3.27e8
//               blocks/s), the 200-step burst +2.4 ... +6.8 %; ZF + 2 IC step (cfg3) +1.2 ... +3.1 %, K=256 M=31 (cfg5) +0.4 %
#ifndef GFDM_PACKED_TWT
#define GFDM_PACKED_TWT 1
#endif
//   ROOTS = 0   the kernels alone gain (modulate 9.08 -> 8.55 us, demodulate 9.23 -> 8.90 us; with TWT 8.25 / 8.39 us) but the pipelined step does not: alone
//               -0.7 ... +0.6 % against the parent (inside the spread), on top of TWT the step ties or loses against TWT alone (-1.1 ... -0.1 %, six rounds),
//               and alone it LOSES 1.2 % at K=256 M=31 (cfg5) in every round
#ifndef GFDM_PACKED_ROOTS
#define GFDM_PACKED_ROOTS 0
#endif
// The first pass(es) of the subcarrier FFT (RowShape in gfdm_rowlane_impl.h states the same plan; static_asserts there hold the two together)
constexpr int wide_r0(int K) { return K == 256 ? 16 : K == 128 ? 8 : mixed(K) ? mixed_r0(K) : mixed3(K) ? mixed3_r0(K) : (K == 512 || K == 1024) ? 8 : 1; }
constexpr int wide_r1(int K) { return (K == 256 || K == 128) ? 16 : mixed(K) ? mixed_r1(K) : mixed3(K) ? mixed3_r1(K) : (K == 512 || K == 1024) ? 8 : 1; }
constexpr bool wide3(int K) { return K == 512 || K == 1024 || mixed3(K); }
constexpr bool wide(int K) { return K == 256 || K == 128 || mixed(K) || wide3(K); }
// Roots of unity a lane of k_row_receive / k_row_modulate reads from wK before its first transform, in the order it consumes them:
//   wide plans      W_K^{tq u}, u = 1 .. R0 - 1 (first pass), then for three passes W_K^{qq R0 u}, u = 1 .. R1 - 1 (middle pass)
//   radix-4 plans   three roots for every pass that has any (K / 4^s > 4); K = 64 runs pass 0 from the registers and ONE radix-16 pass
//                   behind it, so only pass 0's roots are read
constexpr int root_count(int K)
{
    if (wide(K)) return (wide_r0(K) - 1) + (wide3(K) ? wide_r1(K) - 1 : 0);
    if (K == 64) return 3;
    int n = 0;
    for (int len = K; len >= 4; len /= 4)
        if (len / 4 > 1) n += 3;
    return n;
}
// index into wK of root i of lane `lane` (the lane's place in its block)
constexpr int root_index(int K, int lane, int i)
{
    if (wide(K)) {
        const int R0 = wide_r0(K), R1 = wide_r1(K);
        if (i < R0 - 1) return (lane % (K / R0)) * (i + 1) % K;
        return ((lane % (K / R1)) / R0) * R0 * (i - (R0 - 1) + 1) % K;
    }
    int str = 1;
    for (int s = 0; s < i / 3; ++s) str *= 4;
    return ((lane % (K / 4)) / str) * (i % 3 + 1) * str % K;
}
// Where a stage applies.  A shape on which a stage costs some kernel registers down to the next occupancy step is excluded HERE, never by a
// register bound (-Rpass-analysis=kernel-resource-usage over the 13 compiled shapes, VGPRs / waves per SIMD, no kernel gains scratch):
//   twiddles  K=128 M=15 (L = 2 and 4): k_row_receive<.,1,0,0> 78 / 6 -> 83 / 5, <.,2,0,2> (the matrix-core rounds) 96 / 5 -> 97 / 4, the burst
//             demodulator 91 / 5 -> 97 / 4;  K=128 M=21: <.,0,2,0> 90 / 5 -> 104 / 4;  K=4 M=16: <.,0,0,0> 64 / 8 -> 77 / 6, <.,1,2,0> 78 / 6 -> 86 / 5
//   roots     K=128 M=15: <.,0,0,0> 71 / 7 -> 75 / 6, <.,1,0,0> 78 / 6 -> 81 / 5;  K=96 M=25: <.,1,0,0> 105 / 4 -> 129 / 3
// With these out, no kernel of the compiled shapes drops a step with either stage or both.
constexpr bool packed_twt(int K, int M)
{
    return GFDM_PACKED_TWT != 0 && M >= 3 && !(K == 128 && (M == 15 || M == 21)) && !(K == 4 && M == 16);
}
constexpr bool packed_roots(int K, int M)
{
    return GFDM_PACKED_ROOTS != 0 && root_count(K) >= 2 && !(K == 128 && M == 15) && !(K == 96 && M == 25);
}
// complex elements of a pair-packed table of n entries per lane; of the region a row-lane launch's twT points at -- [m][K] or pair-packed, M K
// elements either way -- behind which the packed roots lie (the launchers point their copy of the plan's wK there)
constexpr size_t packed_elems(int n, int K) { return ((size_t)n * (size_t)K + 1) & ~(size_t)1; }
constexpr size_t packed_roots_offset(int K, int M) { return packed_elems(M, K); }

}  // namespace rowgeom
}  // namespace gfdm
