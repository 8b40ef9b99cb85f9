// Stand-alone check of the pair-packed per-lane tables (gr-gfdm_amd/csrc/gfdm_packed_tables.h), driven by tests/test_packed_tables.py:
//   packed_tables_host K M [K M ...]
// For every shape it builds the plain tables as the plan builder does ([M][K] twiddles W_N^{q m}, [K] roots W_K^q), packs them behind a
// prefix of other tables, and reads them back THE WAY THE KERNELS DO (gfdm_rowlane_impl.h, load_lane_packed: entry pair j of lane q as the
// 16 bytes at element 2 (j K + q), the last entry of an odd count as the 8 bytes at element 2 (n / 2) K + q):
//   * every unpacked twiddle and root has the bits of the plain table's value,
//   * the roots are the ones the plain code of load_fft_twiddles reads, in that order (restated here from the pass plans, not taken from
//     rowgeom::root_index),
//   * every plane starts on a 16-byte boundary and every 16-byte read is aligned,
//   * the twiddle region keeps the M K (+ 1) elements of the plain table (the roots lie packed_roots_offset behind its start).
// Prints one line per shape and "ok"; any mismatch prints the first offender and exits with 1.
#include "gfdm_packed_tables.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct c32 { float x, y; };
static_assert(sizeof(c32) == 8, "a complex sample is 8 bytes");

bool same_bits(const c32& a, const c32& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int fails = 0;
void fail(const char* what, int K, int M, int q, int i)
{
    if (fails++ == 0) std::printf("MISMATCH %s: K=%d M=%d lane %d entry %d\n", what, K, M, q, i);
}

std::vector<c32> unit_roots(int n)
{
    std::vector<c32> w(n);
    for (int i = 0; i < n; ++i) {
        const double a = -6.283185307179586476925286766559 * (double)i / (double)n;
        w[i] = c32{ (float)std::cos(a), (float)std::sin(a) };
    }
    return w;
}

// what the kernel's loads return: entry i of lane q of a pair-packed table of n entries per lane that starts at `tab`
c32 kernel_read(const c32* tab, int n, int K, int q, int i, int M)
{
    if (n % 2 && i == n - 1) return tab[(size_t)(n / 2) * 2 * K + q];
    const c32* pair = tab + 2 * ((size_t)(i / 2) * K + q);
    if (reinterpret_cast<uintptr_t>(pair) % 16 != 0) fail("16-byte read not aligned", K, M, q, i);
    c32 both[2];
    std::memcpy(both, pair, 16);
    return both[i % 2];
}

// the wK indices lane `lane` reads in the plain code of load_fft_twiddles, in program order
std::vector<int> plain_root_indices(int K, int lane)
{
    namespace g = gfdm::rowgeom;
    std::vector<int> idx;
    const bool wide3 = (K == 512 || K == 1024 || g::mixed3(K));
    const bool wide = (K == 256 || K == 128 || g::mixed(K) || wide3);
    if (wide) {
        const int R0 = K == 256 ? 16 : K == 128 ? 8 : g::mixed(K) ? g::mixed_r0(K) : g::mixed3(K) ? g::mixed3_r0(K) : 8;
        const int R1 = (K == 256 || K == 128) ? 16 : g::mixed(K) ? g::mixed_r1(K) : g::mixed3(K) ? g::mixed3_r1(K) : 8;
        const int tq0 = lane % (K / R0);
        for (int u = 1; u < R0; ++u) idx.push_back(tq0 * u % K);
        if (wide3) {
            const int qq = (lane % (K / R1)) / R0;
            for (int u = 1; u < R1; ++u) idx.push_back(qq * R0 * u % K);
        }
        return idx;
    }
    int log2K = 0;
    while ((1 << log2K) < K) ++log2K;
    const int NP4 = (K == 64) ? 1 : log2K / 2;      // K = 64: pass 0 from the registers, then one radix-16 pass without twiddles
    const int tq = lane % (K / 4);
    for (int s = 0; s < NP4; ++s) {
        const int str = 1 << (2 * s), ms = K / str / 4;
        if (ms > 1) {
            const int qq = tq / str;
            for (int c = 1; c <= 3; ++c) idx.push_back((qq * c * str) & (K - 1));
        }
    }
    return idx;
}

void check_shape(int K, int M)
{
    namespace g = gfdm::rowgeom;
    const int N = K * M;
    const std::vector<c32> wK = unit_roots(K);
    std::vector<c32> twT((size_t)N);
    for (int m = 0; m < M; ++m)
        for (int q = 0; q < K; ++q) {
            const double a = -6.283185307179586476925286766559 * (double)(((int64_t)q * m) % N) / (double)N;
            twT[(size_t)m * K + q] = c32{ (float)std::cos(a), (float)std::sin(a) };
        }

    // a blob as the plan builder lays it out: other tables in front (an even number of elements), then the packed twiddles, then the roots
    std::vector<c32> blob(2 * (size_t)(M + K), c32{ -1.f, -1.f });
    const size_t tw_at = blob.size();
    gfdm::packed::append_twiddles(blob, twT.data(), M, K);
    const size_t roots_at = blob.size();
    gfdm::packed::append_roots(blob, wK.data(), K);
    const int nr = g::root_count(K);
    if (reinterpret_cast<uintptr_t>(blob.data()) % 16 != 0) { std::printf("the allocation itself is not 16-byte aligned\n"); std::exit(2); }

    if (roots_at - tw_at != g::packed_roots_offset(K, M) || roots_at - tw_at < (size_t)N) fail("twiddle region size", K, M, 0, 0);
    if (blob.size() - roots_at != g::packed_elems(nr, K)) fail("root region size", K, M, 0, 0);
    const c32* tw = blob.data() + tw_at;
    const c32* roots = blob.data() + roots_at;
    // planes: pair plane j at 2 j K, the single plane of an odd count at 2 (n / 2) K
    for (int j = 0; j <= (M - 1) / 2; ++j)
        if (reinterpret_cast<uintptr_t>(tw + (size_t)2 * j * K) % 16 != 0) fail("twiddle plane alignment", K, M, 0, 2 * j);
    for (int j = 0; j <= nr / 2; ++j)
        if (reinterpret_cast<uintptr_t>(roots + (size_t)2 * j * K) % 16 != 0) fail("root plane alignment", K, M, 0, 2 * j);

    for (int q = 0; q < K; ++q) {
        for (int m = 1; m < M; ++m)
            if (!same_bits(kernel_read(tw, M - 1, K, q, m - 1, M), twT[(size_t)m * K + q])) fail("twiddle", K, M, q, m - 1);
        const std::vector<int> idx = plain_root_indices(K, q);
        if ((int)idx.size() != nr) { fail("root count", K, M, q, (int)idx.size()); continue; }
        for (int i = 0; i < nr; ++i) {
            if (idx[i] != g::root_index(K, q, i)) fail("root index", K, M, q, i);
            if (!same_bits(kernel_read(roots, nr, K, q, i, M), wK[idx[i]])) fail("root", K, M, q, i);
        }
    }
    std::printf("K=%d M=%d: %d twiddles (%d 16-byte + %d 8-byte loads), %d roots (%d + %d)\n", K, M, M - 1, (M - 1) / 2, (M - 1) % 2, nr, nr / 2, nr % 2);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3 || argc % 2 == 0) { std::printf("usage: packed_tables_host K M [K M ...]\n"); return 2; }
    for (int i = 1; i + 1 < argc; i += 2) check_shape(std::atoi(argv[i]), std::atoi(argv[i + 1]));
    if (fails) { std::printf("%d mismatches\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
