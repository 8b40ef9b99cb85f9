// Every timeslot codelet of csrc/gfdm_dft.h on the CPU (tests/test_codelets.py compiles and runs this; -x hip --offload-host-only).
//
// The header is included UNMODIFIED; only __device__ is redefined so that its functions exist on the host as well.  dft_inplace<N, INV> is
// instantiated for every N = 1 .. 48 in both directions by a template loop (no list to fall out of date):
//
//     dft_codelets_host <in> <out> <B>
//
// <in>: for N = 1 .. 48, for INV = 0, 1: B vectors of N complex64 (raw float32 pairs); <out>: the transforms, in the same layout.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "gfdm_dft.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

#ifndef DFT_MAX_N
#define DFT_MAX_N 48
#endif

static int g_instantiated = 0;

template <int N, bool INV>
static void run_one(const float*& in, float*& out, int B)
{
    for (int b = 0; b < B; ++b, in += 2 * N, out += 2 * N) {
        gfdm::dft::cf x[N];
        for (int n = 0; n < N; ++n) x[n] = make_float2(in[2 * n], in[2 * n + 1]);
        gfdm::dft::dft_inplace<N, INV>(x);
        for (int n = 0; n < N; ++n) { out[2 * n] = x[n].x; out[2 * n + 1] = x[n].y; }
    }
    ++g_instantiated;
}

template <int N>
static void run_from(const float*& in, float*& out, int B)
{
    run_one<N, false>(in, out, B);
    run_one<N, true>(in, out, B);
    if constexpr (N < DFT_MAX_N) run_from<N + 1>(in, out, B);
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s <in> <out> <vectors per codelet>\n", argv[0]); return 2; }
    const int B = atoi(argv[3]);
    const size_t total = (size_t)B * 2 * 2 * (DFT_MAX_N * (DFT_MAX_N + 1) / 2);     // floats: B vectors x 2 directions x sum of N x (re, im)
    std::vector<float> in(total), out(total);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), sizeof(float), total, f) != total || fgetc(f) != EOF) { fprintf(stderr, "%s: not %zu floats\n", argv[1], total); return 1; }
    fclose(f);
    const float* pi = in.data();
    float* po = out.data();
    run_from<1>(pi, po, B);
    if (pi != in.data() + total || po != out.data() + total) { fprintf(stderr, "layout error\n"); return 1; }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(float), total, f) != total || fclose(f) != 0) { fprintf(stderr, "%s: write failed\n", argv[2]); return 1; }
    printf("%d instantiations, N = 1 .. %d\n", g_instantiated, DFT_MAX_N);
    return 0;
}
