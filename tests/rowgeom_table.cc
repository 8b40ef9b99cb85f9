// The plan table of the run-time row-lane family, printed from csrc/gfdm_rowgeom.h itself (tests/test_codelets.py compiles and reads it):
// one line per K = 1 .. 1024
//
//     K supported pow2 lim passes r0 r1 r2 wg bpw  bytes(M) ...
//
// passes / r0 r1 r2: the wide passes of a K that is not a power of two, in the order they run (the LAST one is the last column that is
// not 0; a single pass prints passes = 1; a power of two prints passes = 0: its passes are chosen in gfdm_rowlane_impl.h);
// bytes(M) = lds_bytes(K, M + 2) + est_bytes(K), the sum jit_eligible() holds against 160 KiB, for every M given on the command line.
#include <stdio.h>
#include <stdlib.h>

#include "gfdm_rowgeom.h"

namespace g = gfdm::rowgeom;

int main(int argc, char** argv)
{
    for (int K = 1; K <= 1024; ++K) {
        int r[3] = { 0, 0, 0 }, passes = 0;
        if (g::mixed(K)) {
            if (g::mixed_r0(K) > 1) r[passes++] = g::mixed_r0(K);
            r[passes++] = g::mixed_r1(K);
        } else if (g::mixed3(K)) {
            r[0] = g::mixed3_r0(K); r[1] = g::mixed3_r1(K); r[2] = g::mixed3_r2(K);
            passes = 3;
        }
        printf("%d %d %d %d %d %d %d %d %d %d", K, (int)g::supported(K), (int)g::pow2(K), g::plan_lim(K), passes, r[0], r[1], r[2], g::wg(K), g::bpw(K));
        for (int i = 1; i < argc; ++i) {
            const int M = atoi(argv[i]);
            printf(" %zu", g::lds_bytes(K, M + 2) + g::est_bytes(K));
        }
        printf("\n");
    }
    return 0;
}
