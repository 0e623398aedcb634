// Host program of tests/test_cull_band_cpu.py: the cull band (csrc/p3d_cull_band.hpp) compiled without any device code.
// One argument per threshold; prints one line per threshold, "<thresh> <s_lo> <s_hi> <delta>", every float as its %a image
// (inf / -inf for an open side) and the header's delta last.
#include <stdio.h>
#include <stdlib.h>

#include "p3d_cull_band.hpp"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const float t = strtof(argv[i], nullptr);
        float lo, hi;
        p3d_cull_band(t, &lo, &hi);
        printf("%a %a %a %a\n", (double)t, (double)lo, (double)hi, (double)P3D_CULL_BAND_DELTA);
    }
    return 0;
}
