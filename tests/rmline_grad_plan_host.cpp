// Host program of tests/test_rmline_train_cpu.py: the plan of a weight gradient of the illustration-to-render module
// (csrc/p3d_rmline_grad_plan.hpp) compiled without any device code.  argv: N CI CO FORCE.  Prints "plan SLICES SETS CI16 CO16 LDS WS" and
// one line "slice S LO HI" per slice, or "error CODE".  Exit status 1 and a line on stderr when the plan breaks what k_rm_wgrad
// (csrc/p3d_rmline_grad.hip) relies on: the slices cover every patch exactly once, in order, none empty; a forced count is taken; a
// wave's accumulator sets cover every (ci block, co block) pair; the largest LDS indices lie inside the allocation, which fits a CU.
#include <stdio.h>
#include <stdlib.h>

#include "p3d_rmline_grad_plan.hpp"

static int fail(const char* what, long long a, long long b) {
    fprintf(stderr, "wgrad plan: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 5) return fail("usage: N CI CO FORCE", argc, 0);
    const int N = atoi(argv[1]), Ci = atoi(argv[2]), Co = atoi(argv[3]), force = atoi(argv[4]);
    RmWgradPlan p;
    const int rc = rm_wgrad_plan(N, Ci, Co, force, &p);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    if (force && p.slices != force) return fail("the forced slice count was not taken", p.slices, force);
    if (p.slices < 1 || p.slices > N || p.slices > P3D_RMLINE_WG_MAX_SLICES) return fail("slices", p.slices, N);
    if (p.ci16 % 16 || p.ci16 < Ci || p.ci16 - Ci > 15 || p.co16 % 16 || p.co16 < Co || p.co16 - Co > 15) return fail("channel pitches", p.ci16, p.co16);
    if (p.nci * 16 != p.ci16 || p.nco * 16 != p.co16) return fail("blocks", p.nci, p.nco);
    if ((p.sets != 1 && p.sets != 4) || 4 * p.sets < p.nci * p.nco) return fail("four waves' sets do not cover the pairs", p.sets, p.nci * p.nco);
    const long long patch = (long long)(RM_WG_ROWS + 2) * RM_PW * p.ci16, dz = (long long)RM_WG_ROWS * RM_TW * p.co16;
    if ((long long)p.lds != 4 * (patch + dz)) return fail("LDS bytes", (long long)p.lds, 4 * (patch + dz));
    if (p.lds > RM_LDS_LIMIT) return fail("more LDS than a CU has", (long long)p.lds, RM_LDS_LIMIT);
    // the largest indices k_rm_wgrad forms: input pixel (rows + 1, RM_PW - 1), channel ci16 - 1; dz pixel 255, channel co16 - 1
    if (((long long)(RM_WG_ROWS + 1) * RM_PW + RM_PW - 1) * p.ci16 + p.ci16 - 1 >= patch) return fail("a patch index beyond the patch", patch, 0);
    if ((long long)(RM_WG_ROWS * RM_TW - 1) * p.co16 + p.co16 - 1 >= dz) return fail("a dz index beyond its tile", dz, 0);
    if (p.ws_floats != (long long)p.slices * (9LL * Ci * Co + 2 * Co)) return fail("workspace", p.ws_floats, p.slices);
    printf("plan %d %d %d %d %zu %lld\n", p.slices, p.sets, p.ci16, p.co16, p.lds, (long long)p.ws_floats);
    int next = 0;
    for (int s = 0; s < p.slices; ++s) {
        int lo, hi;
        rm_wgrad_slice(s, p.slices, N, &lo, &hi);
        if (lo != next || hi <= lo) return fail("a slice does not continue the one before, or is empty", lo, hi);
        next = hi;
        printf("slice %d %d %d\n", s, lo, hi);
    }
    if (next != N) return fail("the slices do not end at N", next, N);
    return 0;
}
