// Host program of tests/test_rmline_cpu.py: the plan of one generator layer (csrc/p3d_rmline_plan.hpp) compiled without any device code.
// argv: CI CO FORCE.  Prints "plan PLAN ROWS CI4 CIP COT CBLOCKS LDS", or "error CODE".  Exit status 1 and a line on stderr when the plan
// breaks what k_rm_conv (csrc/p3d_rmline.hip) relies on: the channel pitch even (8-byte LDS stores), == 2 mod 4 (conflict-free operand
// reads) and at least the padded channel count; the workgroups along Co covering every output channel exactly once with at most two
// 16-channel blocks each; the largest LDS index the kernel forms inside the allocation; the allocation within one CU's LDS.
#include <stdio.h>
#include <stdlib.h>

#include "p3d_rmline_plan.hpp"

static int fail(const char* what, long long a, long long b) {
    fprintf(stderr, "plan: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 4) return fail("usage: CI CO FORCE", argc, 0);
    const int Ci = atoi(argv[1]), Co = atoi(argv[2]), force = atoi(argv[3]);
    RmPlan p;
    const int rc = rm_conv_plan(Ci, Co, force, &p);
    if (rc) {
        printf("error %d\n", rc);
        return 0;
    }
    if (p.rows != 8 && p.rows != 4) return fail("rows", p.rows, 0);
    if ((p.plan == P3D_RMLINE_TILE_8) != (p.rows == 8)) return fail("plan and rows disagree", p.plan, p.rows);
    if (force && p.plan != force) return fail("the forced plan was not taken", p.plan, force);
    if (p.ci4 % 4 || p.ci4 < Ci || p.ci4 - Ci > 3) return fail("ci4", p.ci4, Ci);
    if (p.cip % 2 || p.cip % 4 != 2 || p.cip < p.ci4) return fail("the channel pitch", p.cip, p.ci4);
    if (p.cot != 16 && p.cot != 32) return fail("cot", p.cot, 0);
    if (p.cblocks * p.cot < Co || (p.cblocks - 1) * p.cot >= Co) return fail("the workgroups along Co do not cover it exactly", p.cblocks, p.cot);
    const long long patch = (long long)(p.rows + 2) * RM_PW * p.cip, weights = 9LL * p.cot * p.cip;
    if ((long long)p.lds != 4 * (patch + weights)) return fail("LDS bytes", (long long)p.lds, 4 * (patch + weights));
    if (p.lds > RM_LDS_LIMIT) return fail("more LDS than a CU has", (long long)p.lds, RM_LDS_LIMIT);
    // the largest indices k_rm_conv forms: pixel (rows + 1, RM_PW - 1), channel ci4 - 1; filter (tap 8, cot - 1), channel ci4 - 1
    if (((long long)(p.rows + 1) * RM_PW + RM_PW - 1) * p.cip + p.ci4 - 1 >= patch) return fail("a patch index beyond the patch", patch, 0);
    if ((8LL * p.cot + p.cot - 1) * p.cip + p.ci4 - 1 >= weights) return fail("a weight index beyond the weights", weights, 0);
    if (patch % 2) return fail("the weights start on an odd float", patch, 0);
    printf("plan %d %d %d %d %d %d %zu\n", p.plan, p.rows, p.ci4, p.cip, p.cot, p.cblocks, p.lds);
    return 0;
}
