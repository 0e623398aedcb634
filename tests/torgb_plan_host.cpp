// Host program of tests/test_torgb_cases_cpu.py: the ToRGB launch plan (csrc/p3d_torgb_plan.hpp) compiled without any device code.
// stdin, one line per request:
//   p N I O H W   print the plan of one p3d_torgb_f32 call: the instantiation, the grid (x y z), the dynamic LDS bytes; or "err CODE"
// Exit status 1 and a line on stderr for every plan that k_torgb could not run as it indexes its launch (see check()).
#include <stdio.h>

#include "p3d_torgb_plan.hpp"

static const char* kernel_name(TorgbKernel k) {
    switch (k) {
    case TorgbKernel::PX1: return "k_torgb<1,false>";
    case TorgbKernel::KS1: return "k_torgb<1,true>";
    case TorgbKernel::PX3: return "k_torgb<3,false>";
    case TorgbKernel::KS3: return "k_torgb<3,true>";
    case TorgbKernel::MS: return "k_torgb<1,true,true>";
    case TorgbKernel::MS_PRE: return "k_torgb<1,true,true,true>";
    }
    return "?";
}

// What the plan cannot know from its own formulas: what k_torgb (csrc/p3d_torgb.hip) does with a launch of that shape.
static int check(const TorgbPlan& p, int N, int I, int O, int H, int W) {
    const bool px = p.kernel == TorgbKernel::PX1 || p.kernel == TorgbKernel::PX3;
    const bool ms = p.kernel == TorgbKernel::MS || p.kernel == TorgbKernel::MS_PRE;
    const int MT = (p.kernel == TorgbKernel::PX3 || p.kernel == TorgbKernel::KS3) ? 3 : 1;  // the instantiation's channel tiles
    const long long HW = (long long)H * W, tile = px ? 128 : 32;  // pixels of a workgroup: p0 = blockIdx.x * 128 + wave * 32, or blockIdx.x * 32
    const char* bad = nullptr;
    // every pixel has a workgroup and no workgroup is without one (an empty one would clamp all its lanes to HW - 1)
    if ((long long)p.gx * tile < HW || (long long)(p.gx - 1) * tile >= HW) bad = "grid.x does not cover the map tightly";
    // n = blockIdx.y; the channel tile = blockIdx.z in the MS forms only, and 32 * MT * grid.z channels must reach O
    else if (p.gy != (unsigned)N || (!ms && p.gz != 1) || 32ll * MT * p.gz < O) bad = "grid.y / grid.z do not cover N x O";
    // the styles sit behind the two A buffers: Ss[i], i < 512 (PRE) or I rounded up to whole chunks
    else if (p.lds_bytes < (2 * (size_t)TG_KC * 32 * MT + (p.kernel == TorgbKernel::MS_PRE ? 512 : (size_t)(I + 63) / 64 * 64)) * 4) bad = "the styles do not fit the LDS";
    else if (p.kernel == TorgbKernel::MS_PRE && I > 512) bad = "PRE holds eight chunks in registers";
    // the KS epilogue's partial sums [4 waves][16 MT][64 lanes] reuse the LDS from its start
    else if (!px && (size_t)4 * 16 * MT * 64 * 4 > p.lds_bytes) bad = "the partial sums do not fit the LDS";
    else if (p.lds_bytes > 64 * 1024) bad = "beyond the default dynamic-LDS limit";
    if (!bad) return 0;
    fprintf(stderr, "N=%d I=%d O=%d H=%d W=%d: %s\n", N, I, O, H, W, bad);
    return 1;
}

int main() {
    char line[256];
    int nbad = 0, N, I, O, H, W;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "p %d %d %d %d %d", &N, &I, &O, &H, &W) != 5) continue;
        const TorgbPlan p = p3d_torgb_plan(N, I, O, H, W);
        if (p.err) {
            printf("err %d\n", p.err);
            continue;
        }
        nbad += check(p, N, I, O, H, W);
        printf("%s %u %u %u %zu\n", kernel_name(p.kernel), p.gx, p.gy, p.gz, p.lds_bytes);
    }
    return nbad ? 1 : 0;
}
