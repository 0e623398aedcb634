// Host program of tests/test_interior_taps_cpu.py: the launch's interior-taps decision (csrc/p3d_render_plan.hpp) compiled without
// any device code, with contraction off.  One geometry per five arguments "<coord_scale> <crop_limit> <H> <W> <flags>" (floats as
// their %a image); prints one line per geometry:
//   <decision> <floor(ix(-L))> <floor(ix(+L))> <min floor(ix)> <max floor(ix)> <points> <order violations>
// the last four from a sweep of the plan's chain p3d_tap_coord over every float within 2^16 floats of -L and of +L and every 4096th
// bit pattern of [-L, L], each point taken only where |p| <= L.  An order violation is a pair of neighbouring points of the sweep,
// taken in increasing p, whose ix decreases.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p3d_render_plan.hpp"

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct Sweep {
    float half, scale, L, lo = INFINITY, hi = -INFINITY, prev_ix = -INFINITY;
    long long n = 0, bad = 0;
    void at(float p) {  // called in increasing p
        if (!(fabsf(p) <= L)) return;
        const float ix = p3d_tap_coord(p, scale, half), f = floorf(ix);
        lo = f < lo ? f : lo;
        hi = f > hi ? f : hi;
        bad += ix < prev_ix ? 1 : 0;
        prev_ix = ix;
        ++n;
    }
};

int main(int argc, char** argv) {
    for (int i = 1; i + 4 < argc; i += 5) {
        p3d_opts o;
        memset(&o, 0, sizeof(o));
        o.coord_scale = strtof(argv[i], nullptr);
        o.crop_limit = strtof(argv[i + 1], nullptr);
        const int H = atoi(argv[i + 2]), W = atoi(argv[i + 3]);
        o.flags = atoi(argv[i + 4]);
        const float L = o.crop_limit, half = 0.5f * (float)W;
        Sweep s;
        s.half = half; s.scale = o.coord_scale; s.L = L;
        if (L > 0.0f && isfinite(L)) {
            const uint32_t bl = bits_of(L);  // positive floats order like their bit patterns
            const uint32_t w = 1u << 16, top = bl + w, inner = bl > w ? bl - w : 0u;
            // the magnitudes: every 4096th bit pattern of [0, inner), then every one of [inner, top]; negative side first, descending
            for (uint32_t u = top; u > inner; --u) s.at(-float_of(u));
            s.at(-float_of(inner));
            if (inner > 0u)
                for (uint32_t u = ((inner - 1u) / 4096u) * 4096u;; u -= 4096u) {
                    s.at(-float_of(u));
                    if (u == 0u) break;
                }
            for (uint32_t u = 0u; u < inner; u += 4096u) s.at(float_of(u));
            for (uint32_t u = inner; u <= top; ++u) s.at(float_of(u));
        }
        printf("%d %a %a %a %a %lld %lld\n", p3d_render_interior_taps(H, W, o) ? 1 : 0,
               (double)floorf(p3d_tap_coord(-L, o.coord_scale, half)), (double)floorf(p3d_tap_coord(L, o.coord_scale, half)), (double)s.lo,
               (double)s.hi, s.n, s.bad);
    }
    return 0;
}
