// Host program of tests/test_optim_cpu.py: the chunk plan of the optimiser step (csrc/p3d_optim_plan.hpp) compiled without any device
// code.  argv: the numels of the tensors.  Prints "count N", then one line "chunk TENSOR OFFSET COUNT" per chunk, then the answers of
// optim_aligned16 to pointer sets built from one 64-byte aligned buffer, as "aligned OFFSETS... = FLAG".  Exit status 1 and a line on
// stderr when the plan breaks what k_adam_ema (csrc/p3d_optim.hip) relies on: every element covered exactly once, in order, no chunk
// across a tensor, no empty chunk, chunk starts at multiples of P3D_OPTIM_CHUNK.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "p3d_optim_plan.hpp"

static int fail(const char* what, long long a, long long b) {
    fprintf(stderr, "plan: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    std::vector<int64_t> numels;
    for (int i = 1; i < argc; ++i) numels.push_back(atoll(argv[i]));
    const int n = (int)numels.size();
    const int64_t count = optim_plan(numels.data(), n, nullptr, 0);
    printf("count %lld\n", (long long)count);
    if (count < 0) return 0;
    std::vector<p3d_optim_chunk> plan((size_t)count + 1);
    if (count > 0 && optim_plan(numels.data(), n, plan.data(), count - 1) != P3D_E_WORKSPACE) return fail("a short capacity was accepted", count, 0);
    if (optim_plan(numels.data(), n, plan.data(), count) != count) return fail("the plan does not have the size it announced", count, 0);
    int64_t c = 0;
    for (int t = 0; t < n; ++t) {
        int64_t next = 0;  // the next element of tensor t that needs a chunk
        while (c < count && plan[c].tensor == t) {
            const p3d_optim_chunk& k = plan[c];
            if (k.offset != next) return fail("a gap or an overlap", t, k.offset);
            if (k.offset % P3D_OPTIM_CHUNK) return fail("a chunk start off the grid", t, k.offset);
            if (k.count < 1 || k.count > P3D_OPTIM_CHUNK) return fail("a chunk of a bad size", t, k.count);
            if (k.offset + k.count > numels[t]) return fail("a chunk across the end of its tensor", t, k.offset + k.count);
            next += k.count;
            ++c;
        }
        if (next != numels[t]) return fail("a tensor not covered", t, next);
    }
    if (c != count) return fail("chunks left over or out of order", c, count);
    for (int64_t i = 0; i < count; ++i) printf("chunk %d %lld %d\n", plan[i].tensor, (long long)plan[i].offset, plan[i].count);

    alignas(64) static char buf[256];
    const int sets[][4] = {{0, 16, 32, 48}, {0, 16, 32, 52}, {4, 16, 32, 48}, {0, 8, 32, 48}, {0, 16, 33, 48}, {0, 16, -1, -1}, {0, 12, -1, -1}};
    for (const auto& s : sets) {
        const void* ptrs[4];
        printf("aligned");
        for (int i = 0; i < 4; ++i) {
            ptrs[i] = s[i] < 0 ? nullptr : buf + s[i];  // (-1: a pointer the mode does not use)
            printf(" %d", s[i]);
        }
        printf(" = %d\n", optim_aligned16(ptrs, 4));
    }
    printf("aligned none = %d\n", optim_aligned16(nullptr, 4));
    return 0;
}
