// p3d_optim_plan.hpp — which workgroup of the optimiser step (k_adam_ema, p3d_optim.hip) takes which elements, decided in ONE
// place: the chunk -> (tensor, offset, count) plan and the 16-byte alignment flag of a tensor's pointers.  Host code only (no HIP
// headers): tests/test_optim_cpu.py compiles it into a plain host program.
//   optim_chunk_count   how many chunks a list of numels needs (or a negative P3D_E_*)
//   optim_plan          writes them
//   optim_aligned16     the flag that lets a tensor take the 16-byte path
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/p3d_optim.h"

#define OPTIM_MAX_CHUNKS 0x7fffffffLL  // one chunk per workgroup: the launch's grid.x

static inline int64_t optim_chunks_of(int64_t numel) { return (numel + P3D_OPTIM_CHUNK - 1) / P3D_OPTIM_CHUNK; }

static inline int64_t optim_chunk_count(const int64_t* numels, int n_tensors) {
    if (!numels || n_tensors <= 0) return P3D_E_ARG;
    int64_t n = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numels[t] < 0) return P3D_E_ARG;
        if (numels[t] > OPTIM_MAX_CHUNKS * P3D_OPTIM_CHUNK) return P3D_E_RANGE;  // (before the sum: no overflow below)
        n += optim_chunks_of(numels[t]);
        if (n > OPTIM_MAX_CHUNKS) return P3D_E_RANGE;
    }
    return n;
}

// Tensor by tensor, ascending offsets; every chunk but a tensor's last is full, so every chunk starts at a multiple of
// P3D_OPTIM_CHUNK elements: 16 KiB, which keeps the 16-byte alignment of the tensor's base.
static inline int64_t optim_plan(const int64_t* numels, int n_tensors, p3d_optim_chunk* chunks, int64_t capacity) {
    const int64_t total = optim_chunk_count(numels, n_tensors);
    if (total < 0 || !chunks) return total;
    if (capacity < total) return P3D_E_WORKSPACE;
    int64_t c = 0;
    for (int t = 0; t < n_tensors; ++t)
        for (int64_t off = 0; off < numels[t]; off += P3D_OPTIM_CHUNK) {
            const int64_t left = numels[t] - off;
            chunks[c].offset = off;
            chunks[c].tensor = t;
            chunks[c].count = (int32_t)(left < P3D_OPTIM_CHUNK ? left : P3D_OPTIM_CHUNK);
            ++c;
        }
    return c;
}

static inline int optim_aligned16(const void* const* ptrs, int n) {
    if (!ptrs || n <= 0) return 0;
    uintptr_t bits = 0;
    for (int i = 0; i < n; ++i) bits |= (uintptr_t)ptrs[i];  // (NULL adds nothing)
    return (bits & 15) == 0;
}
