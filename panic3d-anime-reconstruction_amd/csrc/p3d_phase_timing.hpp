// Per-section clock accounting inside k_render: a measurement build only (-DP3D_PHASE_TIMING, tools/phase_timing.py).
// Without the switch every macro below expands to nothing, so the product's code is what it is without this header.
//
// With it, each wave stamps s_memtime (one tick = one shader cycle) at the section borders named below and adds the
// difference to a per-wave accumulator; lane 0 adds the accumulators to g_p3d_phase with one atomicAdd per section when the
// wave ends.  p3d_phase_read() (exported only by this build) copies the totals out.  A stamp waits for its own result only,
// so a section is charged the ISSUE time of its instructions plus whatever it waited for itself; the stamps cost ~10 % of a
// wave's cycles, which is why the table gives shares and not milliseconds.
//
// Each wave also leaves one record of its own in g_p3d_wave (slot = blockIdx.x * waves per block + wave, the launches of at
// most P3D_WAVE_RECORDS waves): the device-wide real-time counter (s_memrealtime: 100 MHz, one clock for all XCDs, unlike the
// per-XCD shader clock) when it started and when it ended, its block index and the XCD it really ran on (HW_REG_XCC_ID).
// p3d_phase_read_waves() copies them out; tools/phase_timing.py --xcd prints when the last wave of each XCD ended.
#pragma once

#ifdef P3D_PHASE_TIMING
enum P3dPhase {
    P3D_PH_WEIGHTS = 0,  // weights -> LDS, workgroup barrier, tile index
    P3D_PH_STRAT,        // ray set-up + stratified depths
    P3D_PH_COARSE,       // coarse loop (decodes included)
    P3D_PH_CDF,          // pdf row + the two binary64 accumulations
    P3D_PH_DRAWS,        // u loads + inverse-CDF draws
    P3D_PH_SORT,         // sorting network + the stores of the sorted column (+ TCG crop bits)
    P3D_PH_MERGE,        // merge pre-pass (bit rows)
    P3D_PH_SELECT,       // final loop: select / skip walk
    P3D_PH_DECODE,       // final loop: gather + MLP
    P3D_PH_MARCH,        // final loop: march, guards, composite
    P3D_PH_OUT,          // outputs + min / max reduction
    P3D_PH_WAVES,        // waves that ran
    P3D_PH_LIFE,         // first to last stamp of a wave
    P3D_PH_N
};
__device__ unsigned long long g_p3d_phase[P3D_PH_N];
#define P3D_WAVE_RECORDS 65536
struct P3dWaveRecord { unsigned long long t0, t1; unsigned block, xcc; };
__device__ P3dWaveRecord g_p3d_wave[P3D_WAVE_RECORDS];

struct P3dPhaseClock {
    unsigned long long first, last, real0, acc[P3D_PH_N];
    __device__ __forceinline__ static unsigned long long now() {
        unsigned long long t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
        return t;
    }
    __device__ __forceinline__ static unsigned long long real_now() {
        unsigned long long t;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
        return t;
    }
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int q = 0; q < P3D_PH_N; ++q) acc[q] = 0ull;
        real0 = real_now();
        first = last = now();
    }
    __device__ __forceinline__ void mark(int slot) {
        const unsigned long long t = now();
        acc[slot] += t - last;
        last = t;
    }
    __device__ __forceinline__ void flush() {
        acc[P3D_PH_WAVES] = 1ull;
        acc[P3D_PH_LIFE] = last - first;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < P3D_PH_N; ++q) atomicAdd(&g_p3d_phase[q], acc[q]);
            const unsigned long long slot = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
            if (slot < P3D_WAVE_RECORDS) {
                unsigned xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
                P3dWaveRecord r;
                r.t0 = real0; r.t1 = real_now(); r.block = blockIdx.x; r.xcc = xcc;
                g_p3d_wave[slot] = r;
            }
        }
    }
};
#define P3D_PHASE_START() P3dPhaseClock p3d_phase_clock; p3d_phase_clock.start()
#define P3D_PHASE(slot) p3d_phase_clock.mark(slot)
#define P3D_PHASE_FLUSH() p3d_phase_clock.flush()
#else
#define P3D_PHASE_START() ((void)0)
#define P3D_PHASE(slot) ((void)0)
#define P3D_PHASE_FLUSH() ((void)0)
#endif
