// The per-ray importance work of k_render that the two halves of a wave share out between them: the sorting-network
// schedules and the split of the merge pre-pass.  In k_render a lane is (ray j = lane & 31) x (half h = lane >> 5); the
// halves serve the decode (each owns half of the hidden channels), so anything per ray would run twice with equal results.
// Here half h owns half of it:
//
//   draws       half h makes the inverse-CDF draws [h * Sf/2, (h + 1) * Sf/2);
//   sort        each half sorts its Sf/2 keys in registers (p3d_sort_network), half 1 on the NEGATED keys, i.e. descending;
//               one cross-half exchange (p3d_cross_half_exchange: key i of half 0 against key i of half 1) leaves the Sf/2
//               smallest keys in half 0 and the Sf/2 largest in half 1, each as a sequence that falls and then rises
//               (half 0 holds its keys negated for that); p3d_valley_merge sorts such a sequence.  Half 1 ends with rank
//               Sf/2 + i in register i, half 0 with MINUS rank Sf/2 - 1 - i (p3d_half_rank / the sign are applied by the store);
//   merge       the stable merge of the coarse and the fine column is cut at merged position S/2 (p3d_merge_split finds how many
//               coarse samples lie in front of the cut); half h walks [h * S/2, ...) and the bit words are OR-ed across halves.
//               Or, without the serial walk (p3d_merge_ranks_half): half h finds the merged positions of half of the coarse
//               ranks, each by a search in the sorted fine column, eight searches in flight.
//
// The networks only move values (min / max of finite floats; a negation is exact), so the sorted column — and with it every
// result — is the one any correct sort gives.  The schedules are templates over the key type and its operations, so a host
// program can run the very schedules on 0-1 inputs, 64 of them per machine word (tests/importance_split_host.cpp); the block at
// the end (under __HIPCC__) holds the pieces that need the lanes of a wave and is device only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define P3D_IMP_FN __host__ __device__ __forceinline__
#define P3D_IMP_UNROLL _Pragma("unroll")
#else
#define P3D_IMP_FN inline
#define P3D_IMP_UNROLL
#endif

// keys on the device: finite floats
struct P3dFloatKey {
    P3D_IMP_FN static float mn(float a, float b) { return __builtin_fminf(a, b); }
    P3D_IMP_FN static float mx(float a, float b) { return __builtin_fmaxf(a, b); }
    P3D_IMP_FN static float neg(float a) { return -a; }
};

P3D_IMP_FN constexpr int p3d_pow2_ceil(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// In-register sort of a ray's NR keys: Batcher's odd-even merge sort on N = the next power of two with keys NR..N-1 = +inf:
// a comparator writes min to the lower and max to the upper index, so one whose upper index is >= NR never changes anything
// and is simply not emitted (NR = 48: 543 -> 384 comparators, NR = 96: 1471 -> 1056, NR = 24: 191 -> 132).
// (one pass of it, p3d_sort_merge_pass<NR>(a, pp), merges every pair of neighbouring sorted blocks of pp keys: the unit the host
// test proves on all sorted 0-1 blocks)
template <int NR, typename K = P3dFloatKey, typename T>
P3D_IMP_FN void p3d_sort_merge_pass(T (&a)[NR], int pp) {
    constexpr int N = p3d_pow2_ceil(NR);
P3D_IMP_UNROLL
    for (int k = pp; k >= 1; k >>= 1) {
P3D_IMP_UNROLL
        for (int jj = k % pp; jj + k < N; jj += 2 * k) {
P3D_IMP_UNROLL
            for (int i = 0; i < k; ++i) {
                if (i + jj + k < NR && (i + jj) / (2 * pp) == (i + jj + k) / (2 * pp)) {
                    T x = a[i + jj], y = a[i + jj + k];
                    a[i + jj] = K::mn(x, y);
                    a[i + jj + k] = K::mx(x, y);
                }
            }
        }
    }
}
template <int NR, typename K = P3dFloatKey, typename T>
P3D_IMP_FN void p3d_sort_network(T (&a)[NR]) {
P3D_IMP_UNROLL
    for (int pp = 1; pp < p3d_pow2_ceil(NR); pp <<= 1) p3d_sort_merge_pass<NR, K>(a, pp);
}

// The cross-half exchange on ONE key index, written on the two halves' values: half 0 holds lo = A[i] of its ascending keys,
// half 1 holds hi_neg = -B[H-1-i] (its keys sorted on their negation).  Half 0 keeps the minimum — negated — and half 1 the
// maximum.  (-min(a, b) = max(-a, -b): the device gets both results from v_max_f32 with source modifiers.)
template <typename K = P3dFloatKey, typename T>
P3D_IMP_FN void p3d_cross_half_exchange(T lo, T hi_neg, T& lo_out_neg, T& hi_out) {
    lo_out_neg = K::mx(K::neg(lo), hi_neg);
    hi_out = K::mx(lo, K::neg(hi_neg));
}

// Ascending sort of H keys that fall and then rise (either part may be empty): the bitonic merge network on N = the next power
// of two with keys H..N-1 = +inf — the padded sequence still falls and then rises — and, as above, no comparator whose upper
// index is >= H (H = 24: 52 comparators, H = 48: 128).
template <int H, typename K = P3dFloatKey, typename T>
P3D_IMP_FN void p3d_valley_merge(T (&a)[H]) {
    constexpr int N = p3d_pow2_ceil(H);
P3D_IMP_UNROLL
    for (int k = N / 2; k >= 1; k >>= 1) {
P3D_IMP_UNROLL
        for (int i = 0; i < H; ++i) {
            if ((i & k) == 0 && i + k < H) {
                T x = a[i], y = a[i + k];
                a[i] = K::mn(x, y);
                a[i + k] = K::mx(x, y);
            }
        }
    }
}

// sorted rank (0 .. 2H-1) of the key that register i of half h holds after p3d_valley_merge; half 0 holds it negated
P3D_IMP_FN constexpr int p3d_half_rank(int H, int h, int i) { return h ? H + i : H - 1 - i; }

// The cut of the stable merge (ties: coarse first) of a sorted coarse column and a sorted fine column at merged position D:
// the number of coarse samples among the first D merged ones.  rd(true, x) reads coarse rank x, rd(false, k) fine rank k.
// Coarse x lies at merged position x + #{k : fine(k) < coarse(x)}, which grows with x; it is >= D exactly when D - x <= 0, or
// D - x <= Sf and fine(D - x - 1) < coarse(x).  The answer is the first x in [max(0, D - Sf), min(D, Sc)] for which that holds
// (min(D, Sc) if none): a binary search of `steps` rounds (p3d_merge_split_steps), two column reads per round.
P3D_IMP_FN int p3d_merge_split_steps(int Sc, int Sf) {
    int n = Sc < Sf ? Sc : Sf, s = 0;  // the interval holds at most min(Sc, Sf) + 1 candidates
    while (n > 0) { ++s; n >>= 1; }
    return s;
}
template <typename RD>
P3D_IMP_FN int p3d_merge_split(RD rd, int Sc, int Sf, int D, int steps) {
    int lo = D - Sf > 0 ? D - Sf : 0, hi = D < Sc ? D : Sc;  // the answer is in [lo, hi]
    for (int s = 0; s < steps; ++s) {
        const int mid = (lo + hi) >> 1;  // lo < hi: mid < hi, so coarse `mid` and fine D - mid - 1 exist (clamped for closed intervals)
        const int cm = mid < Sc - 1 ? mid : Sc - 1, fm = D - mid - 1 < 0 ? 0 : (D - mid - 1 < Sf ? D - mid - 1 : Sf - 1);
        const bool behind = rd(false, fm) < rd(true, cm);  // coarse `mid` lies at or behind the cut
        const bool open = lo < hi;
        hi = (open && behind) ? mid : hi;
        lo = (open && !behind) ? mid + 1 : lo;
    }
    return lo;
}

// Half h's share of the merge pre-pass: the merged positions [h ? S/2 : 0, h ? S : S/2) of the stable merge, S = Sc + Sf.  For
// each it decides whether the sample is the head of the coarse list (bit in sw) and whether known(is_coarse, index, depth) says
// its density needs no decode (bit in kw), and hands every 32-bit word it touched to put(word, kw, sw) — the word that holds the
// cut gets a part from each half, so put has to OR.  Both halves run S - S/2 steps (the wave's loop is uniform); with S odd
// half 0's last step is idle.
template <typename RD, typename KN, typename PUT>
P3D_IMP_FN void p3d_merge_bits_half(RD rd, KN known, PUT put, int Sc, int Sf, int h) {
    const int S = Sc + Sf, D = S >> 1, qb = h ? D : 0, qe = h ? S : D;
    int ci = p3d_merge_split(rd, Sc, Sf, qb, p3d_merge_split_steps(Sc, Sf)), fi = qb - ci;
    const float inf = __builtin_inff();
    float ta = rd(true, ci < Sc ? ci : Sc - 1), tb = Sf > 0 ? rd(false, fi < Sf ? fi : Sf - 1) : inf;
    unsigned kw = 0u, sw = 0u;
    for (int it = 0; it < S - D; ++it) {
        const int q = qb + it;
        const bool mine = q < qe;
        const bool take_c = (ci < Sc) && (fi >= Sf || ta <= tb);
        const bool kn = known(take_c, take_c ? ci : fi, take_c ? ta : tb);
        kw |= (mine && kn) ? (1u << (q & 31)) : 0u;
        sw |= (mine && take_c) ? (1u << (q & 31)) : 0u;
        // pop the head of the coarse or of the fine list: ONE read at a selected address and two selects (a store through a
        // selected pointer parks ta / tb in scratch memory)
        ci += take_c ? 1 : 0;
        fi += take_c ? 0 : 1;
        const int cq = ci < Sc ? ci : Sc - 1, fq = fi < Sf ? fi : (Sf > 0 ? Sf - 1 : 0);
        const float nv = rd(take_c, take_c ? cq : fq);
        ta = take_c ? nv : ta;
        tb = take_c ? tb : nv;
        if (mine && ((q & 31) == 31 || q == qe - 1)) {
            put(q >> 5, kw, sw);
            kw = 0u; sw = 0u;
        }
    }
}

// The merge pre-pass by RANK SEARCH (the counterpart of p3d_merge_bits_half): coarse rank i lands at merged position
// i + #{fine < t_i} (ties: coarse first), and the count comes from a binary search in the sorted fine column fine(k), eight ranks in
// flight — the searches of a batch do not depend on one another, where every step of the serial merge waits for the read before
// it.  NF is the capacity of the fine column (Sf <= NF): the search runs the steps 2^r .. 1, 2^r the largest power of two <= NF
// (NF = 48: six rounds, 96: seven, 0: none), and a bit row over the merged list is NW words (Sc + Sf <= 32 * NW).
// -DP3D_MERGE_RANKS=0 keeps every kernel that has a coarse column on the serial merge (the A/B of DESIGN.md section 6).
#ifndef P3D_MERGE_RANKS
#define P3D_MERGE_RANKS 1
#endif
P3D_IMP_FN constexpr int p3d_rank_first_step(int NF) { return p3d_pow2_ceil(NF + 1) >> 1; }
// Half h's share: the coarse ranks [h * Sch, (h + 1) * Sch), Sch = Sc / 2 rounded up to whole batches of eight.  tc_sorted(i): the
// coarse depth of sorted rank i; known(i, t): coarse rank i at depth t needs no decode (asked for ranks up to 2 * Sch - 1; the answer
// for a rank >= Sc is dropped).  Out, in registers: the bits of ITS ranks in the is-coarse row slw and in the known row knw; the two
// halves' rows OR-ed are the whole is-coarse row and the coarse samples' part of the known row.  And, for the fine samples' part where
// their crop bits are two runs (P3dFineRuns): fine rank k sits at merged position k + #{coarse i : pos_i <= k} (coarse i lies in front
// of it unless fine k < t_i, that is unless k < pos_i), so the half also counts its ranks in front of the fine ranks fr.k1 and fr.k2.
struct P3dFineRuns {
    int k1, k2;  // in: the fine ranks [0, k1) and [k2, Sf) are cropped, the ranks between them are not
    int n1, n2;  // out: the half's coarse ranks in front of fine rank k1 / of fine rank k2 (the two halves' counts add up)
};
template <int NF, int NW, typename TCS, typename FINE, typename KN>
P3D_IMP_FN void p3d_merge_ranks_half(TCS tc_sorted, FINE fine, KN known, uint32_t (&slw)[NW], uint32_t (&knw)[NW], P3dFineRuns& fr, int Sc, int Sf,
                                     int h) {
P3D_IMP_UNROLL
    for (int w = 0; w < NW; ++w) { slw[w] = 0u; knw[w] = 0u; }
    fr.n1 = 0; fr.n2 = 0;
    const int Sch = ((Sc + 15) >> 4) << 3, ib = h * Sch;
    for (int i0 = 0; i0 < Sch; i0 += 8) {
        float tv[8];
        int pos[8];
P3D_IMP_UNROLL
        for (int q = 0; q < 8; ++q) { tv[q] = tc_sorted(ib + i0 + q < Sc ? ib + i0 + q : Sc - 1); pos[q] = 0; }
P3D_IMP_UNROLL
        for (int step = p3d_rank_first_step(NF); step >= 1; step >>= 1) {
            float c[8];
P3D_IMP_UNROLL
            for (int q = 0; q < 8; ++q) c[q] = fine((pos[q] + step <= Sf) ? pos[q] + step - 1 : 0);
P3D_IMP_UNROLL
            for (int q = 0; q < 8; ++q) pos[q] = ((pos[q] + step <= Sf) && (c[q] < tv[q])) ? pos[q] + step : pos[q];
        }
P3D_IMP_UNROLL
        for (int q = 0; q < 8; ++q) {
            const int i = ib + i0 + q;
            const bool kn = known(i, tv[q]);
            const int P = i + pos[q], pw = (i < Sc) ? (P >> 5) : -1;  // (a rank past the end sets no bit)
            const uint32_t b = 1u << (P & 31);
P3D_IMP_UNROLL
            for (int w = 0; w < NW; ++w) {
                slw[w] |= (pw == w) ? b : 0u;
                knw[w] |= (pw == w && kn) ? b : 0u;
            }
            fr.n1 += (i < Sc && pos[q] <= fr.k1) ? 1 : 0;
            fr.n2 += (i < Sc && pos[q] <= fr.k2) ? 1 : 0;
        }
    }
}
// The fine samples' crop bits fw (bit k: sorted fine sample k is cropped; at most 64 of them) as two runs, one at each end of the
// column: k1, k2 as in P3dFineRuns; false if the bits are anything else.  A crop by position along a ray gives such runs wherever the
// uncropped part of the ray is one stretch — the kernel does not rely on it: it asks, and deposits bit by bit otherwise.
template <int NFW>
P3D_IMP_FN bool p3d_fine_runs(const uint32_t (&fw)[NFW], int Sf, int& k1, int& k2) {
    static_assert(NFW <= 2, "the bits in one 64-bit word");
    const uint64_t F = (uint64_t)fw[0] | (NFW > 1 ? (uint64_t)fw[NFW - 1] << 32 : 0ull);
    const uint64_t all = Sf >= 64 ? ~0ull : ((1ull << Sf) - 1ull);
    if ((F & all) == all) { k1 = Sf; k2 = Sf; return (F & ~all) == 0ull; }  // every fine sample (Sf = 0: none there is)
    k1 = __builtin_ctzll(~F);                       // F has a zero below bit Sf
    const uint64_t top = ~(F << (64 - Sf)) ;        // bit 63: fine rank Sf - 1, zeros shifted in below
    const int tail = __builtin_clzll(top);          // top != 0: that zero again
    k2 = Sf - tail;
    return __builtin_popcountll(F) == k1 + tail;
}
// The fine samples' part of the known row from the runs: fine rank k1 sits at merged position P1 = k1 + (coarse ranks in front of it)
// and k2 at P2 likewise (a rank Sf: at S); the fine samples in front of P1 and from P2 on are the cropped ones.
template <int NW>
P3D_IMP_FN void p3d_deposit_fine_runs(const uint32_t (&slw)[NW], uint32_t (&knw)[NW], int P1, int P2, int S) {
P3D_IMP_UNROLL
    for (int w = 0; w < NW; ++w) {
        const int lo = 32 * w;
        const uint32_t below1 = P1 >= lo + 32 ? ~0u : (P1 <= lo ? 0u : (1u << (P1 - lo)) - 1u);  // merged positions < P1
        const uint32_t below2 = P2 >= lo + 32 ? ~0u : (P2 <= lo ? 0u : (1u << (P2 - lo)) - 1u);
        const uint32_t inlist = S >= lo + 32 ? ~0u : (S <= lo ? 0u : (1u << (S - lo)) - 1u);
        knw[w] |= ~slw[w] & (below1 | ~below2) & inlist;
    }
}
// ... and the fine samples' part of the known row: sorted fine sample k sits at the k-th zero of the (whole) is-coarse row, and bit
// k of the words fw says that it is cropped.  Walks the S merged positions and ORs the bits into knw.
template <int NW, int NFW>
P3D_IMP_FN void p3d_deposit_fine_bits(const uint32_t (&slw)[NW], uint32_t (&knw)[NW], const uint32_t (&fw)[NFW], int S) {
    int fk = 0;
P3D_IMP_UNROLL
    for (int w = 0; w < NW; ++w) {
        if (w * 32 < S) {  // wave-uniform
            uint32_t kk = 0u;
            for (int b = 0; b < 32; ++b) {
                const bool isf = !((slw[w] >> b) & 1u) && (w * 32 + b < S);
                uint32_t fwv = fw[NFW - 1];
P3D_IMP_UNROLL
                for (int x = NFW - 2; x >= 0; --x) fwv = (fk < 32 * (x + 1)) ? fw[x] : fwv;
                kk |= (isf && ((fwv >> (fk & 31)) & 1u)) ? (1u << b) : 0u;
                fk += isf ? 1 : 0;
            }
            knw[w] |= kk;
        }
    }
}

#if defined(__HIPCC__)
// ---- device only: the pieces of the split that need the lanes of a wave
// The sort of the split (see the top of this file): in, half h's H = Sf/2 draws; out, half 1 holds rank H + i in register i,
// half 0 MINUS rank H - 1 - i (p3d_half_rank).
template <int H>
__device__ __forceinline__ void p3d_sort_halves(float (&tf)[H], int h) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const uint32_t neg1 = h ? 0x80000000u : 0u;  // the sign bit in half 1
P3D_IMP_UNROLL
    for (int i = 0; i < H; ++i) tf[i] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, tf[i]) ^ neg1);  // half 1 sorts descending
    p3d_sort_network<H>(tf);
P3D_IMP_UNROLL
    for (int i = 0; i < H; i += 2) {
        // v_permlane32_swap: afterwards lanes 0-31 hold key i of both halves (x: half 0's, y: half 1's), lanes 32-63 key i + 1;
        // the second swap hands half 0 its (negated) minima and half 1 its maxima back, for both keys
        u32x2 in = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, tf[i]), __builtin_bit_cast(uint32_t, tf[i + 1]), false, false);
        const uint32_t in0 = in.x, in1 = in.y;  // (scalars first: a bit cast of a vector ELEMENT reads element 0)
        float mn_neg, mx;
        p3d_cross_half_exchange(__builtin_bit_cast(float, in0), __builtin_bit_cast(float, in1), mn_neg, mx);
        u32x2 out = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, mn_neg), __builtin_bit_cast(uint32_t, mx), false, false);
        const uint32_t out0 = out.x, out1 = out.y;
        tf[i] = __builtin_bit_cast(float, out0);
        tf[i + 1] = __builtin_bit_cast(float, out1);
    }
    p3d_valley_merge<H>(tf);
}

// k_render's TCG instantiations keep no coarse-depth column: raw(i) recomputes coarse depth i in DRAW order.  This is the coarse
// depth of sorted RANK i (what the stable sort of renderer.py:289-301 puts there): the draw-order value itself unless the wave
// saw a reversed pair (wave_unsorted) — then the neighbour that rounding swapped in, or (wave_bad: jitter outside [0, 1), never from
// torch.rand_like) the rank-i element of the row by counting, O(Sc^2) reads per access: slow, exact, reached by no renderer.py call.
template <typename RAW>
__device__ __forceinline__ float p3d_coarse_rank(RAW raw, int i, int Sc, bool wave_unsorted, bool wave_bad) {
    float a = raw(i);
    if (wave_unsorted) {  // wave-uniform
        if (!wave_bad) {
            const float lo = i > 0 ? raw(i - 1) : -__builtin_inff(), hi = i < Sc - 1 ? raw(i + 1) : __builtin_inff();
            a = lo > a ? lo : (a > hi ? hi : a);
        } else {
            for (int c = 0; c < Sc; ++c) {
                const float tv = raw(c);
                int r = 0;
                for (int x = 0; x < Sc; ++x) {
                    const float tx = raw(x);
                    r += (tx < tv || (tx == tv && x < c)) ? 1 : 0;
                }
                a = (r == i) ? tv : a;
            }
        }
    }
    return a;
}

// The whole pre-pass by rank search (above) on a wave: half h searches its ranks, the two halves' rows are OR-ed with one lane
// exchange per word, the fine samples' crop bits fw (NFW words over the sorted fine column) are deposited — skipped where no ray of
// the wave has one; from their two runs where every ray's bits are runs, bit by bit otherwise — and every word of the two rows is
// handed to put(word, kw, sw) once: nothing to zero, no OR in memory.  k_render's TCG instantiations (no coarse column: tc_sorted
// recomputes the depth) and, with a column in LDS, its 48-key kernel.
template <int NF, int NW, int NFW, typename TCS, typename FINE, typename KN, typename PUT>
__device__ __forceinline__ void p3d_merge_bits_ranks(TCS tc_sorted, FINE fine, KN known, PUT put, const uint32_t (&fw)[NFW], int Sc, int Sf, int h) {
    const int S = Sc + Sf, nmw = (S + 31) >> 5;
    uint32_t slw[NW], knw[NW];
    P3dFineRuns fr = {0, 0, 0, 0};
    bool runs = false;  // every ray of the wave has its cropped fine samples in two runs (asked where the bits fit 64: the 48-key kernel)
    if constexpr (NFW <= 2) runs = __builtin_amdgcn_ballot_w64(!p3d_fine_runs(fw, Sf, fr.k1, fr.k2)) == 0;
    p3d_merge_ranks_half<NF, NW>(tc_sorted, fine, known, slw, knw, fr, Sc, Sf, h);
P3D_IMP_UNROLL
    for (int w = 0; w < NW; ++w) { slw[w] |= __shfl_xor(slw[w], 32); knw[w] |= __shfl_xor(knw[w], 32); }  // the other half's ranks
    uint32_t any = 0u;
P3D_IMP_UNROLL
    for (int x = 0; x < NFW; ++x) any |= fw[x];
    if (__builtin_amdgcn_ballot_w64(any != 0u) != 0) {
        if (runs) p3d_deposit_fine_runs(slw, knw, fr.k1 + fr.n1 + __shfl_xor(fr.n1, 32), fr.k2 + fr.n2 + __shfl_xor(fr.n2, 32), S);
        else p3d_deposit_fine_bits(slw, knw, fw, S);
    }
P3D_IMP_UNROLL
    for (int w = 0; w < NW; ++w)
        if (w < nmw) put(w, knw[w], slw[w]);
}

// ---- the draw rows of a ray (jitter [Sc], u [Sf]) as 16-byte loads, and the stratified depths shared out
// A ray's row is contiguous and, where the launch says so (RenderParams::wide_rows, p3d_render_plan.hpp), every piece of four
// floats a half takes is 16-byte aligned.  The first `pieces` (wave-uniform, <= MAXP) pieces of `row`, all in flight together:
template <int MAXP>
__device__ __forceinline__ void p3d_load_row_pieces(const float* row, int pieces, f32x4 (&out)[MAXP]) {
P3D_IMP_UNROLL
    for (int q = 0; q < MAXP; ++q)
        if (q < pieces) out[q] = *(const f32x4*)(row + 4 * q);
}
// ... and N floats (whole pieces) of it into a register row
template <int N>
__device__ __forceinline__ void p3d_load_row_wide(const float* row, float (&out)[N]) {
    static_assert(N % 4 == 0, "whole 16-byte pieces");
P3D_IMP_UNROLL
    for (int q = 0; q < N / 4; ++q) {
        const f32x4 v = *(const f32x4*)(row + 4 * q);
        out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
    }
}
// Half h has made the stratified depths [h * Sc/2, (h + 1) * Sc/2) in index order: first / last are the ends of its run, unsorted
// says whether two neighbours INSIDE it are out of order, tcmin / tcmax are its extrema.  One exchange gives both halves the ray's:
// the comparison across the cut, t[Sc/2] < t[Sc/2 - 1], joins the flag, and min / max are order-free, hence exact.
__device__ __forceinline__ void p3d_stratified_combine(int h, float first, float last, bool& unsorted, float& tcmin, float& tcmax) {
    const float other = __shfl_xor(h ? first : last, 32);  // half 0: t[Sc/2]; half 1: t[Sc/2 - 1]
    const int uo = __shfl_xor((int)unsorted, 32);
    const float mn = __shfl_xor(tcmin, 32), mx = __shfl_xor(tcmax, 32);
    unsorted = unsorted || uo != 0 || (h ? first < other : other < last);
    tcmin = __builtin_fminf(tcmin, mn);
    tcmax = __builtin_fmaxf(tcmax, mx);
}
#endif
