// Host program of tests/test_importance_split_cpu.py: the schedules of csrc/p3d_importance.hpp compiled without any device code
// and proved by the 0-1 principle — a network of comparators sorts every input if it sorts every input of zeros and ones.  The
// keys are machine words that carry 64 such inputs at once (min = AND, max = OR, negation = NOT).
//   sort24     p3d_sort_network<24> on all 2^24 inputs
//   passes H   every merge pass of p3d_sort_network<H> (H = 24, 48) on every pair of sorted 0-1 blocks it has to merge
//   cross H    cross-half exchange + p3d_valley_merge<H> on every pair of sorted 0-1 halves, (H + 1)^2 cases
//   floats H   half sorts + exchange + merges on random and tie-heavy floats against std::sort, bit for bit
//   merge      p3d_merge_bits_half against a plain stable two-list merge on random and tie-heavy lists, word for word
// Prints "<name> <cases>" per check; exit status 1 and a line on stderr for a failure.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "p3d_importance.hpp"

struct BitKey {
    static uint64_t mn(uint64_t a, uint64_t b) { return a & b; }
    static uint64_t mx(uint64_t a, uint64_t b) { return a | b; }
    static uint64_t neg(uint64_t a) { return ~a; }
};

static int fails = 0;
static void fail(const char* what, long long c) {
    if (fails++ < 10) fprintf(stderr, "FAIL %s case %lld\n", what, c);
}

template <int N>
static bool sorted01(const uint64_t (&a)[N], int from, int to, uint64_t lanes) {
    uint64_t bad = 0;
    for (int i = from; i + 1 < to; ++i) bad |= a[i] & ~a[i + 1];
    return (bad & lanes) == 0;
}

static long long sort24_all() {
    static const uint64_t pat[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull, 0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    for (uint32_t base = 0; base < (1u << 18); ++base) {  // input number = base * 64 + lane; key i = bit i of it
        uint64_t a[24];
        for (int i = 0; i < 6; ++i) a[i] = pat[i];
        for (int i = 6; i < 24; ++i) a[i] = ((base >> (i - 6)) & 1u) ? ~0ull : 0ull;
        uint64_t ones = 0;  // (parity of the ones of every input, as a cheap check that no value is lost)
        for (int i = 0; i < 24; ++i) ones ^= a[i];
        p3d_sort_network<24, BitKey>(a);
        uint64_t after = 0;
        for (int i = 0; i < 24; ++i) after ^= a[i];
        if (!sorted01(a, 0, 24, ~0ull) || after != ones) fail("sort24", base);
    }
    return 1ll << 24;
}

// every pass pp of the H-key network: blocks [b, b + 2pp) cut at H; all sorted 0-1 contents of the two lists of each block
template <int H>
static long long passes() {
    long long cases = 0;
    for (int pp = 1; pp < p3d_pow2_ceil(H); pp <<= 1) {
        for (int b = 0; b < H; b += 2 * pp) {
            const int n1 = std::min(pp, H - b), n2 = std::max(0, std::min(pp, H - b - pp));
            for (int z1 = 0; z1 <= n1; ++z1)
                for (int z2 = 0; z2 <= n2; ++z2) {
                    uint64_t a[H];
                    for (int i = 0; i < H; ++i) a[i] = 0x5DEECE66Dull * (i + 1);  // other blocks: anything
                    for (int i = 0; i < n1; ++i) a[b + i] = i < z1 ? 0ull : ~0ull;
                    for (int i = 0; i < n2; ++i) a[b + pp + i] = i < z2 ? 0ull : ~0ull;
                    p3d_sort_merge_pass<H, BitKey>(a, pp);
                    bool ok = sorted01(a, b, b + n1 + n2, ~0ull);
                    int zeros = 0;
                    for (int i = 0; i < n1 + n2; ++i) zeros += a[b + i] == 0ull;
                    if (!ok || zeros != z1 + z2) fail("passes", pp * 1000000ll + b * 10000 + z1 * 100 + z2);
                    ++cases;
                }
        }
    }
    return cases;
}

// what the two halves of a wave do with their sorted keys, on any key type: lo ascending, hi ascending on its negation
template <int H, typename K, typename T>
static void split_merge(T (&lo)[H], T (&hi_neg)[H], T (&column)[2 * H]) {
    for (int i = 0; i < H; ++i) {
        T a, b;
        p3d_cross_half_exchange<K>(lo[i], hi_neg[i], a, b);
        lo[i] = a;
        hi_neg[i] = b;
    }
    p3d_valley_merge<H, K>(lo);
    p3d_valley_merge<H, K>(hi_neg);
    for (int i = 0; i < H; ++i) {
        column[p3d_half_rank(H, 0, i)] = K::neg(lo[i]);
        column[p3d_half_rank(H, 1, i)] = hi_neg[i];
    }
}

template <int H>
static long long cross() {
    long long cases = 0;
    for (int za = 0; za <= H; ++za)
        for (int zb = 0; zb <= H; ++zb) {
            uint64_t lo[H], hi[H], col[2 * H];
            for (int i = 0; i < H; ++i) lo[i] = i < za ? 0ull : ~0ull;                 // A ascending
            for (int i = 0; i < H; ++i) hi[i] = ~((H - 1 - i) < zb ? 0ull : ~0ull);    // -B[H-1-i]
            split_merge<H, BitKey>(lo, hi, col);
            int zeros = 0;
            for (int i = 0; i < 2 * H; ++i) zeros += col[i] == 0ull;
            if (!sorted01(col, 0, 2 * H, ~0ull) || zeros != za + zb) fail("cross", za * 1000 + zb);
            ++cases;
        }
    return cases;
}

template <int H>
static long long floats(int rounds) {
    std::mt19937 rng(1234 + H);
    std::uniform_real_distribution<float> u(2.25f, 3.3f);
    for (int r = 0; r < rounds; ++r) {
        float key[2 * H], lo[H], hi[H], col[2 * H];
        for (int i = 0; i < 2 * H; ++i) key[i] = u(rng);
        if (r & 1) for (int i = 0; i < 2 * H; ++i) key[i] = key[rng() % (1 + r % 7)];  // tie-heavy: a handful of distinct values
        for (int i = 0; i < H; ++i) { lo[i] = key[i]; hi[i] = -key[H + i]; }
        p3d_sort_network<H>(lo);
        p3d_sort_network<H>(hi);
        split_merge<H, P3dFloatKey>(lo, hi, col);
        std::sort(key, key + 2 * H);
        if (memcmp(key, col, sizeof(key)) != 0) fail("floats", r);
    }
    return rounds;
}

static long long merge(int rounds) {
    std::mt19937 rng(99);
    long long cases = 0;
    const int shapes[][2] = {{48, 48}, {96, 96}, {48, 0}, {12, 12}, {47, 48}, {48, 64}, {96, 33}, {5, 128}, {128, 128}, {1, 1}};
    for (const auto& sh : shapes)
        for (int r = 0; r < rounds; ++r) {
            const int Sc = sh[0], Sf = sh[1], S = Sc + Sf, nw = (S + 31) >> 5;
            std::vector<float> c(Sc), f(Sf);
            const int mode = r % 4;  // 0 random, 1 fine drawn FROM the coarse values (equal depths), 2 few distinct values, 3 disjoint ranges
            std::uniform_real_distribution<float> u(0.0f, 1.0f);
            for (auto& x : c) x = mode == 2 ? (float)(rng() % 5) : u(rng);
            for (auto& x : f) x = mode == 1 ? c[rng() % Sc] : (mode == 2 ? (float)(rng() % 5) : (mode == 3 ? 2.0f + u(rng) : u(rng)));
            if (mode == 3 && (r & 4)) for (auto& x : c) x += 4.0f;
            std::sort(c.begin(), c.end());
            std::sort(f.begin(), f.end());
            std::vector<uint8_t> kc(Sc), kf(Sf);
            for (auto& x : kc) x = rng() & 1;
            for (auto& x : kf) x = (rng() & 3) == 0;
            // the plain stable merge: coarse first on ties
            std::vector<uint32_t> sl(nw, 0u), kn(nw, 0u), sl2(nw, 0u), kn2(nw, 0u);
            for (int q = 0, ci = 0, fi = 0; q < S; ++q) {
                const bool take_c = ci < Sc && (fi >= Sf || c[ci] <= f[fi]);
                if (take_c) sl[q >> 5] |= 1u << (q & 31);
                if (take_c ? kc[ci] : kf[fi]) kn[q >> 5] |= 1u << (q & 31);
                take_c ? ++ci : ++fi;
            }
            for (int h = 0; h < 2; ++h)
                p3d_merge_bits_half([&](bool cc, int i) { return cc ? c.at(i) : f.at(i); },
                                    [&](bool cc, int i, float t) { return (cc ? c.at(i) : f.at(i)) == t && (cc ? kc[i] : kf[i]) != 0; },
                                    [&](int w, uint32_t kw, uint32_t sw) { kn2.at(w) |= kw; sl2.at(w) |= sw; }, Sc, Sf, h);
            if (sl != sl2 || kn != kn2) fail("merge", Sc * 1000000ll + Sf * 1000 + r);
            ++cases;
        }
    return cases;
}

int main() {
    printf("sort24 %lld\n", sort24_all());
    printf("passes24 %lld\n", passes<24>());
    printf("passes48 %lld\n", passes<48>());
    printf("cross24 %lld\n", cross<24>());
    printf("cross48 %lld\n", cross<48>());
    printf("floats24 %lld\n", floats<24>(20000));
    printf("floats48 %lld\n", floats<48>(20000));
    printf("merge %lld\n", merge(4000));
    return fails ? 1 : 0;
}
