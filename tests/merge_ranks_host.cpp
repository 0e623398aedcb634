// Host program of tests/test_merge_ranks_cpu.py: the merge pre-pass by rank search (p3d_merge_ranks_half + p3d_deposit_fine_bits,
// csrc/p3d_importance.hpp) compiled without any device code and compared, word for word, with the serial merge of the same header
// (p3d_merge_bits_half, both halves OR-ed) and with a plain stable two-list merge (ties: coarse first).  Both bit rows: is-coarse
// (sl) and known (kn: a coarse sample's bit by its rank, a fine sample's "cropped" bit by its rank in the fine column).
//   random     the shapes the kernels run (48+48, 96+96, 32+48, 64+48, 48+0) on random, tie-heavy and disjoint lists
//   small      EVERY pair of sorted lists of up to 5 + 5 depths over four values: every interleaving, every tie, runs of equal
//              depths on both sides; every fine sample cropped, none, and a random choice
//   boundary   on every shape, for every (i0, k): i0 coarse samples, then k fine ones, then the rest of the coarse list, then the
//              rest of the fine list — every merged position is taken by a coarse and by a fine sample, the ends of the 32-bit
//              words included ("bits": the least number of cases that put a coarse, and a fine, sample on position 31, 32, 63 or 64)
// The fine samples' bits are deposited from their two runs where they are two runs (p3d_fine_runs, p3d_deposit_fine_runs: what a crop
// by position gives) — then also bit by bit, and the two must agree — and bit by bit otherwise ("deposit_runs" / "deposit_bits" count).
// Prints "<name> <cases>" per check; exit status 1 and a line on stderr for a failure.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "p3d_importance.hpp"

static int fails = 0;
static void fail(const char* what, long long c) {
    if (fails++ < 10) fprintf(stderr, "FAIL %s case %lld\n", what, c);
}

typedef std::vector<float> Col;
typedef std::vector<uint8_t> Bits;
typedef std::vector<uint32_t> Row;

static void plain_rows(const Col& c, const Col& f, const Bits& kc, const Bits& kf, Row& sl, Row& kn) {
    const int Sc = (int)c.size(), Sf = (int)f.size(), S = Sc + Sf;
    for (int q = 0, ci = 0, fi = 0; q < S; ++q) {
        const bool take_c = ci < Sc && (fi >= Sf || c[ci] <= f[fi]);
        if (take_c) sl[q >> 5] |= 1u << (q & 31);
        if (take_c ? kc[ci] : kf[fi]) kn[q >> 5] |= 1u << (q & 31);
        take_c ? ++ci : ++fi;
    }
}

static void serial_rows(const Col& c, const Col& f, const Bits& kc, const Bits& kf, Row& sl, Row& kn) {
    const int Sc = (int)c.size(), Sf = (int)f.size();
    for (int h = 0; h < 2; ++h)
        p3d_merge_bits_half([&](bool cc, int i) { return cc ? c.at(i) : f.at(i); },
                            [&](bool cc, int i, float t) { return (cc ? c.at(i) : f.at(i)) == t && (cc ? kc.at(i) : kf.at(i)) != 0; },
                            [&](int w, uint32_t kw, uint32_t sw) { kn.at(w) |= kw; sl.at(w) |= sw; }, Sc, Sf, h);
}

static long long runs_cases = 0, bits_cases = 0;  // cases whose fine bits were deposited from their runs / bit by bit
// what a wave does: each half its ranks, the rows OR-ed, the fine bits deposited
template <int NF, int NW>
static void rank_rows(const Col& c, const Col& f, const Bits& kc, const Bits& kf, Row& sl, Row& kn) {
    const int Sc = (int)c.size(), Sf = (int)f.size(), S = Sc + Sf;
    constexpr int NFW = NF > 0 ? (NF + 31) / 32 : 1;
    uint32_t slw[NW], knw[NW], fw[NFW];
    for (int w = 0; w < NW; ++w) slw[w] = knw[w] = 0u;
    for (int x = 0; x < NFW; ++x) fw[x] = 0u;
    for (int k = 0; k < Sf; ++k) fw[k >> 5] |= kf[k] ? 1u << (k & 31) : 0u;
    P3dFineRuns fr = {0, 0, 0, 0};
    bool runs = false;
    if constexpr (NFW <= 2) runs = p3d_fine_runs(fw, Sf, fr.k1, fr.k2);
    int n1 = 0, n2 = 0;
    for (int h = 0; h < 2; ++h) {
        uint32_t s1[NW], k1[NW];
        p3d_merge_ranks_half<NF, NW>([&](int i) { return c.at(i); }, [&](int k) { return Sf > 0 ? f.at(k) : 0.0f; },  // (Sf = 0 under a capacity NF > 0: the searches read rank 0 and drop it)
                                     [&](int i, float t) { return i < Sc && c.at(i) == t && kc.at(i) != 0; }, s1, k1, fr, Sc, Sf, h);
        for (int w = 0; w < NW; ++w) { slw[w] |= s1[w]; knw[w] |= k1[w]; }
        n1 += fr.n1; n2 += fr.n2;
    }
    // the fine samples' bits: from their two runs where they are runs (and then both ways, which must agree), bit by bit otherwise
    bool is_runs = true;
    for (int k = 0; k < Sf; ++k) is_runs = is_runs && (kf[k] != 0) == (k < fr.k1 || k >= fr.k2);
    if (NFW <= 2 && runs != is_runs) fail("p3d_fine_runs", Sf);
    if (runs) {
        uint32_t kr[NW];
        for (int w = 0; w < NW; ++w) kr[w] = knw[w];
        p3d_deposit_fine_runs(slw, kr, fr.k1 + n1, fr.k2 + n2, S);
        p3d_deposit_fine_bits(slw, knw, fw, S);
        for (int w = 0; w < NW; ++w) if (kr[w] != knw[w]) fail("runs against bits", w);
        ++runs_cases;
    } else {
        p3d_deposit_fine_bits(slw, knw, fw, S);
        ++bits_cases;
    }
    for (int w = 0; w < NW; ++w) {
        if (w < (int)sl.size()) { sl[w] = slw[w]; kn[w] = knw[w]; }
        else if (slw[w] | knw[w]) fail("bits past the list", w);
    }
}

template <int NF, int NW>
static bool check(const Col& c, const Col& f, const Bits& kc, const Bits& kf, Row* is_coarse = nullptr) {
    const int nw = ((int)(c.size() + f.size()) + 31) >> 5;
    Row sl0(nw, 0u), kn0(nw, 0u), sl1(nw, 0u), kn1(nw, 0u), sl2(nw, 0u), kn2(nw, 0u);
    plain_rows(c, f, kc, kf, sl0, kn0);
    serial_rows(c, f, kc, kf, sl1, kn1);
    rank_rows<NF, NW>(c, f, kc, kf, sl2, kn2);
    if (is_coarse) *is_coarse = sl0;
    return sl1 == sl2 && kn1 == kn2 && sl0 == sl2 && kn0 == kn2;
}

template <int NF, int NW>
static long long random_shape(int Sc, int Sf, int rounds, std::mt19937& rng) {
    for (int r = 0; r < rounds; ++r) {
        Col c(Sc), f(Sf);
        const int mode = r % 4;  // 0 random, 1 fine drawn FROM the coarse values (equal depths), 2 few distinct values, 3 disjoint ranges
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        for (auto& x : c) x = mode == 2 ? (float)(rng() % 5) : u(rng);
        for (auto& x : f) x = mode == 1 ? c[rng() % Sc] : (mode == 2 ? (float)(rng() % 5) : (mode == 3 ? 2.0f + u(rng) : u(rng)));
        if (mode == 3 && (r & 4)) for (auto& x : c) x += 4.0f;  // all fine in front of all coarse (else the reverse)
        std::sort(c.begin(), c.end());
        std::sort(f.begin(), f.end());
        Bits kc(Sc), kf(Sf);
        for (auto& x : kc) x = rng() & 1;
        const int km = (r / 4) % 4;  // fine crop bits: a random quarter, all, none, a run at each end (either may be empty)
        for (auto& x : kf) x = km == 0 ? (rng() & 3) == 0 : km == 1;
        if (km == 3 && Sf > 0) {
            const int a = rng() % (Sf + 1), b = rng() % (Sf + 1);
            for (int k = 0; k < Sf; ++k) kf[k] = k < a || k >= Sf - b;
        }
        if (!check<NF, NW>(c, f, kc, kf)) fail("random", Sc * 1000000ll + Sf * 1000 + r);
    }
    return rounds;
}

// every sorted list of n depths over the values 0 .. 3, appended to out
static void sorted_lists(int n, std::vector<Col>& out) {
    Col cur;
    struct R {
        static void go(int n, int from, Col& cur, std::vector<Col>& out) {
            if ((int)cur.size() == n) { out.push_back(cur); return; }
            for (int v = from; v < 4; ++v) { cur.push_back((float)v); go(n, v, cur, out); cur.pop_back(); }
        }
    };
    R::go(n, 0, cur, out);
}

static long long small(std::mt19937& rng) {
    std::vector<Col> cs, fs;
    for (int n = 1; n <= 5; ++n) sorted_lists(n, cs);
    for (int n = 0; n <= 5; ++n) sorted_lists(n, fs);
    long long cases = 0;
    for (const Col& c : cs)
        for (const Col& f : fs)
            for (int km = 0; km < 3; ++km) {
                Bits kc(c.size()), kf(f.size());
                for (auto& x : kc) x = rng() & 1;
                for (auto& x : kf) x = km == 0 ? rng() & 1 : km == 1;
                if (!check<8, 1>(c, f, kc, kf)) fail("small", cases);
                ++cases;
            }
    return cases;
}

static long long edge_coarse[4] = {0, 0, 0, 0}, edge_fine[4] = {0, 0, 0, 0};  // cases with a coarse / a fine sample at merged position 31, 32, 63, 64
template <int NF, int NW>
static long long boundary(int Sc, int Sf, std::mt19937& rng) {
    long long cases = 0;
    for (int i0 = 0; i0 <= Sc; ++i0)
        for (int k = 0; k <= Sf; ++k) {
            Col c(Sc), f(Sf);
            for (int i = 0; i < Sc; ++i) c[i] = i < i0 ? 1.0f : 3.0f;
            for (int x = 0; x < Sf; ++x) f[x] = x < k ? 2.0f : 4.0f;
            Bits kc(Sc), kf(Sf);
            for (auto& x : kc) x = rng() & 1;
            const int a = Sf > 0 ? rng() % (Sf + 1) : 0, bb = Sf > 0 ? rng() % (Sf + 1) : 0;
            for (int x = 0; x < Sf; ++x) kf[x] = ((i0 + k) & 1) ? (rng() & 1) : (x < a || x >= Sf - bb);  // every other case: runs
            Row sl;
            if (!check<NF, NW>(c, f, kc, kf, &sl)) fail("boundary", Sc * 100000000ll + Sf * 1000000ll + i0 * 1000 + k);
            const int ends[4] = {31, 32, 63, 64};
            for (int e = 0; e < 4; ++e)
                if (ends[e] < Sc + Sf) ++(((sl[ends[e] >> 5] >> (ends[e] & 31)) & 1u) ? edge_coarse : edge_fine)[e];
            ++cases;
        }
    return cases;
}

int main() {
    std::mt19937 rng(2024);
    long long r = 0, b = 0;
    r += random_shape<48, 3>(48, 48, 3000, rng);
    r += random_shape<96, 6>(96, 96, 3000, rng);
    r += random_shape<48, 3>(32, 48, 3000, rng);
    r += random_shape<48, 4>(64, 48, 3000, rng);
    r += random_shape<0, 2>(48, 0, 3000, rng);
    printf("random %lld\n", r);
    printf("small %lld\n", small(rng));
    b += boundary<48, 3>(48, 48, rng);
    b += boundary<96, 6>(96, 96, rng);
    b += boundary<48, 3>(32, 48, rng);
    b += boundary<48, 4>(64, 48, rng);
    b += boundary<0, 2>(48, 0, rng);
    printf("boundary %lld\n", b);
    long long least = edge_coarse[0];
    for (int e = 0; e < 4; ++e) least = std::min(least, std::min(edge_coarse[e], edge_fine[e]));
    printf("bits %lld\n", least);
    printf("deposit_runs %lld\n", runs_cases);
    printf("deposit_bits %lld\n", bits_cases);
    return fails ? 1 : 0;
}
