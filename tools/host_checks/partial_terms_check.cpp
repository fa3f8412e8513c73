// partial_terms_check.cpp — two pieces of the matrix-pipe permutation that the kernels share with the host through GL_HD code,
// against 128-bit integer arithmetic mod p:
//   * pmf::recombine_wide + pmf::reduce96_terms (poseidon_mfma.hpp): the S-box input of a round of the running group, i.e. the
//     gemm's eight limbs recombined to a 96-bit integer, the group's earlier y added UNREDUCED with their small integer
//     coefficients, one reduce96. Limbs at 0 and at pmf::LIMB_MAX (the largest limb the join is specified for), y at the edges of the 64-bit range (loose values included), one,
//     two and three terms with every choice of the three coefficients, and 10^5 random cases in the device's own coefficient
//     order. The bounds the code states (top word of the recombined sum below 2^18, of the total below 2^24) are checked too.
//   * poseidon::mds_layer_rows<FIRST, COUNT> (poseidon.hpp) against mds_layer_naive, row by row mod p, for the row sets the
//     kernels use, on states at the extremes of the 64-bit range (loose values included).
// Built and run by tests/test_partial_terms_host.py.
#include <cstdio>
#include <vector>
#include "poseidon.hpp"
#include "poseidon_mfma.hpp"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

static u64 g_seed = 0x5DEECE66Dull;
static u64 rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

// one case: limbs z, n terms y[i] g[i]; returns the number of failed expectations
static int terms_case(const u32 (&z)[pmf::LIMBS], const u64 *y, const u32 *g, int n) {
    u128 want = 0;
    for (int l = 0; l < pmf::LIMBS; l++) want += (u128)z[l] << (8 * l);
    int bad = 0;
    u64 lo; u32 top;
    pmf::recombine_wide(z, lo, top);
    bad += (((u128)top << 64) | lo) != want;                       // the 96-bit sum is the integer itself
    bad += top >= (1u << 18);
    bad += gl::canon(pmf::recombine(z)) != (u64)(want % gl::P);
    for (int i = 0; i < n; i++) want += (u128)y[i] * g[i];
    bad += (want >> 64) >= ((u128)1 << 24);                        // what reduce96 is given stays far below 2^96
    bad += gl::canon(pmf::reduce96_terms(lo, top, y, g, n)) != (u64)(want % gl::P);
    return bad;
}
static int check_terms() {
    const u32 G[3] = {pmf::G0, pmf::G1, pmf::G2};
    const u64 Y[] = {0, 1, gl::P - 1, ~0ull, 0xFFFFFFFFull, 1ull << 63, gl::P, 0xFFFFFFFF00000000ull};
    const int NY = sizeof Y / sizeof Y[0];
    int bad = 0;
    long cases = 0;
    for (int zc = 0; zc < 3; zc++) {
        u32 z[pmf::LIMBS];
        for (int l = 0; l < pmf::LIMBS; l++) z[l] = zc == 0 ? 0 : zc == 1 ? pmf::LIMB_MAX : ((l & 1) ? pmf::LIMB_MAX : 0);
        bad += terms_case(z, nullptr, nullptr, 0); cases++;
        for (int n = 1; n <= pmf::MAX_GROUP_TERMS; n++) {
            int ny = 1, ng = 1;
            for (int i = 0; i < n; i++) { ny *= NY; ng *= 3; }
            for (int cy = 0; cy < ny; cy++)
                for (int cg = 0; cg < ng; cg++) {                  // every y of the list with every coefficient, in every position
                    u64 y[pmf::MAX_GROUP_TERMS]; u32 g[pmf::MAX_GROUP_TERMS];
                    for (int i = 0, a = cy, b = cg; i < n; i++, a /= NY, b /= 3) { y[i] = Y[a % NY]; g[i] = G[b % 3]; }
                    bad += terms_case(z, y, g, n); cases++;
                }
        }
    }
    for (int t = 0; t < 100000; t++) {
        u32 z[pmf::LIMBS], g[pmf::MAX_GROUP_TERMS];
        u64 y[pmf::MAX_GROUP_TERMS];
        for (int l = 0; l < pmf::LIMBS; l++) z[l] = (u32)(rnd() % (pmf::LIMB_MAX + 1ull));
        const int n = (int)(rnd() % 4);                            // the round's place in its group: n earlier y
        for (int i = 0; i < n; i++) {
            y[i] = rnd();
            if (t % 5 == 0) y[i] = ~0ull - (rnd() & 0xFF);
            if (t % 7 == 0) y[i] &= 0xFFFFFFFFull;
            g[i] = G[n - 1 - i];                                   // the device's order (group_step)
        }
        bad += terms_case(z, y, g, n); cases++;
    }
    printf("unreduced group terms (%ld cases): mismatches %d\n", cases, bad);
    return bad;
}

template <int FIRST, int COUNT>
static int rows_case(const u64 (&s)[12]) {
    u64 want[12], got[12];
    for (int i = 0; i < 12; i++) want[i] = got[i] = s[i];
    poseidon::mds_layer_naive(want);
    poseidon::mds_layer_rows<FIRST, COUNT>(got);
    int bad = 0;
    for (int r = FIRST; r < FIRST + COUNT; r++) bad += gl::canon(got[r]) != gl::canon(want[r]);
    return bad;
}
static int check_rows() {
    const u64 E[] = {0, 1, gl::P - 1, ~0ull, 0xFFFFFFFFull, 1ull << 63, 1ull << 32, gl::P, 0xFFFFFFFF00000000ull};
    const int NE = sizeof E / sizeof E[0];
    std::vector<std::vector<u64>> states;
    for (int a = 0; a < NE; a++) {
        states.push_back(std::vector<u64>(12, E[a]));                                  // every lane at one extreme
        for (int b = 0; b < NE; b++) {
            std::vector<u64> v(12);
            for (int i = 0; i < 12; i++) v[i] = (i & 1) ? E[a] : E[b];                 // two extremes alternating
            states.push_back(v);
            for (int i = 0; i < 12; i++) v[i] = i == 0 ? E[a] : E[b];                  // lane 0 (the diagonal term) apart
            states.push_back(v);
        }
    }
    for (int t = 0; t < 20000; t++) {
        std::vector<u64> v(12);
        for (int i = 0; i < 12; i++) { v[i] = rnd(); if (t % 3 == 0 && (rnd() & 1)) v[i] = E[rnd() % NE]; }
        states.push_back(v);
    }
    int bad = 0;
    for (size_t t = 0; t < states.size(); t++) {
        u64 s[12];
        for (int i = 0; i < 12; i++) s[i] = states[t][i];
        bad += rows_case<0, 4>(s) + rows_case<8, 4>(s) + rows_case<7, 1>(s) + rows_case<0, 12>(s);
    }
    printf("row-limited MDS layer (%zu states x 4 row sets): mismatches %d\n", states.size(), bad);
    return bad;
}
int main() { return (check_terms() | check_rows()) != 0; }
