// mds_words_check.cpp — two pieces of the matrix-pipe permutation's full rounds that the kernels share with the host through GL_HD
// code, against the reference forms:
//   * poseidon::mds_layer_rows_words<FIRST, COUNT> (poseidon.hpp: one wrapping 64-bit transform and one 32-bit transform of the
//     top 23 bits) against mds_layer_naive, row by row mod p, for the whole layer and the row sets <0,4>, <8,4>, <7,1>, <0,12>:
//     each of 0, 1, p-1, 2^32-1, 2^32, 2^64-1 (and the values around 2^41, where the top transform cuts) in every lane position
//     against every background, and 10^5 seeded random states; every row is also held against the 128-bit integer sum
//     mod p.
//   * poseidon::mds_layer_words_rc (the same layer with the constants of the following round folded into both transforms' outputs)
//     against mds_layer_naive followed by a modular addition, with constants at the extremes of the 64-bit range.
// Built and run by tests/test_mds_words_host.py.
#include <cstdio>
#include <vector>
#include "poseidon.hpp"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

static u64 g_seed = 0x2545F4914F6CDD1Dull;
static u64 rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static u64 row_mod_p(const u64 (&s)[12], int r) {
    constexpr u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    u128 v = 0;
    for (int i = 0; i < 12; i++) v += (u128)s[(i + r) % 12] * C[i];
    if (r == 0) v += (u128)s[0] * 8;
    return (u64)(v % gl::P);
}
template <int FIRST, int COUNT>
static int rows_case(const u64 (&s)[12]) {
    u64 want[12], got[12];
    for (int i = 0; i < 12; i++) want[i] = got[i] = s[i];
    poseidon::mds_layer_naive(want);
    poseidon::mds_layer_rows_words<FIRST, COUNT>(got);
    int bad = 0;
    for (int r = FIRST; r < FIRST + COUNT; r++) bad += gl::canon(got[r]) != gl::canon(want[r]) || gl::canon(got[r]) != row_mod_p(s, r);
    return bad;
}
static int all_row_sets(const u64 (&s)[12]) {
    u64 whole[12], want[12];
    for (int i = 0; i < 12; i++) whole[i] = want[i] = s[i];
    poseidon::mds_layer_words(whole);
    poseidon::mds_layer_naive(want);
    int bad = 0;
    for (int i = 0; i < 12; i++) bad += gl::canon(whole[i]) != gl::canon(want[i]);
    return bad + rows_case<0, 4>(s) + rows_case<8, 4>(s) + rows_case<7, 1>(s) + rows_case<0, 12>(s);
}
static int check_rows() {
    const u64 E[] = {0, 1, gl::P - 1, 0xFFFFFFFFull, 1ull << 32, ~0ull, gl::P, (1ull << 41) - 1, 1ull << 41, ~0ull << 41, 1ull << 63};
    const int NE = sizeof E / sizeof E[0];
    int bad = 0;
    long cases = 0;
    for (int a = 0; a < NE; a++)
        for (int b = 0; b < NE; b++)
            for (int pos = 0; pos < 12; pos++) {          // extreme a in lane `pos`, extreme b everywhere else
                u64 s[12];
                for (int i = 0; i < 12; i++) s[i] = i == pos ? E[a] : E[b];
                bad += all_row_sets(s); cases++;
                for (int i = 0; i < 12; i++) s[i] = ((i + pos) & 1) ? E[a] : E[b];
                bad += all_row_sets(s); cases++;
            }
    for (int t = 0; t < 100000; t++) {
        u64 s[12];
        for (int i = 0; i < 12; i++) {
            s[i] = rnd();
            if (t % 3 == 0 && (rnd() & 1)) s[i] = E[rnd() % NE];
            if (t % 5 == 0) s[i] |= (1ull << 41) - 1;     // the largest fractions below the cut
            if (t % 7 == 0) s[i] = ~0ull - (rnd() & 0xFF);
        }
        bad += all_row_sets(s); cases++;
    }
    printf("word-form MDS layer (%ld states x 5 row sets): mismatches %d\n", cases, bad);
    return bad;
}

// the layer with the constants of the following round folded in, against the reference layer and a modular addition
static int check_rc() {
    const u64 *rc = poseidon::host_hash_round_constants();
    const u64 E[] = {0, 1, gl::P - 1, ~0ull, 0xFFFFFFFFull, 1ull << 32, (1ull << 41) - 1, ~0ull << 41};
    int bad = 0;
    const int N = 100000;
    for (int t = 0; t < N; t++) {
        u64 a[12], b[12], c[12];
        for (int i = 0; i < 12; i++) {
            a[i] = rnd();
            if (t % 3 == 0) a[i] = E[rnd() % 8];
            if (t % 5 == 0) a[i] |= (1ull << 41) - 1;
            b[i] = a[i];
            c[i] = t % 4 == 0 ? E[rnd() % 8] : t % 4 == 1 ? rnd() : rc[(t % 30) * 12 + i];     // extremes, any word, a real round's constants
        }
        poseidon::mds_layer_naive(a);
        poseidon::mds_layer_words_rc(b, c);
        for (int i = 0; i < 12; i++) bad += gl::canon(b[i]) != gl::canon(gl::add(a[i], c[i]));
    }
    printf("word-form MDS layer with the next round's constants (%d states): mismatches %d\n", N, bad);
    return bad;
}
int main() { return (check_rows() | check_rc()) != 0; }
