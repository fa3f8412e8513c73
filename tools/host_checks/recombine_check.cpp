// recombine_check.cpp — the 8-instruction limb join of the matrix-pipe permutation (poseidon_mfma.hpp: pmf::recombine_wide) on the
// host, through the GL_HD code and the table builder the kernels use:
//   * recombine_wide(z) against the unsigned __int128 sum of z[l] 2^(8 l), and recombine(z) against that value mod p: every limb
//     at each of 0, 1, 2^23, 13 107 455 (the most a 9-step chain can reach) and 16 711 935 (pmf::LIMB_MAX, the most the join is
//     specified for) in every one of the 8 positions (5^8 vectors), and 10^6 seeded random vectors of limbs up to LIMB_MAX.
//   * the worst-case limb of every chain of the three tables (Poseidon, the Poseidon gate, Poseidon2), derived from the table
//     bytes (pmf::host::table_limb_max: start + 128 sum |a| per row), stays within LIMB_MAX.
//   * the three upload-time self-checks pass, and emu_permute (the integer emulation of the device schedule, every limb checked
//     against LIMB_MAX) equals poseidon::permute on 2 000 states that include 0, 1, p - 1, 2^64 - 1 and the byte edges.
// A stand-alone program; tests/test_mx_recombine_host.py builds and runs it (it may also be built with -fsanitize=address,undefined).
#include <cstdio>
#include <vector>
#include "poseidon.hpp"
#include "poseidon_mfma.hpp"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

static u64 g_seed = 0x9E3779B97F4A7C15ull;
static u64 rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

static int join_case(const u32 (&z)[pmf::LIMBS]) {
    u128 want = 0;
    for (int l = 0; l < pmf::LIMBS; l++) want += (u128)z[l] << (8 * l);
    u64 lo; u32 top;
    pmf::recombine_wide(z, lo, top);
    int bad = 0;
    bad += (((u128)top << 64) | lo) != want;
    bad += top >= (1u << 18);
    bad += gl::canon(pmf::recombine(z)) != (u64)(want % gl::P);
    return bad;
}
static int check_join() {
    const u32 V[5] = {0, 1, 1u << 23, 13107455u, pmf::LIMB_MAX};
    int bad = 0;
    long grid = 0;
    for (int c = 0; c < 390625; c++, grid++) {                      // 5^8: every value in every position
        u32 z[pmf::LIMBS];
        for (int l = 0, a = c; l < pmf::LIMBS; l++, a /= 5) z[l] = V[a % 5];
        bad += join_case(z);
    }
    const int N = 1000000;
    for (int t = 0; t < N; t++) {
        u32 z[pmf::LIMBS];
        for (int l = 0; l < pmf::LIMBS; l++) z[l] = (u32)(rnd() % (pmf::LIMB_MAX + 1ull));
        bad += join_case(z);
    }
    printf("limb join (%ld grid vectors, %d random): mismatches %d\n", grid, N, bad);
    return bad;
}

struct Tables {
    std::vector<unsigned char> pos, gate, p2;
    bool ok;
    Tables() : pos(pmf::TABLE_BYTES), gate(pmf::TABLE_BYTES), p2(pmf::TABLE_BYTES) {
        ok = pmf::build_tables(poseidon::host_hash_round_constants(), pos.data());
        ok = pmf::build_tables_gate(poseidon::host_round_constants(), gate.data()) && ok;
        ok = pmf::build_tables_p2(poseidon2::qp_params(), p2.data()) && ok;
    }
};
static int check_limb_bound(const Tables &t) {
    if (!t.ok) { printf("table limb bound: table construction failed: mismatches 1\n"); return 1; }
    const u64 m[3] = {pmf::host::table_limb_max(t.pos.data()), pmf::host::table_limb_max(t.gate.data()), pmf::host::table_limb_max(t.p2.data())};
    int bad = 0;
    for (int i = 0; i < 3; i++) bad += m[i] > pmf::LIMB_MAX || m[i] < (1u << 23);
    printf("table-derived worst-case limb (Poseidon %llu, gate %llu, Poseidon2 %llu; bound %u): mismatches %d\n",
           (unsigned long long)m[0], (unsigned long long)m[1], (unsigned long long)m[2], pmf::LIMB_MAX, bad);
    return bad;
}
static int check_permutation(const Tables &t) {
    if (!t.ok) { printf("self-checks and emulated permutation: table construction failed: mismatches 1\n"); return 1; }
    const u64 *rc = poseidon::host_hash_round_constants(), *rcp = poseidon::host_round_constants();
    int bad = 0;
    bad += !pmf::host_selfcheck(rc, t.pos.data());
    bad += !pmf::host_selfcheck_gate(rcp, t.gate.data());
    bad += !pmf::host_selfcheck_p2(poseidon2::qp_params(), t.p2.data());
    const u64 EDGE[] = {0, 1, gl::P - 1, ~0ull, 0x7F7F7F7F7F7F7F7Full, 0x8080808080808080ull, 0x8080808080808080ull - 1, gl::P};
    const int NE = sizeof EDGE / sizeof EDGE[0], N = 2000;
    for (int c = 0; c < N; c++) {
        u64 a[12], b[12];
        for (int i = 0; i < 12; i++) {
            u64 v = rnd();
            if (c < NE) v = EDGE[c];                                           // every lane at one edge
            else if (c < NE + 12 * NE) v = i == (c - NE) % 12 ? EDGE[(c - NE) / 12] : v;   // one edge in one lane, random elsewhere
            else if (c % 3 == 0 && (rnd() & 1)) v = EDGE[rnd() % NE];          // edges mixed in
            a[i] = b[i] = v;
        }
        poseidon::permute(a, rc);
        if (!pmf::host::emu_permute(b, rc, t.pos.data())) { bad += 12; continue; }
        for (int i = 0; i < 12; i++) bad += a[i] != b[i];
    }
    printf("three table self-checks and the emulated permutation (%d states): mismatches %d\n", N, bad);
    return bad;
}
int main() {
    const Tables t;
    return (check_join() | check_limb_bound(t) | check_permutation(t)) != 0;
}
