// digits_check.cpp — the carry-free digits of the matrix-pipe permutation (poseidon_mfma.hpp) on the host, through the GL_HD code
// and the table builder the kernels use:
//   * pmf::to_digits(v): the eight signed base-256 digits sum to the INTEGER v - DIGIT_BIAS, every digit in [-128, 127], for 0, 1,
//     0x7F..7F, 0x80..80, 0x80..80 - 1, p - 1, p, 2^64 - 1 and 10^5 seeded random v (so no wrap and no representative: the
//     tables' additive constants carry the bias, host::fold_digit_bias).
//   * the upload-time self-checks (host_selfcheck, host_selfcheck_gate, host_selfcheck_p2) pass on tables built that way.
//   * emu_permute (the integer emulation of the device schedule, limb range checked) equals poseidon::permute on states made of
//     those edge values: each one in every lane against each other one as background, and all lanes equal.
// A stand-alone program; tests/test_mx_digits_host.py builds and runs it (it may also be built with -fsanitize=address,undefined).
#include <cstdio>
#include <vector>
#include "poseidon.hpp"
#include "poseidon_mfma.hpp"
using gl::u64;

static const u64 EDGE[] = {0, 1, 0x7F7F7F7F7F7F7F7Full, 0x8080808080808080ull, 0x8080808080808080ull - 1, gl::P - 1, gl::P, ~0ull};
static const int NE = sizeof EDGE / sizeof EDGE[0];

static int digit_case(u64 v) {
    const u64 t = pmf::to_digits(v);
    __int128 sum = 0;
    int bad = 0;
    for (int b = 7; b >= 0; b--) {
        const int d = (signed char)(t >> (8 * b));
        bad += d < -128 || d > 127 || d != (int)((v >> (8 * b)) & 0xFF) - 128;
        sum = sum * 256 + d;
    }
    return bad + (sum != (__int128)v - (__int128)pmf::DIGIT_BIAS);
}
static int check_digits() {
    int bad = 0;
    for (u64 v : EDGE) bad += digit_case(v);
    u64 seed = 0x9E3779B97F4A7C15ull;
    for (int t = 0; t < 100000; t++) { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; bad += digit_case(seed); }
    printf("carry-free digits (8 edge values, 100000 random): mismatches %d\n", bad);
    return bad;
}
static int check_selfchecks() {
    const u64 *rc = poseidon::host_hash_round_constants(), *rcp = poseidon::host_round_constants();
    const poseidon2::Params &p2 = poseidon2::qp_params();
    std::vector<unsigned char> tab(pmf::TABLE_BYTES);
    int bad = 0;
    bad += !(pmf::build_tables(rc, tab.data()) && pmf::host_selfcheck(rc, tab.data()));
    bad += !(pmf::build_tables_gate(rcp, tab.data()) && pmf::host_selfcheck_gate(rcp, tab.data()));
    bad += !(pmf::build_tables_p2(p2, tab.data()) && pmf::host_selfcheck_p2(p2, tab.data()));
    printf("table self-checks (Poseidon, gate, Poseidon2): mismatches %d\n", bad);
    return bad;
}
static int permute_case(const u64 (&s)[12], const u64 *rc, const unsigned char *tab) {
    u64 a[12], b[12];
    for (int i = 0; i < 12; i++) a[i] = b[i] = s[i];
    poseidon::permute(a, rc);
    if (!pmf::host::emu_permute(b, rc, tab)) return 12;
    int bad = 0;
    for (int i = 0; i < 12; i++) bad += a[i] != b[i];
    return bad;
}
static int check_permutation() {
    const u64 *rc = poseidon::host_hash_round_constants();
    std::vector<unsigned char> tab(pmf::TABLE_BYTES);
    if (!pmf::build_tables(rc, tab.data())) { printf("emulated permutation: table construction failed\n"); return 1; }
    int bad = 0, cases = 0;
    for (int a = 0; a < NE; a++)
        for (int b = 0; b < NE; b++)
            for (int pos = 0; pos < 12; pos++) {
                u64 s[12];
                for (int i = 0; i < 12; i++) s[i] = i == pos ? EDGE[a] : EDGE[b];
                bad += permute_case(s, rc, tab.data()); cases++;
            }
    printf("emulated permutation on edge states (%d states): mismatches %d\n", cases, bad);
    return bad;
}
int main() { return (check_digits() | check_selfchecks() | check_permutation()) != 0; }
