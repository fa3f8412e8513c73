// mul_add_check.cpp — gl::mul_add(a, b, c) = a b + c mod p with one reduction (gl64.hpp) on the host:
//   * the GL_HD function against unsigned __int128 arithmetic mod p, on a, b in {0, 1, 2^32 - 1, 2^32, p - 1} x c in
//     {0, 2^32 - 1, 2^64 - 1} (and, since the function takes any word, the same with p and 2^64 - 1 as factors) and on 10^6
//     seeded random triples;
//   * the device form's schedule in plain 32-bit words (c_lo in the addend of a0 b0, c_hi with that product's high word in the
//     addend of a0 b1, the second cross term's 65th bit as a carry word) against the same 128-bit integer, with the two "cannot
//     wrap" claims of its comment checked at every step.
// A stand-alone program; tests/test_mul_add_host.py builds and runs it (it may also be built with -fsanitize=address,undefined).
#include <cstdio>
#include "gl64.hpp"
using gl::u32;
using gl::u64;
typedef unsigned __int128 u128;

static int g_wrap = 0;      // a step of the limb schedule left the range its comment claims
static void limb_schedule(u64 a, u64 b, u64 c, u64 &lo, u64 &hi) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u128 p00w = (u128)a0 * b0 + (u32)c;
    g_wrap += (p00w >> 64) != 0;
    const u64 p00 = (u64)p00w;
    const u128 mw = (u128)a0 * b1 + (p00 >> 32) + (c >> 32);
    g_wrap += (mw >> 64) != 0;
    const u128 sw = (u128)a1 * b0 + (u64)mw;            // may reach 65 bits: the multiply-add's own carry-out
    const u64 m = (u64)sw, cm = (u64)(sw >> 64);
    const u128 hw = (u128)a1 * b1 + ((cm << 32) | (m >> 32));
    g_wrap += (hw >> 64) != 0;
    hi = (u64)hw;
    lo = (m << 32) | (u32)p00;
}
static int one(u64 a, u64 b, u64 c) {
    const u128 exact = (u128)a * b + c;
    const u64 want = (u64)(exact % gl::P);
    u64 lo, hi;
    limb_schedule(a, b, c, lo, hi);
    int bad = gl::canon(gl::mul_add(a, b, c)) != want;
    bad += lo != (u64)exact || hi != (u64)(exact >> 64);
    gl::mul_add64wide(a, b, c, lo, hi);
    bad += lo != (u64)exact || hi != (u64)(exact >> 64);
    return bad;
}
int main() {
    const u64 F[] = {0, 1, 0xFFFFFFFFull, 1ull << 32, gl::P - 1, gl::P, ~0ull};
    const u64 C[] = {0, 0xFFFFFFFFull, ~0ull, 1, 1ull << 32, gl::P - 1};
    int bad = 0, cases = 0;
    for (u64 a : F) for (u64 b : F) for (u64 c : C) { bad += one(a, b, c); cases++; }
    printf("mul_add extremes (%d triples): mismatches %d\n", cases, bad);
    int bad_r = 0;
    u64 seed = 0xD1B54A32D192ED03ull;
    auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (int t = 0; t < 1000000; t++) {
        u64 a = rnd(), b = rnd(), c = rnd();
        if (t % 5 == 0) { a %= gl::P; b %= gl::P; }
        if (t % 7 == 0) c |= 0xFFFFFFFF00000000ull;
        if (t % 11 == 0) { a |= 0xFFFFFFFFull; b |= 0xFFFFFFFF00000000ull; }
        bad_r += one(a, b, c);
    }
    printf("mul_add random (1000000 triples): mismatches %d\n", bad_r);
    printf("limb schedule range claims: mismatches %d\n", g_wrap);
    return (bad | bad_r | g_wrap) != 0;
}
