// mul_wide_check.cpp — the word-level schedule of the device form of gl::mul64wide (csrc/gl64.hpp) restated in plain uint32_t /
// uint64_t C++, every no-overflow claim of its comment as an assertion, against unsigned __int128; and the whole lazy product
// (mul_lazy's t = lo - hi_hi with its borrow, mul_fold, mul_finish's multiply-add by 2^32 - 1 with its carry fold) against the
// 128-bit product modulo p. Stand-alone, no GPU, meant to be built with -fsanitize=address,undefined (unsigned wrap-around is
// defined behaviour and is used on purpose in the reduction; a signed overflow, a bad shift or a bad index is not).
//
// usage: mul_wide_check [pairs.bin]     pairs.bin: operand pairs as little-endian u64 (a, b), the vectors of
// tests/field_vectors_wide.py. Always adds every combination of extreme 32-bit halves, the boundaries of the cross-term sum and
// 10^7 xorshift pairs. Built and run by tests/test_mul_wide_host.py.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef uint32_t u32;
typedef uint64_t u64;
typedef unsigned __int128 u128;

static const u64 P = 0xFFFFFFFF00000001ull;
static long bad = 0, carries = 0, rares = 0, compared = 0;
#define CLAIM(c) do { if (!(c)) { if (bad < 8) std::printf("CLAIM FAILED line %d: %s  (a %016" PRIx64 " b %016" PRIx64 ")\n", __LINE__, #c, a, b); bad++; } } while (0)

// v_mad_u64_u32: the 64-bit result and the carry-out of a 32 x 32 product plus a 64-bit addend
static u64 mad(u32 x, u32 y, u64 addend, u32 &carry) {
    const u64 prod = (u64)x * y;
    const u64 r = prod + addend;
    carry = r < prod;
    return r;
}

static void wide(u64 a, u64 b, u64 &lo, u64 &hi) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    u32 c;
    const u64 p00 = mad(a0, b0, 0, c);                         // one 64-bit low product
    CLAIM(c == 0);
    const u32 l00 = (u32)p00;
    const u32 h00 = (u32)(p00 >> 32);                          // moved into the low word of the next addend pair
    const u64 p01 = mad(a0, b1, h00, c);
    CLAIM(c == 0);                                             // (2^32-1)^2 + 2^32-2 < 2^64
    u32 cm;
    const u64 m = mad(a1, b0, p01, cm);                        // may carry: the 65th bit of the cross-term sum
    const u128 S = (u128)a1 * b0 + (u128)a0 * b1 + h00;
    CLAIM((u64)S == m && (u32)(S >> 64) == cm);
    CLAIM(cm == 0 || (u32)(m >> 32) <= 0xFFFFFFFDu);           // S <= 2^65 - 3 2^32
    const u64 addend = ((u64)cm << 32) | (u32)(m >> 32);       // S >> 32, a 33-bit value in a register pair
    hi = mad(a1, b1, addend, c);
    CLAIM(c == 0);                                             // hi = floor(a b / 2^64)
    lo = ((u64)(u32)m << 32) | l00;                            // disjoint words
    const u128 prod = (u128)a * b;
    CLAIM(lo == (u64)prod && hi == (u64)(prod >> 64));
    carries += cm;
}

// mul_lazy + mul_fold + mul_finish on top of it
static void product(u64 a, u64 b) {
    u64 lo, hi;
    wide(a, b, lo, hi);
    const u32 hh = (u32)(hi >> 32), hl = (u32)hi;
    u64 t = lo - hh;
    const bool rare = lo < hh;
    if (rare) t -= 0xFFFFFFFFull;                              // mul_fold: the borrow is worth 2^64 = 2^32 - 1
    CLAIM(!rare || t >= (u64)0 - 0xFFFFFFFFull - hh);          // the fold itself cannot borrow again: t + 2^32 - 1 wrapped below 2^64
    u32 c;
    u64 r = mad(hl, 0xFFFFFFFFu, t, c);
    const u64 before = r;
    r += c ? 0xFFFFFFFFull : 0;
    CLAIM(r >= before);                                        // the carry fold cannot wrap
    CLAIM(r % P == (u64)(((u128)a * b) % P));
    rares += rare;
    compared++;
}

static u64 seed = 0x9E3779B97F4A7C15ull;
static u64 rnd() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; }

int main(int argc, char **argv) {
    const u32 H[7] = {0, 1, 2, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (u32 a0 : H) for (u32 a1 : H) for (u32 b0 : H) for (u32 b1 : H) product(((u64)a1 << 32) | a0, ((u64)b1 << 32) | b0);
    std::printf("halves: %ld pairs compared\n", compared);
    const u64 B[5][2] = {{0xFFFFFFFFAAAAAAAAull, 0x2FFFFFFFFull}, {0xFFFFFFFF49249249ull, 0x6FFFFFFFFull}, {0xFFFFFFFF80000000ull, 0x3FFFFFFFFull},
                         {0xFFFFFFFFAAAAAAABull, 0x2FFFFFFFFull}, {~0ull, ~0ull}};
    const long c0 = carries;
    for (auto &p : B) { product(p[0], p[1]); product(p[1], p[0]); }
    std::printf("boundaries: 10 pairs compared, %ld carry\n", carries - c0);
    if (carries - c0 != 6) { std::printf("FAILED: the boundaries 2^64, 2^64 + 1 and the all-ones pair must carry\n"); bad++; }
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
        std::vector<u64> w(1 << 16);
        long n = 0;
        for (size_t got; (got = std::fread(w.data(), 8, w.size(), f)) > 0;) {
            if (got % 2) { std::printf("odd number of words in %s\n", argv[1]); return 2; }
            for (size_t i = 0; i < got; i += 2) product(w[i], w[i + 1]);
            n += (long)(got / 2);
        }
        std::fclose(f);
        std::printf("file: %ld pairs compared\n", n);
    }
    const long c1 = carries;
    const long N = 10000000;
    for (long i = 0; i < N; i++) { const u64 a = rnd(), b = rnd(); product(a, b); }
    std::printf("random: %ld pairs compared, %.2f %% carry\n", N, 100.0 * (double)(carries - c1) / (double)N);
    if ((carries - c1) * 20 < N || (carries - c1) * 10 > N) { std::printf("FAILED: share of carries outside 5 %% .. 10 %%\n"); bad++; }
    std::printf("mul wide: failures %ld (%ld pairs, %ld rare borrows)\n", bad, compared, rares);
    return bad ? 1 : 0;
}
