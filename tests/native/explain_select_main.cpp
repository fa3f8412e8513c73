// explain_select_main.cpp — csrc/explain_select.hpp stand-alone: the ordered selection of the first set bits of a device-written
// bitmap (the rows and cells qpgpu_circuit_explain_witness reports) and the fixed constants of its detection pass, against a
// bit-by-bit reference. Built with -fsanitize=address,undefined by tests/test_witness_explain_host.py: every bitmap is a heap block
// of exactly bitmap_words(nbits) words, so a read or write past it is caught.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "explain_select.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static uint64_t state = 0x243F6A8885A308D3ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

static void one_case(uint64_t nbits, unsigned density_shift, size_t max, bool dirty_tail) {
    const size_t words = explain::bitmap_words(nbits);
    uint32_t *bm = (uint32_t *)std::calloc(words ? words : 1, 4);
    std::vector<uint64_t> want;
    for (uint64_t i = 0; i < nbits; i++)
        if ((rnd() >> 11) % (1u << density_shift) == 0) { bm[i >> 5] |= 1u << (i & 31); want.push_back(i); }
    if (dirty_tail && (nbits & 31)) bm[words - 1] |= ~0u << (nbits & 31);          // bits past nbits: ignored, not trusted to be clear
    uint64_t *out = max ? (uint64_t *)std::malloc(max * 8) : nullptr;
    uint64_t total = ~0ull;
    const size_t got = explain::select_first(bm, nbits, max, out, &total);
    CHECK(total == want.size());
    CHECK(got == (want.size() < max ? want.size() : max));
    for (size_t i = 0; i < got; i++) CHECK(out[i] == want[i]);
    CHECK(explain::select_first(bm, nbits, max, out, nullptr) == got);              // the total is optional
    std::free(out); std::free(bm);
}

int main() {
    CHECK(explain::bitmap_words(0) == 0 && explain::bitmap_words(1) == 1 && explain::bitmap_words(32) == 1 && explain::bitmap_words(33) == 2);
    const uint64_t sizes[] = {0, 1, 31, 32, 33, 63, 64, 65, 128, 1000, 4096, 128 * 80, 8192 * 80 + 7};
    for (uint64_t nbits : sizes)
        for (unsigned dens : {0u, 1u, 5u, 12u})                                     // every bit, half, 1/32, nearly none
            for (size_t max : {(size_t)0, (size_t)1, (size_t)2, (size_t)64, (size_t)1024, (size_t)1 << 20})
                for (int dirty = 0; dirty < 2; dirty++) one_case(nbits, dens, max, dirty != 0);
    std::printf("select ok\n");
    {   // an empty and a full bitmap
        std::vector<uint32_t> bm(4, 0);
        uint64_t out[4], total = 7;
        CHECK(explain::select_first(bm.data(), 128, 4, out, &total) == 0 && total == 0);
        for (auto &w : bm) w = ~0u;
        CHECK(explain::select_first(bm.data(), 100, 4, out, &total) == 4 && total == 100 && out[0] == 0 && out[3] == 3);
    }
    std::printf("edges ok\n");
    {   // the detection constants: fixed, distinct per column, field elements other than 0 and 1
        const uint64_t P = 0xFFFFFFFF00000001ull;
        uint64_t c[4];
        for (uint32_t k = 0; k < 4; k++) { c[k] = explain::detect_constant(k); CHECK(c[k] > 1 && c[k] < P && c[k] == explain::detect_constant(k)); }
        CHECK(c[0] != c[1] && c[0] != c[2] && c[0] != c[3] && c[1] != c[2] && c[1] != c[3] && c[2] != c[3]);
        uint64_t s = explain::DETECT_SEED;
        CHECK(explain::splitmix64(s) % P == c[0]);
    }
    std::printf("constants ok\n");
    std::printf("explain select: %s\n", failures ? "FAILED" : "ok");
    return failures != 0;
}
