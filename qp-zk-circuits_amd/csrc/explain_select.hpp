// explain_select.hpp — the ordered selection qpgpu_circuit_explain_witness makes from a device-written bitmap: the indices of
// the first `max` set bits among the first `nbits`, ascending, and the number of set bits among them all. Bit i lives in word
// i / 32 at position i % 32 (what explain_bitmap_kernel and explain_copy_kernel set with atomicOr). Plain host C++ without a
// HIP call, so that a stand-alone program drives it under the sanitizers (tests/native/explain_select_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace explain {

inline size_t bitmap_words(uint64_t nbits) { return (size_t)((nbits + 31) / 32); }

// out[0 .. returned) = the smallest set bit indices below nbits, at most `max` of them (out may be NULL when max is 0); *total =
// how many bits below nbits are set. Bits at or above nbits in the last word are ignored, not trusted to be clear.
inline size_t select_first(const uint32_t *bitmap, uint64_t nbits, size_t max, uint64_t *out, uint64_t *total) {
    size_t taken = 0;
    uint64_t count = 0;
    const size_t words = bitmap_words(nbits);
    for (size_t w = 0; w < words; w++) {
        uint32_t v = bitmap[w];
        const uint64_t base = (uint64_t)w * 32;
        if (nbits - base < 32) v &= (1u << (nbits - base)) - 1u;
        while (v) {
            const unsigned b = (unsigned)__builtin_ctz(v);
            v &= v - 1;
            if (taken < max) out[taken++] = base + b;
            count++;
        }
    }
    if (total) *total = count;
    return taken;
}

// The fixed weights of the detection pass: column c of the table is the powers 1, a_c, a_c^2, ... of a constant a_c drawn from a
// SplitMix64 stream with this seed (the (c+1)-th output, reduced mod p). They depend on no transcript and no witness; the
// constants of different columns are different outputs of the stream.
constexpr uint64_t DETECT_SEED = 0x5150475055455850ull;   // "QPGPUEXP"
inline uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t detect_constant(uint32_t column) {
    constexpr uint64_t P = 0xFFFFFFFF00000001ull;
    uint64_t s = DETECT_SEED, z = 0;
    for (uint32_t i = 0; i <= column; i++) z = splitmix64(s);
    z %= P;
    return z < 2 ? z + 2 : z;    // never 0 or 1: their powers would weigh every constraint alike
}

}  // namespace explain
