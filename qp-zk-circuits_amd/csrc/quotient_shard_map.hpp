// quotient_shard_map.hpp — the index arithmetic of stage s6 on a coset-sharded oracle (qpgpu_stage_plan_create_sharded): which
// shards hold points of the quotient domain, what a working shard's launch looks like, and where its values go among the coefficient
// chunks. Host only and free of HIP, so that tests/native/quotient_shard_map_main.cpp can run it under the sanitizers on its own.
//
// Notation: d = degree_bits, r = rate_bits, qbits = ceil(log2 quotient_degree_factor) <= r, q_shift = r - qbits, G = 2^lg shards.
// The quotient is evaluated on Nq = 2^(d + qbits) points: the LDE points whose natural index is 0 mod 2^q_shift. Shard g holds the
// natural indices brev_lg(g) mod G (oracle_shard_map.hpp), local index i' being the global brev_lg(g) + G i'. So:
//   lg <= q_shift: only shard 0 holds quotient points, all Nq of them, at its local indices 0 mod 2^(q_shift - lg);
//   lg >  q_shift: the first Gq = G >> q_shift shards do, every local point is one (M = N/G = Nq/Gq each), and local index i' of
//                  shard g is the quotient point e + Gq i' with e = brev_lq(g), lq = log2 Gq.
// A working shard ends with A_g[j], j < M: the size-M inverse transform of its values, times (g_mult w^e)^-j (w = w_(d+qbits)), which
// is B_e[j] = sum_c (q_(j + cM) g_mult^(cM)) w_Gq^(e c). The home context inverts that Gq-point transform (quotient_merge_kernel):
//   q_(j + cM) = g_mult^(-cM) / Gq * sum_e w_Gq^(-e c) B_e[j].
#pragma once
#include <stdint.h>
#include "oracle_shard_map.hpp"

namespace shard_map {

struct QuotientMap {
    unsigned d = 0, r = 0, qbits = 0, lg = 0;
    // a circuit's s6 over 2^lg shards; lg = 0 is the unsharded stage: one working shard, whose launch is the circuit's own LDE
    static QuotientMap of(unsigned degree_bits, unsigned rate_bits, uint64_t quotient_degree_factor, unsigned lg) {
        QuotientMap m;
        m.d = degree_bits; m.r = rate_bits; m.lg = lg;
        while ((1ull << m.qbits) < quotient_degree_factor) m.qbits++;
        return m;
    }
    unsigned q_shift() const { return r - qbits; }
    uint64_t nq() const { return 1ull << (d + qbits); }
    unsigned log_working() const { return lg > q_shift() ? lg - q_shift() : 0; }      // lq
    uint32_t working() const { return 1u << log_working(); }                           // Gq: shards 0 .. Gq - 1 evaluate
    bool works(uint32_t g) const { return g < working(); }
    // a working shard's launch: its LDE has 2^local_log_lde() leaves at rate 2^local_rate_bits(), the quotient points are its local
    // natural indices 0 mod 2^local_q_shift(), points() of them
    unsigned local_log_lde() const { return d + r - lg; }
    unsigned local_rate_bits() const { return r - lg; }
    unsigned local_q_shift() const { return q_shift() > lg ? q_shift() - lg : 0; }
    unsigned log_points() const { return d + qbits - log_working(); }
    uint64_t points() const { return 1ull << log_points(); }                            // M
    // shard g's i'-th quotient point is the global quotient index exponent(g) + Gq i'
    uint32_t exponent(uint32_t g) const { return brev(g, log_working()); }
    uint32_t shard_of_exponent(uint32_t e) const { return brev(e, log_working()); }
    uint64_t quotient_index(uint32_t g, uint64_t i) const { return exponent(g) + ((uint64_t)i << log_working()); }
    // the shard's shift is g_mult w_(d+r)^shift_exponent(g), which is g_mult w_(d+qbits)^exponent(g)
    uint32_t shift_exponent(uint32_t g) const { return brev(g, lg); }
    // coefficient j + c M of a challenge's quotient polynomial: word output_position(j, c) of its 2^qbits chunks of 2^d, which takes
    // B_e[j] of every e (read at gather block shard_of_exponent(e), word j)
    uint64_t output_position(uint64_t j, uint32_t c) const { return (uint64_t)c * points() + j; }
};

}  // namespace shard_map
