// Drives the index arithmetic of stage s6 over a coset-sharded oracle (csrc/quotient_shard_map.hpp), which has no HIP in it, under
// the address and undefined-behaviour sanitizers: for every (degree_bits, rate_bits, qbits, shards) on the command line's grid, one
// shard (the stage on one context, lg = 0) included, it prints which shards evaluate quotient points, each one's launch, the quotient
// index of every local point and where every (exponent, j, c) of the merge reads and writes, one record per line. Built and run by tests/test_quotient_shard_map_host.py,
// which checks every line against Python integers.
//   quotient_shard_map <max degree_bits> <max rate_bits> <max qbits>
#include <cstdio>
#include <cstdlib>
#include "quotient_shard_map.hpp"

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s max_degree_bits max_rate_bits max_qbits\n", argv[0]); return 2; }
    const unsigned max_d = (unsigned)std::atoi(argv[1]), max_r = (unsigned)std::atoi(argv[2]), max_q = (unsigned)std::atoi(argv[3]);
    for (unsigned d = 1; d <= max_d; d++)
        for (unsigned r = 1; r <= max_r; r++)
            for (unsigned qbits = 0; qbits <= max_q && qbits <= r; qbits++)
                for (uint32_t G = 1; G <= (1u << r); G *= 2) {
                    // G = 1 is the stage on one context (a plan that is not sharded): log2_shards refuses it for the commitments
                    const int lg = G == 1 ? 0 : shard_map::log2_shards(G, r);
                    if (lg < 0) { std::printf("FAIL log2_shards %u %u\n", G, r); return 1; }
                    const shard_map::QuotientMap m = shard_map::QuotientMap::of(d, r, 1ull << qbits, (unsigned)lg);
                    // qbits = ceil(log2 factor): the smallest factor that needs qbits bits gives it as the largest does
                    if (m.qbits != qbits || shard_map::QuotientMap::of(d, r, (1ull << qbits) / 2 + 1, (unsigned)lg).qbits != qbits) {
                        std::printf("FAIL qbits %u %u\n", m.qbits, qbits);
                        return 1;
                    }
                    std::printf("case %u %u %u %u\n", d, r, qbits, G);
                    std::printf("domain %u %llu %u %u %llu\n", m.q_shift(), (unsigned long long)m.nq(), m.log_working(), m.working(),
                                (unsigned long long)m.points());
                    for (uint32_t g = 0; g < G; g++) {
                        std::printf("shard %u %d", g, m.works(g) ? 1 : 0);
                        if (m.works(g))
                            std::printf(" %u %u %u %u %u %u", m.local_log_lde(), m.local_rate_bits(), m.local_q_shift(), m.log_points(), m.exponent(g),
                                        m.shift_exponent(g));
                        std::printf("\n");
                        if (!m.works(g)) continue;
                        if (m.shard_of_exponent(m.exponent(g)) != g) { std::printf("FAIL shard_of_exponent %u\n", g); return 1; }
                        std::printf("points %u", g);
                        for (uint64_t i = 0; i < m.points(); i++) std::printf(" %llu", (unsigned long long)m.quotient_index(g, i));
                        std::printf("\n");
                    }
                    // the merge: output word (j, c) reads word j of gather block shard_of_exponent(e), every e
                    for (uint32_t c = 0; c < m.working(); c++) {
                        std::printf("out %u", c);
                        for (uint64_t j = 0; j < m.points(); j++) std::printf(" %llu", (unsigned long long)m.output_position(j, c));
                        std::printf("\n");
                    }
                    std::printf("blocks");
                    for (uint32_t e = 0; e < m.working(); e++) std::printf(" %u", m.shard_of_exponent(e));
                    std::printf("\n");
                }
    std::printf("quotient shard map: ok\n");
    return 0;
}
