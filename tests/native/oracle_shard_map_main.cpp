// Drives the index arithmetic of a coset-sharded oracle (csrc/oracle_shard_map.hpp), which has no HIP in it, under the address and
// undefined-behaviour sanitizers: for every (degree_bits, rate_bits, shards) on the command line's grid it prints the shards' leaf
// ranges, their cosets and shifts, the leaf -> (shard, local leaf) map and the split of a Merkle path, one record per line.
// Built and run by tests/test_oracle_shard_map_host.py, which checks every line against Python integers.
//   oracle_shard_map <max degree_bits> <max rate_bits> <max cap_height>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "oracle_shard_map.hpp"

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s max_degree_bits max_rate_bits max_cap_height\n", argv[0]); return 2; }
    const unsigned max_d = (unsigned)std::atoi(argv[1]), max_r = (unsigned)std::atoi(argv[2]), max_cap = (unsigned)std::atoi(argv[3]);
    // shard counts that are refused: not a power of two, one, more than the cosets
    for (uint32_t G : {0u, 1u, 3u, 6u, 12u})
        for (unsigned r = 1; r <= max_r; r++) std::printf("refused %u %u %d\n", G, r, shard_map::log2_shards(G, r));
    for (unsigned r = 1; r <= max_r; r++) std::printf("refused %u %u %d\n", 2u << r, r, shard_map::log2_shards(2u << r, r));
    for (unsigned d = 1; d <= max_d; d++)
        for (unsigned r = 1; r <= max_r; r++)
            for (uint32_t G = 2; G <= 8 && G <= (1u << r); G *= 2) {
                shard_map::Map m;
                m.d = d; m.r = r;
                const int lg = shard_map::log2_shards(G, r);
                if (lg < 0) { std::printf("FAIL log2_shards %u %u\n", G, r); return 1; }
                m.lg = (unsigned)lg;
                std::printf("case %u %u %u\n", d, r, m.shards());
                for (uint32_t g = 0; g < G; g++) {
                    std::printf("range %u %llu %llu\n", g, (unsigned long long)m.first_leaf(g), (unsigned long long)m.local_leaves());
                    std::printf("shift %u %u %u %u\n", g, m.shift_exponent(g), m.local_rate_bits(), m.local_log_leaves());
                    std::printf("cosets %u", g);
                    for (uint32_t j = 0; j < m.cosets_per_shard(); j++) std::printf(" %u", m.coset_of(g, j));
                    std::printf("\nowns %u", g);
                    for (uint32_t k = 0; k < (1u << r); k++) std::printf(" %d", m.owns_coset(g, k) ? 1 : 0);
                    std::printf("\n");
                }
                for (uint64_t leaf = 0; leaf < (1ull << (d + r)); leaf++) {
                    const uint32_t g = m.shard_of(leaf);
                    const uint64_t local = m.local_of(leaf);
                    std::printf("leaf %llu %u %llu %llu\n", (unsigned long long)leaf, g, (unsigned long long)local, (unsigned long long)m.global_of(g, local));
                }
                for (unsigned cap = 0; cap <= max_cap && cap <= d + r; cap++) {
                    m.cap_h = cap;
                    std::printf("path %u %u %u %u %u %llu", cap, m.local_cap_h(), m.local_path_len(), m.merge_levels(), m.path_len(),
                                (unsigned long long)m.merge_digests());
                    for (unsigned t = 0; t < m.merge_levels(); t++) std::printf(" %llu", (unsigned long long)m.merge_level_offset(t));
                    std::printf("\n");
                    for (uint32_t g = 0; g < G; g++) {
                        std::printf("siblings %u %u", cap, g);
                        for (unsigned t = 0; t < m.merge_levels(); t++) std::printf(" %u", m.merge_sibling(g, t));
                        std::printf("\n");
                    }
                }
            }
    std::printf("oracle shard map: ok\n");
    return 0;
}
