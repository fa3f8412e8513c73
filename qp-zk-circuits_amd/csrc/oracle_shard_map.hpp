// oracle_shard_map.hpp — the index arithmetic of a coset-sharded oracle (qpgpu_oracle_commit_sharded): which leaves, which cosets
// and which part of a Merkle path belong to which shard. Host only and free of HIP, so that tests/native/oracle_shard_map_main.cpp
// can run it under the sanitizers on its own.
//
// The LDE of 2^d coefficients at rate 2^r has N = 2^(d + r) leaves; leaf s holds the value at shift w_(d+r)^brev_(d+r)(s). Coset k
// (the points shift w_(d+r)^k w_d^t) is the contiguous leaf block brev_r(k) 2^d. G = 2^lg shards split the leaves into G contiguous
// ranges, so shard g owns the cosets k with brev_r(k) >> (r - lg) == g, which are exactly the k = brev_lg(g) (mod G): writing
// k = brev_lg(g) + G k', the shard's points are (shift w_(d+r)^brev_lg(g)) w_(d+r-lg)^k' w_d^t. That is a whole LDE of its own, at rate
// 2^(r - lg), on the shift `shift w_(d+r)^brev_lg(g)`, and its leaf order is the shard's slice of the global leaf order. A range of
// N/G leaves is a subtree, so the shard reduces it to max(1, 2^cap_h / G) roots alone; when G > 2^cap_h the home context hashes the
// remaining lg - cap_h levels over the G roots.
#pragma once
#include <stdint.h>

namespace shard_map {

inline uint32_t brev(uint32_t x, unsigned bits) {
    uint32_t r = 0;
    for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

// log2 of a valid shard count (a power of two, 2 <= G <= 2^rate_bits), or -1
inline int log2_shards(uint32_t n_shards, unsigned rate_bits) {
    if (n_shards < 2 || (n_shards & (n_shards - 1)) || rate_bits > 31) return -1;
    int lg = 0;
    while ((1u << lg) < n_shards) lg++;
    return (unsigned)lg <= rate_bits ? lg : -1;
}

struct Map {
    unsigned d = 0, r = 0, cap_h = 0, lg = 0;      // degree_bits, rate_bits, cap_height, log2 of the shard count
    uint32_t shards() const { return 1u << lg; }
    unsigned log_leaves() const { return d + r; }
    // the shard's own LDE and tree
    unsigned local_rate_bits() const { return r - lg; }
    unsigned local_log_leaves() const { return d + r - lg; }
    uint64_t local_leaves() const { return 1ull << local_log_leaves(); }
    unsigned local_cap_h() const { return cap_h > lg ? cap_h - lg : 0; }
    unsigned merge_levels() const { return lg > cap_h ? lg - cap_h : 0; }      // hashed by the home context over the shards' roots
    unsigned local_path_len() const { return local_log_leaves() - local_cap_h(); }
    unsigned path_len() const { return local_path_len() + merge_levels(); }     // = d + r - cap_h
    // leaves
    uint64_t first_leaf(uint32_t g) const { return (uint64_t)g << local_log_leaves(); }
    uint32_t shard_of(uint64_t leaf) const { return (uint32_t)(leaf >> local_log_leaves()); }
    uint64_t local_of(uint64_t leaf) const { return leaf & (local_leaves() - 1); }
    uint64_t global_of(uint32_t g, uint64_t local) const { return first_leaf(g) | local; }
    // cosets: the j-th 2^d-leaf block of shard g holds coset coset_of(g, j) of the 2^r
    uint32_t cosets_per_shard() const { return 1u << local_rate_bits(); }
    uint32_t coset_of(uint32_t g, uint32_t j) const { return brev((g << local_rate_bits()) | j, r); }
    bool owns_coset(uint32_t g, uint32_t k) const { return (brev(k, r) >> local_rate_bits()) == g; }
    // the shard's LDE runs on the shift `shift * w_(d+r)^shift_exponent(g)`
    uint32_t shift_exponent(uint32_t g) const { return brev(g, lg); }
    // merge level t (0: the G roots) holds G >> t nodes, the levels back to back as the digest arrays everywhere; a leaf of shard g
    // passes node g >> t there and its path takes the sibling
    uint32_t merge_sibling(uint32_t g, unsigned t) const { return (g >> t) ^ 1u; }
    uint64_t merge_level_offset(unsigned t) const { return (2ull * shards()) - ((2ull * shards()) >> t); }   // in digests
    uint64_t merge_digests() const { return merge_levels() ? 2ull * shards() - (1ull << cap_h) : 0; }
};

}  // namespace shard_map
