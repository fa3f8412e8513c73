// zk_tree.hpp — the chain's 4-ary ZK Merkle tree on the device: level geometry and argument checks (host only, no HIP: also compiled
// stand-alone under the sanitizers by tools/host_checks/zk_tree_plan_check.cpp, zk_tree_append_check.cpp and zk_tree_reorg_check.cpp;
// what the kernels share of it is marked ZK_TREE_HD) and the launch interface of zk_tree_kernels.hip.
//
// Storage: one array of 32-byte nodes, level 0 (the leaves) first, every level behind the one below it. Level l holds
// ceil(count / 4^l) nodes; a child beyond a level's end is the empty hash (32 zero bytes) and is not stored.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ZK_TREE_HD __host__ __device__       // the geometry that the kernels share with the host
#else
#define ZK_TREE_HD
#endif

namespace zk_tree {

constexpr unsigned MAX_DEPTH = 16;                       // common/src/zk_merkle.rs:65
constexpr uint64_t MAX_LEAVES = 1ull << 24;
constexpr unsigned FLAG_FROM_TRANSFERS = 1u, KNOWN_FLAGS = FLAG_FROM_TRANSFERS;
constexpr size_t NODE_BYTES = 32, LEAF_RECORD_BYTES = 48, PATH_LEVEL_BYTES = 96;

// passed to the kernels by value
struct Plan {
    uint64_t count = 0;
    uint32_t depth = 0;
    uint64_t size[MAX_DEPTH + 1] = {0};                  // nodes of level l, l = 0 .. depth
    uint64_t off[MAX_DEPTH + 2] = {0};                   // first node of level l; off[depth + 1] = nodes in all
    uint64_t total() const { return off[depth + 1]; }
};

// ceil(count / 4^level); level <= 16, so 4^level fits 33 bits and the sum cannot wrap for count <= 2^24
ZK_TREE_HD inline uint64_t level_size(uint64_t count, unsigned level) { return (count + ((1ull << (2 * level)) - 1)) >> (2 * level); }

// the smallest depth with 4^depth >= count, at least 1 (a path always has a level); 0 when there is none up to MAX_DEPTH
inline unsigned min_depth(uint64_t count) {
    for (unsigned d = 1; d <= MAX_DEPTH; d++)
        if ((1ull << (2 * d)) >= count) return d;
    return 0;
}

// nullptr and a filled plan, or the reason the arguments are refused. depth = 0: the smallest valid depth.
inline const char *make_plan(uint64_t count, unsigned depth, unsigned flags, Plan &p) {
    if (count == 0) return "count is 0";
    if (count > MAX_LEAVES) return "count exceeds 2^24 leaves";
    if (flags & ~KNOWN_FLAGS) return "unknown flag";
    if (depth > MAX_DEPTH) return "depth exceeds 16";
    const unsigned dmin = min_depth(count);
    if (depth == 0) depth = dmin;
    if (depth < dmin) return "depth too small: 4^depth is below count";
    p = Plan();
    p.count = count; p.depth = depth;
    uint64_t at = 0;
    for (unsigned l = 0; l <= depth; l++) { p.size[l] = level_size(count, l); p.off[l] = at; at += p.size[l]; }
    p.off[depth + 1] = at;
    return nullptr;
}

// nodes first .. first + n of `level`
inline const char *check_range(const Plan &p, unsigned level, uint64_t first, uint64_t n) {
    if (level > p.depth) return "level above the tree's depth";
    if (first > p.size[level] || n > p.size[level] - first) return "range past the level's end";
    return nullptr;
}

// n paths: the output sizes must not wrap size_t (n x depth x 96 bytes), and every index names a leaf. *bad: the first refused entry.
inline const char *check_open(const Plan &p, const uint64_t *indices, uint64_t n, uint64_t *bad) {
    if (n > (uint64_t)SIZE_MAX / (PATH_LEVEL_BYTES * MAX_DEPTH)) return "too many paths for one call";
    for (uint64_t i = 0; i < n; i++)
        if (indices[i] >= p.count) { if (bad) *bad = i; return "leaf index out of range"; }
    return nullptr;
}

// ---- an append-only tree with room to grow (qpgpu_zk_tree_build_reserved / _append / _open_at) ----
// Appending k leaves at count n changes, at level l, exactly the nodes floor(n / 4^l) .. ceil((n + k) / 4^l) - 1: a node is dirty when
// its leaf range [i 4^l, (i + 1) 4^l) meets [n, n + k). So at count n the only node of level l >= 1 that a later append can change is
// the level's last one, and those `depth` nodes plus n describe the tree as it stood at n.

// The same layout as qpgpu_zk_snapshot (include/qpgpu_leaf.h), the nodes as words: passed to zk_open_at_kernel by value.
struct Snapshot {
    uint64_t count = 0;
    uint32_t depth = 0, reserved = 0;
    uint64_t last[MAX_DEPTH][4] = {{0}};                 // last[l - 1] = the last node of level l, l = 1 .. depth; the root is last[depth - 1]
};
constexpr size_t SNAPSHOT_NODES_BYTES = MAX_DEPTH * NODE_BYTES;

// the smallest depth with 4^depth >= capacity is min_depth(capacity). off[l] is laid out for `capacity` leaves, size[l] is that of the
// live `count`: an append never moves a node, and the kernels and check_range read the plan as they read make_plan's (which this is
// for capacity == count). total() is the nodes allocated.
inline const char *make_plan_reserved(uint64_t count, uint64_t capacity, unsigned depth, unsigned flags, Plan &p) {
    if (count == 0) return "count is 0";
    if (capacity > MAX_LEAVES) return "capacity exceeds 2^24 leaves";
    if (count > capacity) return "count exceeds the capacity";
    if (flags & ~KNOWN_FLAGS) return "unknown flag";
    if (depth > MAX_DEPTH) return "depth exceeds 16";
    const unsigned dmin = min_depth(capacity);
    if (depth == 0) depth = dmin;
    if (depth < dmin) return "depth too small: 4^depth is below capacity";
    p = Plan();
    p.count = count; p.depth = depth;
    uint64_t at = 0;
    for (unsigned l = 0; l <= depth; l++) { p.size[l] = level_size(count, l); p.off[l] = at; at += level_size(capacity, l); }
    p.off[depth + 1] = at;
    return nullptr;
}

// the nodes of `level` that an append of k >= 1 leaves at count n rehashes (level 0: the new leaves themselves)
inline void dirty_range(uint64_t n, uint64_t k, unsigned level, uint64_t &first, uint64_t &cnt) {
    first = n >> (2 * level);
    cnt = level_size(n + k, level) - first;
}

// reserved: the tree came from qpgpu_zk_tree_build_reserved
inline const char *check_append(const Plan &p, uint64_t capacity, bool reserved, uint64_t k, unsigned flags) {
    if (flags & ~KNOWN_FLAGS) return "unknown flag";
    if (!reserved) return "the tree was built by qpgpu_zk_tree_build, whose capacity is its count: nothing can be appended (use qpgpu_zk_tree_build_reserved)";
    if (k == 0) return "k is 0";
    if (p.count > capacity || k > capacity - p.count) return "count + k exceeds the tree's capacity";
    return nullptr;
}

// a snapshot against the tree it is opened on, then check_open against the snapshot's count
inline const char *check_open_at(const Plan &p, uint64_t snap_count, uint32_t snap_depth, const uint64_t *indices, uint64_t n, uint64_t *bad) {
    if (snap_count == 0) return "snapshot count is 0";
    if (snap_count > p.count) return "snapshot count exceeds the tree's leaf count";
    if (snap_depth != p.depth) return "snapshot depth differs from the tree's";
    if (n > (uint64_t)SIZE_MAX / (PATH_LEVEL_BYTES * MAX_DEPTH)) return "too many paths for one call";
    for (uint64_t i = 0; i < n; i++)
        if (indices[i] >= snap_count) { if (bad) *bad = i; return "leaf index out of range"; }
    return nullptr;
}

// ---- the tree as it stood at an earlier count, out of the tree alone (qpgpu_zk_tree_snapshots_at / _open_at_counts / _truncate) ----
// At count n every node of level l >= 1 except the level's last is still resident and unchanged (above). The last one, index
// level_size(n, l) - 1, is the hash of its children 4i .. 4i + 3 of level l - 1 as they stood at n: those at or beyond
// level_size(n, l - 1) were empty, the last existing one is the last node of level l - 1 (for l - 1 >= 1 the node derived one step
// earlier; a leaf is never rehashed), the others are resident. So the snapshot at n is a chain of `depth` node hashes over resident nodes.

// the last node of level l >= 1 at count n >= 1
struct LastNode {
    uint64_t index;                  // its index in level l: level_size(n, l) - 1
    uint32_t children;               // how many of its four children existed at n (1 .. 4): slots 0 .. children - 1 of level l - 1
    int32_t computed;                // the child slot that takes the node derived at level l - 1 (children - 1), or -1 at l = 1
};
ZK_TREE_HD inline LastNode last_node(uint64_t n, unsigned l) {
    LastNode r;
    r.index = level_size(n, l) - 1;
    r.children = (uint32_t)(level_size(n, l - 1) - 4 * r.index);
    r.computed = l >= 2 ? (int32_t)r.children - 1 : -1;
    return r;
}

// m counts, each 1 .. the live count. *bad: the first refused entry.
inline const char *check_counts(const Plan &p, const uint64_t *counts, uint64_t m, uint64_t *bad) {
    if (m > (uint64_t)SIZE_MAX / sizeof(Snapshot)) return "too many counts for one call";
    for (uint64_t i = 0; i < m; i++) {
        if (counts[i] == 0) { if (bad) *bad = i; return "count is 0"; }
        if (counts[i] > p.count) { if (bad) *bad = i; return "count exceeds the tree's leaf count"; }
    }
    return nullptr;
}

// n paths, path i against the tree as it stood at counts[i]: check_open_at with a count per path
inline const char *check_open_at_counts(const Plan &p, const uint64_t *counts, const uint64_t *indices, uint64_t n, uint64_t *bad) {
    if (n > (uint64_t)SIZE_MAX / (PATH_LEVEL_BYTES * MAX_DEPTH)) return "too many paths for one call";
    for (uint64_t i = 0; i < n; i++) {
        if (counts[i] == 0) { if (bad) *bad = i; return "count is 0"; }
        if (counts[i] > p.count) { if (bad) *bad = i; return "count exceeds the tree's leaf count"; }
        if (indices[i] >= counts[i]) { if (bad) *bad = i; return "leaf index out of range"; }
    }
    return nullptr;
}

// back to the first n leaves
inline const char *check_truncate(const Plan &p, uint64_t n) {
    if (n == 0) return "n is 0";
    if (n > p.count) return "n exceeds the tree's leaf count";
    return nullptr;
}

}  // namespace zk_tree

#ifndef ZK_TREE_PLAN_ONLY   // the stand-alone host check takes the geometry alone
#include <hip/hip_runtime_api.h>
namespace poseidon2 { struct Params; }
// every launcher: p2 = the device copy of qp-poseidon-core's parameter set (qpgpu_ctx::d_p2_app)
// count records of 48 bytes (qpgpu_zk_leaf) -> count leaf hashes
hipError_t zk_tree_leaf_hashes(const uint8_t *d_records, uint64_t count, uint8_t *d_out, const poseidon2::Params *p2, hipStream_t st);
// levels 1 .. depth of a tree whose level 0 is in place; *d_bad_leaf (preset to 0xFFFFFFFF) receives the lowest index of a leaf with a
// non-canonical limb
hipError_t zk_tree_reduce(uint8_t *d_nodes, const zk_tree::Plan &plan, uint32_t *d_bad_leaf, const poseidon2::Params *p2, hipStream_t st);
// n paths: d_siblings n x depth x 96 bytes, d_positions n x depth bytes
hipError_t zk_tree_open_paths(const uint8_t *d_nodes, const zk_tree::Plan &plan, const uint64_t *d_indices, uint64_t n, uint8_t *d_siblings,
                              uint8_t *d_positions, hipStream_t st);
// leaves first .. first + k of level 0 (just uploaded, beyond the live count): *d_bad_leaf (preset to 0xFFFFFFFF) receives the lowest
// tree index of one with a non-canonical limb
hipError_t zk_tree_check_leaves(const uint8_t *d_nodes, const zk_tree::Plan &plan, uint64_t first, uint64_t k, uint32_t *d_bad_leaf, hipStream_t st);
// after an append: `grown` is the plan at the new count, n_old the count before it, level 0 is in place. Rehashes the dirty nodes of
// levels 1 .. depth and gathers the grown tree's snapshot nodes into d_snap_nodes (16 x 32 bytes); does neither when *d_bad_leaf is set.
hipError_t zk_tree_rehash(uint8_t *d_nodes, const zk_tree::Plan &grown, uint64_t n_old, const uint32_t *d_bad_leaf, uint8_t *d_snap_nodes,
                          const poseidon2::Params *p2, hipStream_t st);
// the snapshot nodes of the tree as it stands
hipError_t zk_tree_gather_snapshot(const uint8_t *d_nodes, const zk_tree::Plan &plan, uint8_t *d_snap_nodes, hipStream_t st);
// zk_tree_open_paths on the tree as it stood at snap.count (checked against the plan on the host: zk_tree::check_open_at)
hipError_t zk_tree_open_paths_at(const uint8_t *d_nodes, const zk_tree::Plan &plan, const zk_tree::Snapshot &snap, const uint64_t *d_indices,
                                 uint64_t n, uint8_t *d_siblings, uint8_t *d_positions, hipStream_t st);
// d_out[j] = the snapshot of the tree as it stood at d_counts[j] leaves, j < m, derived from the resident nodes (counts checked on the
// host: zk_tree::check_counts)
hipError_t zk_tree_derive_snapshots(const uint8_t *d_nodes, const zk_tree::Plan &plan, const uint64_t *d_counts, uint64_t m, zk_tree::Snapshot *d_out,
                                    const poseidon2::Params *p2, hipStream_t st);
// zk_tree_open_paths_at with a snapshot per path: path q is opened at d_snaps[d_snap_of[q]] (m of them, from zk_tree_derive_snapshots
// on this tree; zk_tree::check_open_at_counts on the host). d_roots (n x 32 bytes, may be null): the root each path leads to.
hipError_t zk_tree_open_paths_at_many(const uint8_t *d_nodes, const zk_tree::Plan &plan, const zk_tree::Snapshot *d_snaps, uint64_t m,
                                      const uint32_t *d_snap_of, const uint64_t *d_indices, uint64_t n, uint8_t *d_siblings, uint8_t *d_positions,
                                      uint8_t *d_roots, hipStream_t st);
// a truncate: `cut` is the plan at the new count, *d_snap the snapshot derived at that count. Its nodes go over the last node of every
// level of `cut` and into d_snap_nodes (16 x 32 bytes).
hipError_t zk_tree_place_snapshot(uint8_t *d_nodes, const zk_tree::Plan &cut, const zk_tree::Snapshot *d_snap, uint8_t *d_snap_nodes, hipStream_t st);
#endif  // ZK_TREE_PLAN_ONLY
