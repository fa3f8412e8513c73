// zk_tree_kernels.hip — the chain's 4-ary ZK Merkle tree for gfx950 (common/src/zk_merkle.rs; the host restatement is
// leaf_witness.cpp's qpgpu_zk_*, which is the specification these kernels are tested against byte for byte).
//
//   zk_leaf_hash_kernel   one thread per transfer: Poseidon2 of (to_account x4, transfer_count hi/lo, asset_id, input_amount), two permutations
//   zk_node_kernel        one thread per parent: four children sorted as 32-byte strings, sixteen limbs absorbed, three permutations
//   zk_top_kernel         the levels that fit one workgroup, in one launch, a workgroup barrier between levels
//   zk_open_kernel        one thread per (query, level): the group of four sorted, the running node taken out; no hashing
// and for a tree that is appended to (zk_tree.hpp: dirty ranges, snapshots):
//   zk_leaf_check_kernel  one thread per appended leaf hash: the canonicity test, before anything is rehashed
//   zk_node_range_kernel  zk_node_kernel over the dirty parents of a level, while there are more than a workgroup of them
//   zk_append_top_kernel  zk_top_kernel over the dirty ranges of every remaining level, then the snapshot of the grown tree
//   zk_snapshot_kernel    the snapshot alone
//   zk_open_at_kernel     zk_open_kernel on the tree as it stood at a snapshot
// and for the tree at earlier counts without a kept snapshot, and for a reorg (zk_tree.hpp: last_node):
//   zk_snapshots_at_kernel    one thread per count: the snapshot at that count, `depth` node hashes over the resident nodes
//   zk_open_at_many_kernel    zk_open_at_kernel with a snapshot per path, read from memory; the path's root too
//   zk_place_snapshot_kernel  a derived snapshot written over the last node of every level: the tree truncated to that count
//
// The hash is the application hash of the Wormhole circuits: the pad `|| 1 || 0*` sponge with additive absorption over
// poseidon2::permute_qp (qp-poseidon-core's set), the permutation behind p2_pad10_sponge_kernel<true>; the context's proof-system
// hasher plays no part. Integer-ALU-bound like every thread-per-hash kernel here (merkle_hash_impl.hpp).
#include <hip/hip_runtime.h>
#include "gl64.hpp"
#include "poseidon.hpp"
#include "zk_tree.hpp"

using gl::u32;
using gl::u64;
typedef uint8_t u8;

namespace {

// A node as a sort key: limb i byte-swapped, so that comparing k[0], then k[1], .. as integers is the order of the 32 bytes as a string
// ([u8; 32]'s Ord), which is NOT the order of the little-endian limbs as integers.
struct Key { u64 k0, k1, k2, k3; };

__device__ __forceinline__ Key load_key(const u8 *node) {
    const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(node);     // nodes are 32-byte aligned
    const ulonglong2 a = p[0], b = p[1];
    return Key{__builtin_bswap64(a.x), __builtin_bswap64(a.y), __builtin_bswap64(b.x), __builtin_bswap64(b.y)};
}
__device__ __forceinline__ void store_key(u8 *node, const Key &a) {
    ulonglong2 *p = reinterpret_cast<ulonglong2 *>(node);
    p[0] = make_ulonglong2(__builtin_bswap64(a.k0), __builtin_bswap64(a.k1));
    p[1] = make_ulonglong2(__builtin_bswap64(a.k2), __builtin_bswap64(a.k3));
}
__device__ __forceinline__ bool key_less(const Key &a, const Key &b) {
    return a.k0 < b.k0 || (a.k0 == b.k0 && (a.k1 < b.k1 || (a.k1 == b.k1 && (a.k2 < b.k2 || (a.k2 == b.k2 && a.k3 < b.k3)))));
}
__device__ __forceinline__ bool key_equal(const Key &a, const Key &b) { return a.k0 == b.k0 && a.k1 == b.k1 && a.k2 == b.k2 && a.k3 == b.k3; }
__device__ __forceinline__ Key key_select(bool c, const Key &a, const Key &b) {
    return Key{c ? a.k0 : b.k0, c ? a.k1 : b.k1, c ? a.k2 : b.k2, c ? a.k3 : b.k3};
}
// comparator: afterwards a <= b (equal keys are the same bytes, so their order is not observable)
__device__ __forceinline__ void key_cswap(Key &a, Key &b) {
    const bool sw = key_less(b, a);
    const Key lo = key_select(sw, b, a), hi = key_select(sw, a, b);
    a = lo; b = hi;
}
// the five-comparator network for four: named registers throughout, nothing indexed by data
__device__ __forceinline__ void key_sort4(Key &a, Key &b, Key &c, Key &d) {
    key_cswap(a, b); key_cswap(c, d); key_cswap(a, c); key_cswap(b, d); key_cswap(b, c);
}
// a limb >= p anywhere in the node (the test is on the limb itself: bswap of the key)
__device__ __forceinline__ bool key_noncanonical(const Key &a) {
    return __builtin_bswap64(a.k0) >= gl::P || __builtin_bswap64(a.k1) >= gl::P || __builtin_bswap64(a.k2) >= gl::P || __builtin_bswap64(a.k3) >= gl::P;
}

// children 4g .. 4g + 3 of a level of n_in nodes; a child beyond the level's end is the empty hash
__device__ __forceinline__ void load_group(const u8 *level, u64 n_in, u64 g, Key &a, Key &b, Key &c, Key &d) {
    const Key zero{0, 0, 0, 0};
    const u64 i = 4 * g;
    a = i < n_in ? load_key(level + 32 * i) : zero;
    b = i + 1 < n_in ? load_key(level + 32 * (i + 1)) : zero;
    c = i + 2 < n_in ? load_key(level + 32 * (i + 2)) : zero;
    d = i + 3 < n_in ? load_key(level + 32 * (i + 3)) : zero;
}

// hash_node of four children in any order: sorted as 32-byte strings, sixteen limbs absorbed, three permutations. out: the node's limbs.
__device__ __forceinline__ void hash_keys(Key a, Key b, Key c, Key d, u64 out[4], const poseidon2::Params &p2) {
    key_sort4(a, b, c, d);
    u64 s[12];
    s[0] = __builtin_bswap64(a.k0); s[1] = __builtin_bswap64(a.k1); s[2] = __builtin_bswap64(a.k2); s[3] = __builtin_bswap64(a.k3);
    s[4] = __builtin_bswap64(b.k0); s[5] = __builtin_bswap64(b.k1); s[6] = __builtin_bswap64(b.k2); s[7] = __builtin_bswap64(b.k3);
    s[8] = s[9] = s[10] = s[11] = 0;
    poseidon2::permute_qp(s, p2);
    // (limbs are canonical, or the tree is refused and never read: add_canonical is exact for them)
    s[0] = gl::add_canonical(s[0], __builtin_bswap64(c.k0)); s[1] = gl::add_canonical(s[1], __builtin_bswap64(c.k1));
    s[2] = gl::add_canonical(s[2], __builtin_bswap64(c.k2)); s[3] = gl::add_canonical(s[3], __builtin_bswap64(c.k3));
    s[4] = gl::add_canonical(s[4], __builtin_bswap64(d.k0)); s[5] = gl::add_canonical(s[5], __builtin_bswap64(d.k1));
    s[6] = gl::add_canonical(s[6], __builtin_bswap64(d.k2)); s[7] = gl::add_canonical(s[7], __builtin_bswap64(d.k3));
    poseidon2::permute_qp(s, p2);
    s[0] = gl::add_canonical(s[0], 1);           // sixteen elements fill two rate blocks: the terminator opens a third
    poseidon2::permute_qp(s, p2);
    out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = s[3];
}

// hash_node: parent g of a level. bad_leaf != nullptr (the pass over level 0 only): the lowest index of a child with a limb >= p is
// recorded; inner nodes are permutation outputs, canonical by construction.
__device__ __forceinline__ void hash_parent(const u8 *in, u64 n_in, u64 g, u8 *out, u32 *bad_leaf, const poseidon2::Params &p2) {
    Key a, b, c, d;
    load_group(in, n_in, g, a, b, c, d);
    if (bad_leaf) {                              // wave-uniform; children are tested in index order, before the sort moves them
        const u32 i = (u32)(4 * g);
        const u32 bad = key_noncanonical(a) ? i : key_noncanonical(b) ? i + 1 : key_noncanonical(c) ? i + 2 : key_noncanonical(d) ? i + 3 : 0xFFFFFFFFu;
        if (bad != 0xFFFFFFFFu) atomicMin(bad_leaf, bad);     // (a missing child is zero: canonical)
    }
    u64 h[4];
    hash_keys(a, b, c, d, h, p2);
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 32 * g);
    o[0] = make_ulonglong2(h[0], h[1]);
    o[1] = make_ulonglong2(h[2], h[3]);
}

__global__ void __launch_bounds__(256) zk_node_kernel(const u8 *in, u64 n_in, u8 *out, u64 n_out, u32 *bad_leaf, const poseidon2::Params *p2) {
    const u64 g = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (g >= n_out) return;
    hash_parent(in, n_in, g, out, bad_leaf, *p2);
}

// levels first + 1 .. depth, each of at most blockDim.x parents, by one workgroup: a level's nodes are written to the node array and read
// back by the next level's threads after the barrier (the same CU, and __syncthreads orders global memory within the workgroup)
__global__ void __launch_bounds__(256) zk_top_kernel(u8 *nodes, zk_tree::Plan plan, u32 first, u32 *bad_leaf, const poseidon2::Params *p2) {
    for (u32 l = first; l < plan.depth; l++) {
        const u64 n_in = plan.size[l], n_out = plan.size[l + 1];
        if (threadIdx.x < n_out) hash_parent(nodes + 32 * plan.off[l], n_in, threadIdx.x, nodes + 32 * plan.off[l + 1], l == 0 ? bad_leaf : nullptr, *p2);
        __syncthreads();
    }
}

// record i: 48 bytes = six little-endian words (qpgpu_zk_leaf: account x4, transfer_count, asset_id | input_amount << 32)
__global__ void __launch_bounds__(256) zk_leaf_hash_kernel(const u64 *records, u64 count, u8 *out, const poseidon2::Params *p2) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(records + 6 * i);    // 48-byte records: 16-byte aligned
    const ulonglong2 a = r[0], b = r[1], c = r[2];
    u64 s[12];
    s[0] = gl::canon(a.x); s[1] = gl::canon(a.y); s[2] = gl::canon(b.x); s[3] = gl::canon(b.y);     // bytes_to_digest reduces mod p
    s[4] = c.x >> 32; s[5] = c.x & 0xFFFFFFFFull;                                                    // u64_to_felts: most significant limb first
    s[6] = c.y & 0xFFFFFFFFull; s[7] = c.y >> 32;
    s[8] = s[9] = s[10] = s[11] = 0;
    poseidon2::permute_qp(s, *p2);
    s[0] = gl::add_canonical(s[0], 1);           // eight elements fill the rate: the terminator opens a second block
    poseidon2::permute_qp(s, *p2);
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 32 * i);
    o[0] = make_ulonglong2(s[0], s[1]);
    o[1] = make_ulonglong2(s[2], s[3]);
}

// thread t = query q, level l: the three siblings of the running node (ancestor of leaf indices[q] at level l) in sorted order and the
// position the node takes among the four: ZkMerkleProof::from_unsorted without its hashing, since the tree holds every running node
__global__ void __launch_bounds__(256) zk_open_kernel(const u8 *nodes, zk_tree::Plan plan, const u64 *indices, u64 n, u8 *siblings, u8 *positions) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n * plan.depth) return;
    const u64 q = t / plan.depth;
    const u32 l = (u32)(t - q * plan.depth);
    const u64 idx = indices[q] >> (2 * l);       // checked against the leaf count on the host
    const u8 *level = nodes + 32 * plan.off[l];
    Key a, b, c, d;
    load_group(level, plan.size[l], idx >> 2, a, b, c, d);
    const Key cur = load_key(level + 32 * idx);
    key_sort4(a, b, c, d);
    const u32 pos = key_equal(a, cur) ? 0u : key_equal(b, cur) ? 1u : key_equal(c, cur) ? 2u : 3u;      // the first slot holding the running node
    u8 *o = siblings + 96 * t;                   // t = q * depth + l: level major within a query
    store_key(o, pos < 1 ? b : a);
    store_key(o + 32, pos < 2 ? c : b);
    store_key(o + 64, pos < 3 ? d : c);
    positions[t] = (u8)pos;
}

// ---- the append-only tree (zk_tree.hpp: dirty ranges and snapshots) ----

// thread j: leaf first + j of level 0, uploaded beyond the live count and not yet part of the tree, is tested before any node is rehashed
__global__ void __launch_bounds__(256) zk_leaf_check_kernel(const u8 *level0, u64 first, u64 k, u32 *bad_leaf) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= k) return;
    if (key_noncanonical(load_key(level0 + 32 * (first + j)))) atomicMin(bad_leaf, (u32)(first + j));     // (indices are below 2^24)
}

// parents first .. first + cnt of a level: zk_node_kernel over a dirty range. Nothing is written once a new leaf was refused.
__global__ void __launch_bounds__(256) zk_node_range_kernel(const u8 *in, u64 n_in, u8 *out, u64 first, u64 cnt, const u32 *bad_leaf,
                                                            const poseidon2::Params *p2) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= cnt || *bad_leaf != 0xFFFFFFFFu) return;
    hash_parent(in, n_in, first + t, out, nullptr, *p2);
}

// snap[l - 1] = the last node of level l, l = 1 .. depth, the rest zero; by the first 16 threads of a workgroup
__device__ __forceinline__ void gather_snapshot(const u8 *nodes, const zk_tree::Plan &plan, u8 *snap) {
    if (threadIdx.x >= zk_tree::MAX_DEPTH) return;
    const u32 l = threadIdx.x + 1;
    const Key zero{0, 0, 0, 0};
    store_key(snap + 32 * threadIdx.x, l <= plan.depth ? load_key(nodes + 32 * (plan.off[l] + plan.size[l] - 1)) : zero);
}

// zk_top_kernel over dirty ranges: `plan` is the tree at its new count, n_old the count before the append. Levels first + 1 .. depth,
// each with at most blockDim.x dirty parents, by one workgroup with a barrier between levels; then the snapshot of the grown tree.
// The refusal word is read by every thread before the first barrier and written by nobody here: the early return is uniform.
__global__ void __launch_bounds__(256) zk_append_top_kernel(u8 *nodes, zk_tree::Plan plan, u32 first, u64 n_old, const u32 *bad_leaf, u8 *snap,
                                                            const poseidon2::Params *p2) {
    if (*bad_leaf != 0xFFFFFFFFu) return;
    for (u32 l = first; l < plan.depth; l++) {
        const u64 lo = n_old >> (2 * (l + 1)), cnt = plan.size[l + 1] - lo;
        if (threadIdx.x < cnt) hash_parent(nodes + 32 * plan.off[l], plan.size[l], lo + threadIdx.x, nodes + 32 * plan.off[l + 1], nullptr, *p2);
        __syncthreads();
    }
    gather_snapshot(nodes, plan, snap);
}

__global__ void __launch_bounds__(64) zk_snapshot_kernel(const u8 *nodes, zk_tree::Plan plan, u8 *snap) { gather_snapshot(nodes, plan, snap); }

// node i of level l of the tree as it stood at snap.count, n_l = ceil(snap.count / 4^l) its size then: beyond the end the empty hash,
// the last node of a level above the leaves from the snapshot (later appends may have rehashed it), every other node still resident
__device__ __forceinline__ Key load_key_at(const u8 *level, const zk_tree::Snapshot &snap, u32 l, u64 n_l, u64 i) {
    if (i >= n_l) return Key{0, 0, 0, 0};
    if (l >= 1 && i == n_l - 1) {
        const uint64_t *w = snap.last[l - 1];
        return Key{__builtin_bswap64(w[0]), __builtin_bswap64(w[1]), __builtin_bswap64(w[2]), __builtin_bswap64(w[3])};
    }
    return load_key(level + 32 * i);
}

// zk_open_kernel against an earlier count of the same tree: the group and the running node go through load_key_at
__global__ void __launch_bounds__(256) zk_open_at_kernel(const u8 *nodes, zk_tree::Plan plan, zk_tree::Snapshot snap, const u64 *indices, u64 n,
                                                         u8 *siblings, u8 *positions) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n * plan.depth) return;
    const u64 q = t / plan.depth;
    const u32 l = (u32)(t - q * plan.depth);
    const u64 idx = indices[q] >> (2 * l);       // checked against the snapshot's count on the host
    const u64 n_l = (snap.count + ((1ull << (2 * l)) - 1)) >> (2 * l), g = idx & ~(u64)3;
    const u8 *level = nodes + 32 * plan.off[l];
    Key a = load_key_at(level, snap, l, n_l, g), b = load_key_at(level, snap, l, n_l, g + 1), c = load_key_at(level, snap, l, n_l, g + 2),
        d = load_key_at(level, snap, l, n_l, g + 3);
    const Key cur = load_key_at(level, snap, l, n_l, idx);
    key_sort4(a, b, c, d);
    const u32 pos = key_equal(a, cur) ? 0u : key_equal(b, cur) ? 1u : key_equal(c, cur) ? 2u : 3u;
    u8 *o = siblings + 96 * t;
    store_key(o, pos < 1 ? b : a);
    store_key(o + 32, pos < 2 ? c : b);
    store_key(o + 64, pos < 3 ? d : c);
    positions[t] = (u8)pos;
}

// ---- the tree at earlier counts, out of the tree alone (zk_tree.hpp: last_node) ----

// thread j: the snapshot of the tree as it stood at counts[j] leaves: the last node of level l = 1 .. depth is the hash of its children
// of level l - 1 as they stood then: beyond the level's end the empty hash, the level's last node the one derived a step earlier (later
// appends may have rehashed the resident copy; a leaf is never rehashed), every other child resident. A chain of `depth` dependent
// node hashes on one thread, the latency class of the narrow levels of zk_append_top_kernel; a wave per workgroup spreads many counts
// over the CUs. Counts are checked on the host (1 .. plan.count), so every read is below the live size of its level.
__global__ void __launch_bounds__(64) zk_snapshots_at_kernel(const u8 *nodes, zk_tree::Plan plan, const u64 *counts, u64 m, zk_tree::Snapshot *out,
                                                             const poseidon2::Params *p2) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= m) return;
    const u64 n = counts[j];
    zk_tree::Snapshot *o = out + j;
    o->count = n; o->depth = plan.depth; o->reserved = 0;
    const Key zero{0, 0, 0, 0};
    Key cur = zero;
#pragma unroll 1
    for (u32 l = 1; l <= plan.depth; l++) {
        const zk_tree::LastNode ln = zk_tree::last_node(n, l);
        const u8 *group = nodes + 32 * (plan.off[l - 1] + 4 * ln.index);
        const Key a = ln.computed == 0 ? cur : load_key(group);                          // (a last node has at least one child)
        const Key b = ln.children < 2 ? zero : ln.computed == 1 ? cur : load_key(group + 32);
        const Key c = ln.children < 3 ? zero : ln.computed == 2 ? cur : load_key(group + 64);
        const Key d = ln.children < 4 ? zero : ln.computed == 3 ? cur : load_key(group + 96);
        u64 h[4];
        hash_keys(a, b, c, d, h, *p2);
        o->last[l - 1][0] = h[0]; o->last[l - 1][1] = h[1]; o->last[l - 1][2] = h[2]; o->last[l - 1][3] = h[3];
        cur = Key{__builtin_bswap64(h[0]), __builtin_bswap64(h[1]), __builtin_bswap64(h[2]), __builtin_bswap64(h[3])};
    }
    for (u32 l = plan.depth; l < zk_tree::MAX_DEPTH; l++) o->last[l][0] = o->last[l][1] = o->last[l][2] = o->last[l][3] = 0;
}

// zk_open_at_kernel with a snapshot per path, read from memory: path q is opened at snaps[snap_of[q]]. roots != nullptr: the thread of a
// path's top level also writes the root the path leads to, the snapshot's last[depth - 1].
__global__ void __launch_bounds__(256) zk_open_at_many_kernel(const u8 *nodes, zk_tree::Plan plan, const zk_tree::Snapshot *snaps, const u32 *snap_of,
                                                              const u64 *indices, u64 n, u8 *siblings, u8 *positions, u8 *roots) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= n * plan.depth) return;
    const u64 q = t / plan.depth;
    const u32 l = (u32)(t - q * plan.depth);
    const zk_tree::Snapshot &snap = snaps[snap_of[q]];
    const u64 idx = indices[q] >> (2 * l);       // checked against the path's count on the host
    const u64 n_l = zk_tree::level_size(snap.count, l), g = idx & ~(u64)3;
    const u8 *level = nodes + 32 * plan.off[l];
    Key a = load_key_at(level, snap, l, n_l, g), b = load_key_at(level, snap, l, n_l, g + 1), c = load_key_at(level, snap, l, n_l, g + 2),
        d = load_key_at(level, snap, l, n_l, g + 3);
    const Key cur = load_key_at(level, snap, l, n_l, idx);
    key_sort4(a, b, c, d);
    const u32 pos = key_equal(a, cur) ? 0u : key_equal(b, cur) ? 1u : key_equal(c, cur) ? 2u : 3u;
    u8 *o = siblings + 96 * t;
    store_key(o, pos < 1 ? b : a);
    store_key(o + 32, pos < 2 ? c : b);
    store_key(o + 64, pos < 3 ? d : c);
    positions[t] = (u8)pos;
    if (roots && l == plan.depth - 1) {
        const uint64_t *w = snap.last[l];
        ulonglong2 *r = reinterpret_cast<ulonglong2 *>(roots + 32 * q);
        r[0] = make_ulonglong2(w[0], w[1]);
        r[1] = make_ulonglong2(w[2], w[3]);
    }
}

// a truncate's last step, by the first 16 threads of a workgroup: the snapshot derived at the new count goes over the last node of every
// level of `plan` (the tree at that count) and into snap_nodes, as gather_snapshot leaves them
__global__ void __launch_bounds__(64) zk_place_snapshot_kernel(u8 *nodes, zk_tree::Plan plan, const zk_tree::Snapshot *snap, u8 *snap_nodes) {
    if (threadIdx.x >= zk_tree::MAX_DEPTH) return;
    const u32 l = threadIdx.x + 1;
    const uint64_t *w = snap->last[l - 1];
    const ulonglong2 lo = make_ulonglong2(w[0], w[1]), hi = make_ulonglong2(w[2], w[3]);      // (zero above the depth)
    ulonglong2 *s = reinterpret_cast<ulonglong2 *>(snap_nodes + 32 * threadIdx.x);
    s[0] = lo; s[1] = hi;
    if (l > plan.depth) return;
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(nodes + 32 * (plan.off[l] + plan.size[l] - 1));
    o[0] = lo; o[1] = hi;
}

}  // namespace

hipError_t zk_tree_leaf_hashes(const uint8_t *d_records, uint64_t count, uint8_t *d_out, const poseidon2::Params *p2, hipStream_t st) {
    if (count == 0) return hipSuccess;
    if (count > zk_tree::MAX_LEAVES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_leaf_hash_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const u64 *)d_records, count, d_out, p2);
    return hipGetLastError();
}

hipError_t zk_tree_reduce(uint8_t *d_nodes, const zk_tree::Plan &plan, uint32_t *d_bad_leaf, const poseidon2::Params *p2, hipStream_t st) {
    if (plan.depth == 0 || plan.depth > zk_tree::MAX_DEPTH || plan.count > zk_tree::MAX_LEAVES) return hipErrorInvalidValue;
    for (u32 l = 0; l < plan.depth; l++) {
        const u64 n_out = plan.size[l + 1];
        if (n_out <= 256) {                      // this level and all above it (they only shrink) fit one workgroup
            hipLaunchKernelGGL(zk_top_kernel, dim3(1), dim3(256), 0, st, d_nodes, plan, l, d_bad_leaf, p2);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(zk_node_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, d_nodes + 32 * plan.off[l], plan.size[l],
                           d_nodes + 32 * plan.off[l + 1], n_out, l == 0 ? d_bad_leaf : nullptr, p2);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t zk_tree_open_paths(const uint8_t *d_nodes, const zk_tree::Plan &plan, const uint64_t *d_indices, uint64_t n, uint8_t *d_siblings,
                              uint8_t *d_positions, hipStream_t st) {
    const u64 threads = n * plan.depth;
    if (threads == 0) return hipSuccess;
    if ((threads + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_open_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_nodes, plan, d_indices, n, d_siblings, d_positions);
    return hipGetLastError();
}

hipError_t zk_tree_check_leaves(const uint8_t *d_nodes, const zk_tree::Plan &plan, uint64_t first, uint64_t k, uint32_t *d_bad_leaf, hipStream_t st) {
    if (k == 0) return hipSuccess;
    if (first > zk_tree::MAX_LEAVES || k > zk_tree::MAX_LEAVES - first) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_leaf_check_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, d_nodes + 32 * plan.off[0], first, k, d_bad_leaf);
    return hipGetLastError();
}

hipError_t zk_tree_rehash(uint8_t *d_nodes, const zk_tree::Plan &grown, uint64_t n_old, const uint32_t *d_bad_leaf, uint8_t *d_snap_nodes,
                          const poseidon2::Params *p2, hipStream_t st) {
    if (grown.depth == 0 || grown.depth > zk_tree::MAX_DEPTH || grown.count > zk_tree::MAX_LEAVES || n_old >= grown.count) return hipErrorInvalidValue;
    for (u32 l = 0; l < grown.depth; l++) {
        u64 first, cnt;
        zk_tree::dirty_range(n_old, grown.count - n_old, l + 1, first, cnt);
        if (cnt <= 256) {                        // this level's dirty range and all above it (they only shrink) fit one workgroup
            hipLaunchKernelGGL(zk_append_top_kernel, dim3(1), dim3(256), 0, st, d_nodes, grown, l, n_old, d_bad_leaf, d_snap_nodes, p2);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(zk_node_range_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, d_nodes + 32 * grown.off[l], grown.size[l],
                           d_nodes + 32 * grown.off[l + 1], first, cnt, d_bad_leaf, p2);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipErrorInvalidValue;                 // not reached: level `depth` has one node
}

hipError_t zk_tree_gather_snapshot(const uint8_t *d_nodes, const zk_tree::Plan &plan, uint8_t *d_snap_nodes, hipStream_t st) {
    if (plan.depth == 0 || plan.depth > zk_tree::MAX_DEPTH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_snapshot_kernel, dim3(1), dim3(64), 0, st, d_nodes, plan, d_snap_nodes);
    return hipGetLastError();
}

hipError_t zk_tree_open_paths_at(const uint8_t *d_nodes, const zk_tree::Plan &plan, const zk_tree::Snapshot &snap, const uint64_t *d_indices,
                                 uint64_t n, uint8_t *d_siblings, uint8_t *d_positions, hipStream_t st) {
    const u64 threads = n * plan.depth;
    if (threads == 0) return hipSuccess;
    if ((threads + 255) / 256 > 0x7FFFFFFFull || snap.count == 0 || snap.count > plan.count || snap.depth != plan.depth) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_open_at_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_nodes, plan, snap, d_indices, n, d_siblings,
                       d_positions);
    return hipGetLastError();
}

hipError_t zk_tree_derive_snapshots(const uint8_t *d_nodes, const zk_tree::Plan &plan, const uint64_t *d_counts, uint64_t m, zk_tree::Snapshot *d_out,
                                    const poseidon2::Params *p2, hipStream_t st) {
    if (m == 0) return hipSuccess;
    if (plan.depth == 0 || plan.depth > zk_tree::MAX_DEPTH || plan.count == 0 || plan.count > zk_tree::MAX_LEAVES || (m + 63) / 64 > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_snapshots_at_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, d_nodes, plan, d_counts, m, d_out, p2);
    return hipGetLastError();
}

hipError_t zk_tree_open_paths_at_many(const uint8_t *d_nodes, const zk_tree::Plan &plan, const zk_tree::Snapshot *d_snaps, uint64_t m,
                                      const uint32_t *d_snap_of, const uint64_t *d_indices, uint64_t n, uint8_t *d_siblings, uint8_t *d_positions,
                                      uint8_t *d_roots, hipStream_t st) {
    const u64 threads = n * plan.depth;
    if (threads == 0) return hipSuccess;
    if ((threads + 255) / 256 > 0x7FFFFFFFull || m == 0 || m > 0xFFFFFFFFull || plan.depth > zk_tree::MAX_DEPTH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_open_at_many_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_nodes, plan, d_snaps, d_snap_of, d_indices,
                       n, d_siblings, d_positions, d_roots);
    return hipGetLastError();
}

hipError_t zk_tree_place_snapshot(uint8_t *d_nodes, const zk_tree::Plan &cut, const zk_tree::Snapshot *d_snap, uint8_t *d_snap_nodes, hipStream_t st) {
    if (cut.depth == 0 || cut.depth > zk_tree::MAX_DEPTH || cut.count == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zk_place_snapshot_kernel, dim3(1), dim3(64), 0, st, d_nodes, cut, d_snap, d_snap_nodes);
    return hipGetLastError();
}
