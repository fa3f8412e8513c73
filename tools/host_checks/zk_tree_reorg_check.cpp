// zk_tree_reorg_check.cpp — the host side of the device ZK tree at earlier counts and through reorgs (csrc/zk_tree.hpp: last_node, the
// checks behind qpgpu_zk_tree_snapshots_at / _open_at_counts / _truncate), stand-alone and without a GPU, meant to be built with
// -fsanitize=address,undefined. last_node is checked against a brute-force model (the level sizes by repeated grouping, the children
// counted one by one), and the derivation of zk_snapshots_at_kernel and the truncate of zk_place_snapshot_kernel are replayed through
// last_node alone on a model tree over a stand-in hash, whose storage beyond the live sizes holds stale nodes, and compared with fresh
// builds. Built and run by tests/test_zk_tree_reorg_plan.py.
#define ZK_TREE_PLAN_ONLY
#include <cstdio>
#include <cstring>
#include <vector>
#include "zk_tree.hpp"

using namespace zk_tree;
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

// ---- last_node against brute force ----
static void check_last_node(uint64_t n, unsigned depth) {
    std::vector<uint64_t> size(depth + 1);
    size[0] = n;
    for (unsigned l = 1; l <= depth; l++) size[l] = (size[l - 1] + 3) / 4;               // repeated grouping
    for (unsigned l = 1; l <= depth; l++) {
        const LastNode r = last_node(n, l);
        const uint64_t i = size[l] - 1;
        uint32_t children = 0;
        int32_t computed = -1;
        for (uint32_t s = 0; s < 4; s++) {
            const uint64_t c = 4 * i + s;
            if (c >= size[l - 1]) continue;
            EXPECT(s == children);                                                       // the existing children are the first slots
            children++;
            if (l - 1 >= 1 && c == size[l - 1] - 1) computed = (int32_t)s;               // the last node of the level below
        }
        EXPECT(r.index == i && r.children == children && r.computed == computed && children >= 1);
        EXPECT(l == 1 ? computed == -1 : computed == (int32_t)children - 1);
        EXPECT(size[l] == level_size(n, l));
    }
}

// ---- a model tree: nodes are words, the hash a stand-in that depends on the order and on every child ----
static uint64_t mix(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint64_t v : {a, b, c, d}) { h ^= v + 0x7F4A7C15ull; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 29; }
    return h | 1;                                                                        // never the empty hash
}
static uint64_t child(const std::vector<uint64_t> &nodes, const Plan &p, unsigned l, uint64_t i) { return i < p.size[l] ? nodes[p.off[l] + i] : 0; }
static void hash_range(std::vector<uint64_t> &nodes, const Plan &p, unsigned l, uint64_t first, uint64_t cnt) {      // parents of level l + 1
    for (uint64_t g = first; g < first + cnt; g++)
        nodes[p.off[l + 1] + g] = mix(child(nodes, p, l, 4 * g), child(nodes, p, l, 4 * g + 1), child(nodes, p, l, 4 * g + 2), child(nodes, p, l, 4 * g + 3));
}
static std::vector<uint64_t> fresh(const std::vector<uint64_t> &leaves, uint64_t count, unsigned depth, Plan &p) {
    EXPECT(make_plan(count, depth, 0, p) == nullptr);
    std::vector<uint64_t> nodes(p.total());
    for (uint64_t i = 0; i < count; i++) nodes[i] = leaves[i];
    for (unsigned l = 0; l < depth; l++) hash_range(nodes, p, l, 0, p.size[l + 1]);
    return nodes;
}
// zk_snapshots_at_kernel: the last node of every level at count n, out of the tree `p` (n <= p.count) through last_node alone. Every
// read is checked to lie below the live size of its level.
static void derive(const std::vector<uint64_t> &nodes, const Plan &p, uint64_t n, uint64_t last[MAX_DEPTH]) {
    uint64_t cur = 0;
    for (unsigned l = 1; l <= p.depth; l++) {
        const LastNode r = last_node(n, l);
        uint64_t c[4];
        for (uint32_t s = 0; s < 4; s++) {
            if (s >= r.children) c[s] = 0;
            else if ((int32_t)s == r.computed) c[s] = cur;
            else { EXPECT(4 * r.index + s < p.size[l - 1]); c[s] = nodes[p.off[l - 1] + 4 * r.index + s]; }
        }
        last[l - 1] = cur = mix(c[0], c[1], c[2], c[3]);
    }
    for (unsigned l = p.depth; l < MAX_DEPTH; l++) last[l] = 0;
}
static void append(std::vector<uint64_t> &nodes, Plan &p, uint64_t capacity, const std::vector<uint64_t> &leaves, uint64_t k) {
    const uint64_t n = p.count;
    Plan grown;
    EXPECT(make_plan_reserved(n + k, capacity, p.depth, 0, grown) == nullptr);
    for (uint64_t j = 0; j < k; j++) nodes[n + j] = leaves[n + j];
    for (unsigned l = 0; l < p.depth; l++) { uint64_t first, cnt; dirty_range(n, k, l + 1, first, cnt); hash_range(nodes, grown, l, first, cnt); }
    p = grown;
}
static void expect_fresh(const std::vector<uint64_t> &nodes, const Plan &p, const std::vector<uint64_t> &leaves) {
    Plan q;
    const std::vector<uint64_t> want = fresh(leaves, p.count, p.depth, q);
    for (unsigned l = 0; l <= p.depth; l++) {
        EXPECT(p.size[l] == q.size[l]);
        for (uint64_t i = 0; i < p.size[l] && i < q.size[l]; i++) EXPECT(nodes[p.off[l] + i] == want[q.off[l] + i]);
    }
}

// a tree grown to `capacity` in `step`s: the snapshot derived at every count equals the last nodes of a fresh tree of that many leaves
static void check_derivation(uint64_t capacity, unsigned depth, uint64_t step) {
    std::vector<uint64_t> leaves(capacity);
    for (uint64_t i = 0; i < capacity; i++) leaves[i] = mix(i, capacity, depth, 11);
    Plan p;
    EXPECT(make_plan_reserved(1, capacity, depth, 0, p) == nullptr);
    std::vector<uint64_t> nodes(p.total(), 0xDEADull);
    nodes[0] = leaves[0];
    for (unsigned l = 0; l < p.depth; l++) hash_range(nodes, p, l, 0, 1);
    while (p.count < capacity) append(nodes, p, capacity, leaves, step < capacity - p.count ? step : capacity - p.count);
    for (uint64_t n = 1; n <= capacity; n++) {
        uint64_t last[MAX_DEPTH];
        derive(nodes, p, n, last);
        Plan q;
        const std::vector<uint64_t> want = fresh(leaves, n, p.depth, q);
        for (unsigned l = 1; l <= p.depth; l++) EXPECT(last[l - 1] == want[q.off[l] + q.size[l] - 1]);
        for (unsigned l = p.depth; l < MAX_DEPTH; l++) EXPECT(last[l] == 0);
    }
}

// fork A to a_count, truncate to cut (the derived snapshot placed over the last node of every level at the sizes of `cut`), fork B of
// other leaves to b_count: after each step the tree equals a fresh one; a snapshot of fork A above the cut no longer matches
static void check_reorg(uint64_t capacity, unsigned depth, uint64_t a_count, uint64_t cut, uint64_t b_count) {
    std::vector<uint64_t> fork_a(capacity), fork_b(capacity);
    for (uint64_t i = 0; i < capacity; i++) { fork_a[i] = mix(i, capacity, depth, 1); fork_b[i] = i < cut ? fork_a[i] : mix(i, capacity, depth, 2); }
    Plan p;
    EXPECT(make_plan_reserved(1, capacity, depth, 0, p) == nullptr);
    std::vector<uint64_t> nodes(p.total(), 0xDEADull);
    nodes[0] = fork_a[0];
    for (unsigned l = 0; l < p.depth; l++) hash_range(nodes, p, l, 0, 1);
    append(nodes, p, capacity, fork_a, a_count - 1);
    expect_fresh(nodes, p, fork_a);
    const uint64_t kept_at = cut + (a_count - cut + 1) / 2;                                // a block of fork A above the cut
    uint64_t kept[MAX_DEPTH], again[MAX_DEPTH];
    derive(nodes, p, kept_at, kept);
    // truncate
    EXPECT(check_truncate(p, cut) == nullptr);
    uint64_t last[MAX_DEPTH];
    derive(nodes, p, cut, last);
    Plan shorter;
    EXPECT(make_plan_reserved(cut, capacity, p.depth, 0, shorter) == nullptr && std::memcmp(shorter.off, p.off, sizeof p.off) == 0);
    for (unsigned l = 1; l <= p.depth; l++) nodes[shorter.off[l] + shorter.size[l] - 1] = last[l - 1];
    p = shorter;
    expect_fresh(nodes, p, fork_a);
    for (uint64_t n = 1; n <= cut; n++) {                                                // earlier counts still derive
        derive(nodes, p, n, again);
        Plan q;
        const std::vector<uint64_t> want = fresh(fork_a, n, p.depth, q);
        EXPECT(again[p.depth - 1] == want[q.off[p.depth]]);
    }
    // fork B, in two appends
    if (b_count > cut) {
        append(nodes, p, capacity, fork_b, (b_count - cut + 1) / 2);
        expect_fresh(nodes, p, fork_b);
        if (p.count < b_count) append(nodes, p, capacity, fork_b, b_count - p.count);
        expect_fresh(nodes, p, fork_b);
        if (kept_at > cut && kept_at <= p.count) {
            derive(nodes, p, kept_at, again);
            EXPECT(again[p.depth - 1] != kept[p.depth - 1] && std::memcmp(again, kept, sizeof kept) != 0);
        }
    }
    // a truncate to the count itself changes nothing
    const std::vector<uint64_t> before = nodes;
    derive(nodes, p, p.count, last);
    for (unsigned l = 1; l <= p.depth; l++) nodes[p.off[l] + p.size[l] - 1] = last[l - 1];
    EXPECT(nodes == before);
}

int main() {
    // last_node: every n <= 4^4 + 2 at depths 1 .. 5 (where the depth holds n), depth 16 for small n, the 2^24 bound
    for (unsigned depth = 1; depth <= 5; depth++)
        for (uint64_t n = 1; n <= 258; n++)
            if ((1ull << (2 * depth)) >= n) check_last_node(n, depth);
    for (uint64_t n = 1; n <= 70; n++) check_last_node(n, MAX_DEPTH);
    for (uint64_t n : {MAX_LEAVES - 1, MAX_LEAVES, (uint64_t)(1 << 20), (uint64_t)(1 << 20) + 1, (uint64_t)4097}) check_last_node(n, MAX_DEPTH);
    LastNode r = last_node(1, 1); EXPECT(r.index == 0 && r.children == 1 && r.computed == -1);
    r = last_node(1, 2); EXPECT(r.index == 0 && r.children == 1 && r.computed == 0);
    r = last_node(16, 2); EXPECT(r.index == 0 && r.children == 4 && r.computed == 3);
    r = last_node(17, 2); EXPECT(r.index == 1 && r.children == 1 && r.computed == 0);
    r = last_node(17, 1); EXPECT(r.index == 4 && r.children == 1 && r.computed == -1);
    r = last_node(70, 1); EXPECT(r.index == 17 && r.children == 2 && r.computed == -1);
    r = last_node(70, 3); EXPECT(r.index == 1 && r.children == 1 && r.computed == 0);

    // the derivation and the reorg on the model tree
    check_derivation(70, 4, 1); check_derivation(70, 4, 13); check_derivation(258, 0, 7); check_derivation(258, 5, 100);
    check_derivation(6, MAX_DEPTH, 1); check_derivation(1, 0, 1); check_derivation(4, 1, 1); check_derivation(17, MAX_DEPTH, 5);
    check_reorg(70, 4, 50, 20, 55); check_reorg(70, 4, 70, 1, 70); check_reorg(70, 4, 65, 64, 70); check_reorg(70, 4, 17, 16, 17);
    check_reorg(300, 0, 300, 5, 290); check_reorg(20, MAX_DEPTH, 20, 4, 19); check_reorg(70, 4, 50, 50, 50);
    for (uint64_t cut = 1; cut <= 40; cut++) check_reorg(40, 3, 40, cut, 40);

    // the checks
    Plan p;
    EXPECT(make_plan_reserved(65, 100, 0, 0, p) == nullptr && p.depth == 4);
    std::vector<uint64_t> counts = {1, 65, 40, 40, 64};
    uint64_t at = 99;
    EXPECT(check_counts(p, counts.data(), counts.size(), &at) == nullptr && at == 99);
    EXPECT(check_counts(p, nullptr, 0, &at) == nullptr && check_counts(p, nullptr, ~0ull, &at) != nullptr && at == 99);
    counts[3] = 66;                                                                      // within the capacity, above the count
    EXPECT(check_counts(p, counts.data(), counts.size(), &at) != nullptr && at == 3 && check_counts(p, counts.data(), 3, &at) == nullptr);
    counts[1] = 0;
    EXPECT(check_counts(p, counts.data(), counts.size(), &at) != nullptr && at == 1 && check_counts(p, counts.data(), counts.size(), nullptr) != nullptr);
    counts[1] = ~0ull;
    EXPECT(check_counts(p, counts.data(), counts.size(), &at) != nullptr && at == 1);

    counts = {1, 65, 40, 40, 64};
    std::vector<uint64_t> idx = {0, 64, 39, 0, 63};
    at = 99;
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) == nullptr && at == 99);
    EXPECT(check_open_at_counts(p, nullptr, nullptr, 0, &at) == nullptr && check_open_at_counts(p, nullptr, nullptr, SIZE_MAX, &at) != nullptr && at == 99);
    EXPECT(check_open_at_counts(p, nullptr, nullptr, (uint64_t)SIZE_MAX / (PATH_LEVEL_BYTES * MAX_DEPTH) + 1, &at) != nullptr);      // check_open_at's guard
    idx[2] = 40;                                                                         // a leaf of the tree, not of the tree at that count
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) != nullptr && at == 2);
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), 2, &at) == nullptr);
    idx[0] = 1;                                                                          // the index equal to its count
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) != nullptr && at == 0);
    idx = {0, 64, 39, 0, 63}; counts[4] = 0;
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) != nullptr && at == 4);
    counts[4] = 66; idx[4] = 65;
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) != nullptr && at == 4);
    counts[4] = 64; idx[4] = ~0ull;
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), &at) != nullptr && at == 4);
    EXPECT(check_open_at_counts(p, counts.data(), idx.data(), idx.size(), nullptr) != nullptr);

    EXPECT(check_truncate(p, 0) != nullptr && check_truncate(p, 66) != nullptr && check_truncate(p, 100) != nullptr && check_truncate(p, ~0ull) != nullptr);
    EXPECT(check_truncate(p, 1) == nullptr && check_truncate(p, 64) == nullptr && check_truncate(p, 65) == nullptr);
    EXPECT(sizeof(Snapshot) == 528 && sizeof(LastNode) == 16);
    std::printf("zk tree reorg: failures %d\n", bad);
    return bad != 0;
}
