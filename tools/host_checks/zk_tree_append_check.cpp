// zk_tree_append_check.cpp — the host side of the append-only device ZK tree (csrc/zk_tree.hpp: the reserved plan, the dirty range of an
// append, the checks behind qpgpu_zk_tree_append / qpgpu_zk_tree_open_at), stand-alone and without a GPU, meant to be built with
// -fsanitize=address,undefined. Reserved plans are checked against repeated grouping, dirty ranges against brute force (a node is dirty
// iff its leaf range meets the appended one), and a model tree over a stand-in hash is appended to through make_plan_reserved and
// dirty_range alone and compared, node by node, with fresh builds; the snapshot substitution of zk_open_at_kernel is replayed on it.
// Built and run by tests/test_zk_tree_append_plan.py.
#define ZK_TREE_PLAN_ONLY
#include <cstdio>
#include <cstring>
#include <vector>
#include "zk_tree.hpp"

using namespace zk_tree;
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

static void check_reserved(uint64_t count, uint64_t capacity, unsigned depth_in) {
    Plan p;
    const char *why = make_plan_reserved(count, capacity, depth_in, 0, p);
    EXPECT(why == nullptr);
    if (why) return;
    const unsigned depth = p.depth;
    EXPECT(depth >= 1 && depth <= MAX_DEPTH && (1ull << (2 * depth)) >= capacity && p.count == count);
    if (depth_in == 0) EXPECT(depth == 1 || (1ull << (2 * (depth - 1))) < capacity);      // the smallest depth that holds the capacity
    else EXPECT(depth == depth_in);
    uint64_t n = count, room = capacity, at = 0;
    for (unsigned l = 0; l <= depth; l++) {
        EXPECT(p.size[l] == n && p.off[l] == at && n >= 1 && n <= room);
        EXPECT(check_range(p, l, 0, n) == nullptr && check_range(p, l, n, 1) != nullptr);
        at += room; n = (n + 3) / 4; room = (room + 3) / 4;
    }
    EXPECT(p.size[depth] == 1 && p.total() == at && p.total() * NODE_BYTES / NODE_BYTES == p.total());
    if (count == capacity) {                                                             // make_plan's plan, word for word
        Plan q;
        EXPECT(make_plan(count, depth, 0, q) == nullptr && std::memcmp(&p, &q, sizeof p) == 0);
    }
    Plan full;                                                                           // an append never moves a node
    EXPECT(make_plan_reserved(capacity, capacity, depth, 0, full) == nullptr && std::memcmp(p.off, full.off, sizeof p.off) == 0);
}

// level `level` of a tree that grew from n to n + k leaves, inside storage for `capacity`
static void check_dirty(uint64_t n, uint64_t k, unsigned level, uint64_t capacity) {
    uint64_t first, cnt;
    dirty_range(n, k, level, first, cnt);
    const uint64_t span = 1ull << (2 * level), nodes = level_size(n + k, level);
    EXPECT(cnt >= 1 && first + cnt == nodes && first + cnt <= level_size(capacity, level));
    for (uint64_t i = 0; i < nodes; i++) {
        const bool meets = i * span < n + k && (i + 1) * span > n;                       // [i span, (i + 1) span) meets [n, n + k)
        EXPECT(meets == (i >= first && i < first + cnt));
        if (meets != (i >= first && i < first + cnt)) return;
    }
    // what is not dirty existed before, whole: its leaf range ends at or below n
    EXPECT(first <= level_size(n, level) && first * span <= n);
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
// node i of level l as zk_open_at_kernel reads it at a snapshot
static uint64_t node_at(const std::vector<uint64_t> &nodes, const Plan &p, uint64_t snap_count, const uint64_t *last, unsigned l, uint64_t i) {
    const uint64_t n_l = level_size(snap_count, l);
    if (i >= n_l) return 0;
    if (l >= 1 && i == n_l - 1) return last[l - 1];
    return nodes[p.off[l] + i];
}

static void check_model(uint64_t capacity, unsigned depth, const std::vector<uint64_t> &steps) {
    std::vector<uint64_t> leaves(capacity);
    for (uint64_t i = 0; i < capacity; i++) leaves[i] = mix(i, capacity, depth, 7);
    Plan p;
    EXPECT(make_plan_reserved(1, capacity, depth, 0, p) == nullptr);
    depth = p.depth;
    std::vector<uint64_t> nodes(p.total(), 0xDEADull);                                   // stale storage must never be read
    nodes[0] = leaves[0];
    for (unsigned l = 0; l < depth; l++) hash_range(nodes, p, l, 0, 1);
    struct Snap { uint64_t count; uint64_t last[MAX_DEPTH]; };
    std::vector<Snap> snaps;
    auto take = [&]() { Snap s{p.count, {0}}; for (unsigned l = 1; l <= depth; l++) s.last[l - 1] = nodes[p.off[l] + p.size[l] - 1]; snaps.push_back(s); };
    take();
    size_t step = 0;
    while (p.count < capacity) {
        const uint64_t n = p.count;
        uint64_t k = steps.empty() ? 1 : steps[step++ % steps.size()];
        if (k > capacity - n) k = capacity - n;
        EXPECT(check_append(p, capacity, true, k, 0) == nullptr);
        Plan grown;
        EXPECT(make_plan_reserved(n + k, capacity, depth, 0, grown) == nullptr);
        for (uint64_t j = 0; j < k; j++) nodes[n + j] = leaves[n + j];
        for (unsigned l = 0; l < depth; l++) { uint64_t first, cnt; dirty_range(n, k, l + 1, first, cnt); hash_range(nodes, grown, l, first, cnt); }
        p = grown;
        Plan q;
        const std::vector<uint64_t> want = fresh(leaves, p.count, depth, q);
        for (unsigned l = 0; l <= depth; l++)
            for (uint64_t i = 0; i < p.size[l]; i++) EXPECT(nodes[p.off[l] + i] == want[q.off[l] + i]);
        take();
    }
    // every earlier tree read through its snapshot out of the final one
    for (const Snap &s : snaps) {
        Plan q;
        const std::vector<uint64_t> want = fresh(leaves, s.count, depth, q);
        EXPECT(s.last[depth - 1] == want[q.off[depth]]);
        for (unsigned l = 0; l <= depth; l++)
            for (uint64_t i = 0; i < q.size[l] + 4; i++)
                EXPECT(node_at(nodes, p, s.count, s.last, l, i) == (i < q.size[l] ? want[q.off[l] + i] : 0));
    }
}

int main() {
    Plan p;
    // reserved plans: refusals, every (count, capacity) up to 300, the 2^24 bounds
    EXPECT(make_plan_reserved(0, 4, 0, 0, p) != nullptr && make_plan_reserved(5, 4, 0, 0, p) != nullptr && make_plan_reserved(1, 0, 0, 0, p) != nullptr);
    EXPECT(make_plan_reserved(1, MAX_LEAVES + 1, 0, 0, p) != nullptr && make_plan_reserved(~0ull, ~0ull, 0, 0, p) != nullptr);
    EXPECT(make_plan_reserved(MAX_LEAVES + 1, MAX_LEAVES + 1, 0, 0, p) != nullptr);
    EXPECT(make_plan_reserved(1, 5, 1, 0, p) != nullptr && make_plan_reserved(4, 17, 2, 0, p) != nullptr && make_plan_reserved(1, MAX_LEAVES, 11, 0, p) != nullptr);
    EXPECT(make_plan_reserved(1, 4, 17, 0, p) != nullptr && make_plan_reserved(1, 4, ~0u, 0, p) != nullptr);
    EXPECT(make_plan_reserved(1, 4, 1, 2, p) != nullptr && make_plan_reserved(1, 4, 1, FLAG_FROM_TRANSFERS, p) == nullptr);
    EXPECT(make_plan_reserved(1, 5, 0, 0, p) == nullptr && p.depth == 2 && make_plan_reserved(1, 1, 0, 0, p) == nullptr && p.depth == 1);
    for (uint64_t capacity = 1; capacity <= 300; capacity++)
        for (uint64_t count = 1; count <= capacity; count++) check_reserved(count, capacity, 0);
    for (uint64_t count : {1ull, 5ull, 70ull})
        for (unsigned depth = 4; depth <= MAX_DEPTH; depth++) check_reserved(count, 70, depth);
    for (uint64_t count : {(uint64_t)1, (uint64_t)4097, MAX_LEAVES - 1, MAX_LEAVES})
        for (unsigned depth : {0u, 12u, 16u}) check_reserved(count, MAX_LEAVES, depth);
    check_reserved(MAX_LEAVES - 1, MAX_LEAVES - 1, 0); check_reserved(1, MAX_LEAVES - 1, 13);
    EXPECT(make_plan_reserved(1, MAX_LEAVES, 16, 0, p) == nullptr && p.total() == 22369621 + 4 && p.off[12] == 22369620 && p.size[0] == 1 && p.size[12] == 1);

    // dirty ranges against brute force: every n + k <= 300 at every level up to 16, appends that reach 2^24
    for (uint64_t n = 1; n < 300; n++)
        for (uint64_t k = 1; n + k <= 300; k++)
            for (unsigned level = 0; level <= MAX_DEPTH; level++) check_dirty(n, k, level, 300);
    for (unsigned level = 0; level <= MAX_DEPTH; level++) {
        check_dirty(MAX_LEAVES - 1000, 1000, level, MAX_LEAVES); check_dirty(MAX_LEAVES - 1, 1, level, MAX_LEAVES);
        check_dirty(1, MAX_LEAVES - 1, level, MAX_LEAVES); check_dirty(1ull << 22, 3ull << 22, level, MAX_LEAVES);
    }
    uint64_t first, cnt;
    dirty_range(5, 1100, 1, first, cnt); EXPECT(first == 1 && cnt == 276);
    dirty_range(5, 1100, 2, first, cnt); EXPECT(first == 0 && cnt == 70);
    dirty_range(64, 1, 3, first, cnt); EXPECT(first == 1 && cnt == 1);                   // a full subtree is left alone
    dirty_range(64, 1, 4, first, cnt); EXPECT(first == 0 && cnt == 1);

    // the model tree: one leaf at a time up to 90 at the smallest depth and above it, then uneven steps
    check_model(90, 0, {}); check_model(90, 6, {}); check_model(70, 4, {1, 1, 1, 1, 11, 1, 1, 46, 1, 1}); check_model(300, 0, {7, 1, 64, 3, 129});
    check_model(4, 1, {}); check_model(1, 0, {}); check_model(17, MAX_DEPTH, {5});

    // appends
    EXPECT(make_plan_reserved(10, 20, 0, 0, p) == nullptr);
    EXPECT(check_append(p, 20, true, 1, 0) == nullptr && check_append(p, 20, true, 10, FLAG_FROM_TRANSFERS) == nullptr);
    EXPECT(check_append(p, 20, true, 0, 0) != nullptr && check_append(p, 20, true, 11, 0) != nullptr && check_append(p, 20, true, ~0ull, 0) != nullptr);
    EXPECT(check_append(p, 20, true, 1, 2) != nullptr && check_append(p, 20, true, 1, 0x80000000u) != nullptr);
    const char *unreserved = check_append(p, 10, false, 1, 0);
    EXPECT(unreserved != nullptr && std::strstr(unreserved, "qpgpu_zk_tree_build_reserved") != nullptr && check_append(p, 5, true, 1, 0) != nullptr);
    EXPECT(make_plan_reserved(20, 20, 0, 0, p) == nullptr && check_append(p, 20, true, 1, 0) != nullptr);

    // snapshots and indices
    EXPECT(make_plan_reserved(65, 100, 0, 0, p) == nullptr && p.depth == 4);
    std::vector<uint64_t> idx = {0, 39, 3, 39, 0};
    uint64_t at = 99;
    EXPECT(check_open_at(p, 40, 4, idx.data(), idx.size(), &at) == nullptr && at == 99);
    EXPECT(check_open_at(p, 65, 4, idx.data(), idx.size(), &at) == nullptr && check_open_at(p, 1, 4, idx.data(), 1, &at) == nullptr && at == 99);
    EXPECT(check_open_at(p, 0, 4, idx.data(), 0, &at) != nullptr && check_open_at(p, 66, 4, idx.data(), 0, &at) != nullptr && at == 99);
    EXPECT(check_open_at(p, ~0ull, 4, idx.data(), 0, &at) != nullptr && check_open_at(p, 40, 3, idx.data(), 0, &at) != nullptr);
    EXPECT(check_open_at(p, 40, 5, idx.data(), 0, &at) != nullptr && check_open_at(p, 40, 0, idx.data(), 0, &at) != nullptr && at == 99);
    idx[3] = 40;                                                                         // a leaf of the tree, not of the snapshot
    EXPECT(check_open_at(p, 40, 4, idx.data(), idx.size(), &at) != nullptr && at == 3 && check_open_at(p, 41, 4, idx.data(), idx.size(), &at) == nullptr);
    idx[1] = ~0ull;
    EXPECT(check_open_at(p, 40, 4, idx.data(), idx.size(), &at) != nullptr && at == 1 && check_open_at(p, 40, 4, idx.data(), 1, nullptr) == nullptr);
    EXPECT(check_open_at(p, 40, 4, nullptr, 0, nullptr) == nullptr && check_open_at(p, 40, 4, nullptr, SIZE_MAX, nullptr) != nullptr);
    EXPECT(sizeof(Snapshot) == 528);
    std::printf("zk tree append: failures %d\n", bad);
    return bad != 0;
}
