// zk_tree_plan_check.cpp — the host side of the device ZK tree (csrc/zk_tree.hpp: level sizes and offsets, the depth bounds, the range
// and index checks of qpgpu_zk_tree_read_level / qpgpu_zk_tree_open), stand-alone and without a GPU, meant to be built with
// -fsanitize=address,undefined: every level of every plan is walked node range by node range against a brute-force count, the extremes
// (count = 2^24, depth 16, a single leaf) included. Built and run by tests/test_zk_tree_plan.py.
#define ZK_TREE_PLAN_ONLY
#include <cstdio>
#include <cstring>
#include <vector>
#include "zk_tree.hpp"

using namespace zk_tree;
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

// the levels by repeated grouping, the way the reference's test builder folds them
static void check_plan(uint64_t count, unsigned depth_in) {
    Plan p;
    const char *why = make_plan(count, depth_in, 0, p);
    EXPECT(why == nullptr);
    if (why) return;
    const unsigned depth = p.depth;
    EXPECT(depth >= 1 && depth <= MAX_DEPTH && (1ull << (2 * depth)) >= count);
    if (depth_in == 0) EXPECT(depth == 1 || (1ull << (2 * (depth - 1))) < count);       // the smallest valid depth
    else EXPECT(depth == depth_in);
    uint64_t n = count, at = 0;
    for (unsigned l = 0; l <= depth; l++) {
        EXPECT(p.size[l] == n && p.off[l] == at && n >= 1);
        EXPECT(check_range(p, l, 0, n) == nullptr && check_range(p, l, n, 0) == nullptr);
        EXPECT(check_range(p, l, 0, n + 1) != nullptr && check_range(p, l, n, 1) != nullptr && check_range(p, l, n + 1, 0) != nullptr);
        EXPECT(check_range(p, l, 1, ~0ull) != nullptr);                                  // first + n wraps
        at += n; n = (n + 3) / 4;
    }
    EXPECT(p.size[depth] == 1 && p.total() == at && check_range(p, depth + 1, 0, 0) != nullptr);
    EXPECT(p.total() * NODE_BYTES / NODE_BYTES == p.total());
    // a path's ancestors stay inside their levels, for the first, the last and a middle leaf
    for (uint64_t leaf : {(uint64_t)0, count / 2, count - 1})
        for (unsigned l = 0; l < depth; l++) {
            const uint64_t idx = leaf >> (2 * l);
            EXPECT(idx < p.size[l] && (idx >> 2) < p.size[l + 1]);
        }
}

int main() {
    // depth bounds
    EXPECT(min_depth(1) == 1 && min_depth(4) == 1 && min_depth(5) == 2 && min_depth(16) == 2 && min_depth(17) == 3);
    EXPECT(min_depth(MAX_LEAVES) == 12 && min_depth(1ull << 32) == 16 && min_depth((1ull << 32) + 1) == 0);
    Plan p;
    EXPECT(make_plan(0, 0, 0, p) != nullptr && make_plan(MAX_LEAVES + 1, 0, 0, p) != nullptr && make_plan(~0ull, 0, 0, p) != nullptr);
    EXPECT(make_plan(1, 17, 0, p) != nullptr && make_plan(1, ~0u, 0, p) != nullptr);
    EXPECT(make_plan(5, 1, 0, p) != nullptr && make_plan(17, 2, 0, p) != nullptr && make_plan(MAX_LEAVES, 11, 0, p) != nullptr);
    EXPECT(make_plan(4, 1, 2, p) != nullptr && make_plan(4, 1, ~0u, p) != nullptr && make_plan(4, 1, FLAG_FROM_TRANSFERS, p) == nullptr);
    // level sizes and offsets: every count up to a few groups past 4^5, the group boundaries above that, the largest tree
    for (uint64_t count = 1; count <= 1100; count++) check_plan(count, 0);
    for (unsigned k = 5; k <= 12; k++)
        for (int64_t d = -2; d <= 2; d++) {
            const uint64_t count = (uint64_t)((int64_t)(1ull << (2 * k)) + d);
            if (count >= 1 && count <= MAX_LEAVES) { check_plan(count, 0); check_plan(count, MAX_DEPTH); }
        }
    for (unsigned depth = 1; depth <= MAX_DEPTH; depth++) { check_plan(1, depth); check_plan(3, depth); }
    for (unsigned depth = 2; depth <= MAX_DEPTH; depth++) check_plan(5, depth);
    check_plan(MAX_LEAVES, 0); check_plan(MAX_LEAVES, 12); check_plan(MAX_LEAVES, 16); check_plan(MAX_LEAVES - 1, 13);
    EXPECT(make_plan(MAX_LEAVES, 16, 0, p) == nullptr && p.total() == 22369621 + 4 && p.off[12] == 22369620 && p.total() * NODE_BYTES < (1ull << 30));
    // indices
    EXPECT(make_plan(65, 0, 0, p) == nullptr);
    std::vector<uint64_t> idx = {0, 64, 3, 64, 0};
    uint64_t at = 99;
    EXPECT(check_open(p, idx.data(), idx.size(), &at) == nullptr && at == 99);
    idx[3] = 65;
    EXPECT(check_open(p, idx.data(), idx.size(), &at) != nullptr && at == 3);
    idx[1] = ~0ull;
    EXPECT(check_open(p, idx.data(), idx.size(), &at) != nullptr && at == 1 && check_open(p, idx.data(), 1, nullptr) == nullptr);
    EXPECT(check_open(p, idx.data(), 0, nullptr) == nullptr && check_open(p, nullptr, SIZE_MAX, nullptr) != nullptr);
    std::printf("zk tree plan: failures %d\n", bad);
    return bad != 0;
}
