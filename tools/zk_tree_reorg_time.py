"""The resident ZK tree at earlier counts without kept snapshots, paths at many roots in one call, and a reorg, each against the route
that exists without them.

  zk_tree_reorg_time.py [--leaves N] [--capacity C] [--counts M] [--open P] [--roots D] [--block K] [--reps R] [--out profiles/zk_tree_reorg.txt]

A tree of N random canonical leaf hashes (default 2^20) with room for C (default 2^21; leaf.ZkTree(capacity=C), the smallest depth that
holds C). A host timer around every synchronous call, copies included; medians of R repetitions after a warm-up of every call.
  * snapshots_at: the snapshot at 1 count and at M random counts (default 1024) in one qpgpu_zk_tree_snapshots_at each.
  * open_at_counts: P paths (default 4096) over D distinct random counts (default 64), P / D random leaves per count, in one
    qpgpu_zk_tree_open_at_counts with the roots, against D calls of qpgpu_zk_tree_open_at with kept snapshots (P / D paths each; the
    snapshots are taken beforehand and are not timed).
  * truncate + append: qpgpu_zk_tree_truncate(N - K) followed by qpgpu_zk_tree_append of the last K leaves (default 4096), which leaves
    the tree as it was, against qpgpu_zk_tree_build_reserved of the same N leaves from scratch.
Before anything is printed the derived snapshots are compared with those of trees built from the first n leaves (three counts), the paths
and roots of the one call with those of the D calls, and the root after truncate + append with the rebuilt tree's. The kernels' share is
the library's profile regions (HIP events on the context's stream), taken in a second pass of the same calls. Prints one JSON line and
appends it, with the command, to --out. No GPU: it fails, it does not fall back."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=1 << 20)
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--counts", type=int, default=1024)
    ap.add_argument("--open", type=int, default=4096)
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.open % a.roots == 0 and a.block < a.leaves <= a.capacity
    pkg = ge.load_package()
    L = pkg.leaf
    rng = np.random.default_rng(412)
    leaves = rng.integers(0, 256, (a.leaves, 32), dtype=np.uint8)
    leaves[:, 7::8] &= 0x7F
    one = np.array([a.leaves - 12345 if a.leaves > 12345 else a.leaves], dtype=np.uint64)
    many = rng.integers(1, a.leaves + 1, a.counts).astype(np.uint64)
    per = a.open // a.roots
    root_counts = rng.choice(np.arange(a.leaves // 2, a.leaves + 1), a.roots, replace=False).astype(np.uint64)      # recent blocks
    path_counts = np.repeat(root_counts, per)
    path_idx = np.concatenate([rng.integers(0, int(c), per) for c in root_counts]).astype(np.uint64)
    shuffle = rng.permutation(a.open)                                          # a batch is not sorted by block
    path_counts, path_idx = path_counts[shuffle], path_idx[shuffle]
    cut = a.leaves - a.block
    med = lambda v: float(np.median(v))

    def timed(fn, reps):
        ms, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); ms.append(1e3 * (time.perf_counter() - t0))
        return ms, out

    def per_root(tree, kept):
        sib = np.empty((a.open, tree.depth, 3, 32), dtype=np.uint8); pos = np.empty((a.open, tree.depth), dtype=np.uint8)
        for c, snap in zip(root_counts, kept):
            mine = np.flatnonzero(path_counts == c)                            # (the split by block is the caller's work too)
            sib[mine], pos[mine] = tree.open(path_idx[mine], at=snap)
        return sib, pos

    def reorg(tree):
        t0 = time.perf_counter(); tree.truncate(cut); t1 = time.perf_counter(); tree.append(leaves[cut:]); t2 = time.perf_counter()
        return 1e3 * (t1 - t0), 1e3 * (t2 - t1)

    def calls(gpu, tree, kept, reps):
        r = {}
        r["snap1"], s1 = timed(lambda: tree.snapshots_at(one), reps)
        r["snapM"], sm = timed(lambda: tree.snapshots_at(many), reps)
        r["open_counts"], by_count = timed(lambda: tree.open(path_idx, at=path_counts, roots=True), reps)
        r["open_per_root"], by_root = timed(lambda: per_root(tree, kept), reps)
        both = [reorg(tree) for _ in range(reps)]
        r["truncate"], r["append"] = [b[0] for b in both], [b[1] for b in both]
        return r, s1, sm, by_count, by_root

    with pkg.QpGpu(0) as gpu:
        tree = L.ZkTree(gpu, leaves, capacity=a.capacity)
        depth = tree.depth
        kept = tree.snapshots_at(root_counts)
        calls(gpu, tree, kept, 1)                                              # warm-up: code objects, the parameter block
        L.ZkTree(gpu, leaves, capacity=a.capacity).close()
        r, s1, sm, by_count, by_root = calls(gpu, tree, kept, a.reps)
        rebuild_ms, rebuilt_root = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter(); rebuilt = L.ZkTree(gpu, leaves, capacity=a.capacity); rebuild_ms.append(1e3 * (time.perf_counter() - t0))
            rebuilt_root = rebuilt.root
            rebuilt.close()
        # equal results before any figure
        assert tree.leaf_count == a.leaves and tree.root == rebuilt_root, "the root after truncate + append differs from the rebuilt tree's"
        assert np.array_equal(by_count[0], by_root[0]) and np.array_equal(by_count[1], by_root[1]), "paths by count differ from the paths at kept snapshots"
        assert all(by_count[2][j].tobytes() == kept[int(np.flatnonzero(root_counts == path_counts[j])[0])].root for j in range(a.open)), "roots differ"
        for snap in (s1[0], sm[0], sm[-1]):
            with L.ZkTree(gpu, leaves[:snap.count], depth=depth) as old:
                assert bytes(snap) == bytes(old.snapshot()), "derived snapshot differs from the tree of its leaves"
        assert all(tree.check(s) for s in kept[:4])
        # the kernels alone
        gpu.profile(True)
        timed(lambda: tree.snapshots_at(one), a.reps)
        snap1_k = gpu.profile_read("zk_tree_snapshots_at")                     # (sums since the enable: the M counts are the difference)
        calls(gpu, tree, kept, a.reps)
        for _ in range(a.reps):
            L.ZkTree(gpu, leaves, capacity=a.capacity).close()
        k = {name: gpu.profile_read(name) for name in ("zk_tree_snapshots_at", "zk_tree_open_at_counts", "zk_tree_open_at", "zk_tree_truncate",
                                                       "zk_tree_append", "zk_tree_levels")}
        gpu.profile(False)
        tree.close()
    assert snap1_k[1] == a.reps and k["zk_tree_snapshots_at"][1] == 3 * a.reps and k["zk_tree_open_at_counts"][1] == a.reps
    assert k["zk_tree_open_at"][1] == a.roots * a.reps
    assert k["zk_tree_truncate"][1] == a.reps and k["zk_tree_append"][1] == a.reps and k["zk_tree_levels"][1] == a.reps
    snapM_k_ms = (k["zk_tree_snapshots_at"][0] - 2 * snap1_k[0]) / a.reps

    rnd = lambda v: [round(x, 3) for x in v]
    reorg_ms = [t + p for t, p in zip(r["truncate"], r["append"])]
    res = {"leaves": a.leaves, "capacity": a.capacity, "depth": depth, "reps": a.reps,
           "snapshots_at_1_ms": round(med(r["snap1"]), 3), "snapshots_at_1_all_ms": rnd(r["snap1"]),
           "counts": a.counts, "snapshots_at_counts_ms": round(med(r["snapM"]), 3), "snapshots_at_counts_all_ms": rnd(r["snapM"]),
           "snapshots_at_1_kernel_ms": round(snap1_k[0] / snap1_k[1], 4), "snapshots_at_counts_kernel_ms": round(snapM_k_ms, 4),
           "paths": a.open, "distinct_counts": a.roots,
           "open_at_counts_ms": round(med(r["open_counts"]), 3), "open_at_counts_all_ms": rnd(r["open_counts"]),
           "open_at_counts_kernels_ms": round(k["zk_tree_open_at_counts"][0] / k["zk_tree_open_at_counts"][1], 4),
           "open_at_per_root_calls_ms": round(med(r["open_per_root"]), 3), "open_at_per_root_calls_all_ms": rnd(r["open_per_root"]),
           "open_at_per_root_kernels_ms": round(a.roots * k["zk_tree_open_at"][0] / k["zk_tree_open_at"][1], 4),
           "per_root_over_one_call": round(med(r["open_per_root"]) / med(r["open_counts"]), 2),
           "block": a.block, "truncate_ms": round(med(r["truncate"]), 3), "truncate_all_ms": rnd(r["truncate"]),
           "truncate_kernels_ms": round(k["zk_tree_truncate"][0] / k["zk_tree_truncate"][1], 4),
           "append_ms": round(med(r["append"]), 3), "append_all_ms": rnd(r["append"]),
           "append_kernels_ms": round(k["zk_tree_append"][0] / k["zk_tree_append"][1], 4),
           "truncate_plus_append_ms": round(med(reorg_ms), 3),
           "rebuild_reserved_ms": round(med(rebuild_ms), 3), "rebuild_reserved_all_ms": rnd(rebuild_ms),
           "rebuild_levels_kernels_ms": round(k["zk_tree_levels"][0] / k["zk_tree_levels"][1], 4),
           "rebuild_over_truncate_plus_append": round(med(rebuild_ms) / med(reorg_ms), 1), "results_equal": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("  python tools/zk_tree_reorg_time.py --leaves %d --capacity %d --counts %d --open %d --roots %d --block %d --reps %d\n  %s\n"
                    % (a.leaves, a.capacity, a.counts, a.open, a.roots, a.block, a.reps, line))


if __name__ == "__main__":
    main()
