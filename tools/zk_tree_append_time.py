"""Appending a block to the resident ZK tree and opening paths at an earlier root, against rebuilding the tree.

  zk_tree_append_time.py [--leaves N] [--block K] [--open M] [--back B] [--reps R] [--out profiles/zk_tree_append.txt]

A tree of N - (B + R) K random canonical leaf hashes with room for N (default 4^10; leaf.ZkTree(capacity=N): qpgpu_zk_tree_build_reserved)
takes blocks of K leaves (default 1024) one qpgpu_zk_tree_append each, a host timer around the synchronous call, 32 K bytes of upload
included, up to N leaves: the last R are timed, and the snapshot that the paths are opened at is taken B appends (default 8) before the
end. M random leaves of the snapshot's tree (default 4096) are then opened at it in one call (qpgpu_zk_tree_open_at), R times. The rebuild of the same final leaf set
(qpgpu_zk_tree_build, the only route without the append) is timed R times in the same run. Before anything is printed the appended tree's
root and M of its paths are compared with the rebuilt tree's, and the snapshot's root and the paths opened at it with those of a tree
built from the snapshot's leaves alone. Medians of the repetitions after a warm-up of every call; the kernels' share is the library's
profile regions zk_tree_append / zk_tree_open_at / zk_tree_levels (HIP events on the context's stream), taken in a second pass of the
same appends. Prints one JSON line and appends it, with the command, to --out. No GPU: it fails, it does not fall back."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=4 ** 10)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--open", type=int, default=4096)
    ap.add_argument("--back", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    L = pkg.leaf
    rng = np.random.default_rng(411)
    leaves = rng.integers(0, 256, (a.leaves, 32), dtype=np.uint8)
    leaves[:, 7::8] &= 0x7F
    start = a.leaves - (a.back + a.reps) * a.block
    assert start >= 1, "the tree is too small for that many blocks"
    at_count = a.leaves - a.back * a.block                                     # the snapshot's leaves
    picks = rng.integers(0, at_count, a.open).astype(np.uint64)
    med = lambda v: float(np.median(v))

    def follow(gpu, timed, profile=False):
        """the chain from the snapshot's block to the last: (tree, snapshot, append times of the last R blocks)"""
        tree = L.ZkTree(gpu, leaves[:start], capacity=a.leaves)
        if profile:
            gpu.profile(True)                                                  # (behind the first build: its levels are no rebuild)
        snap, ms, n = None, [], start
        for b in range(a.back + a.reps):
            t0 = time.perf_counter(); after = tree.append(leaves[n:n + a.block]); t1 = time.perf_counter()
            n += a.block
            if n == at_count:
                snap = after
            if timed and b >= a.back:
                ms.append(1e3 * (t1 - t0))
        assert tree.leaf_count == a.leaves and snap is not None and snap.count == at_count
        return tree, snap, ms

    with pkg.QpGpu(0) as gpu:
        tree, snap, _ = follow(gpu, False)                                     # warm-up: code objects, the parameter block
        tree.open(picks, at=snap); tree.close()
        L.ZkTree(gpu, leaves).close()
        tree, snap, append_ms = follow(gpu, True)
        open_at_ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); sib_at, pos_at = tree.open(picks, at=snap); open_at_ms.append(1e3 * (time.perf_counter() - t0))
        rebuild_ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); rebuilt = L.ZkTree(gpu, leaves); rebuild_ms.append(1e3 * (time.perf_counter() - t0))
            rebuilt_root, rebuilt_paths = rebuilt.root, rebuilt.open(picks)
            rebuilt.close()
        # equal results before any figure
        assert tree.root == rebuilt_root, "appended root differs from the rebuilt tree's"
        sib, pos = tree.open(picks)
        assert np.array_equal(sib, rebuilt_paths[0]) and np.array_equal(pos, rebuilt_paths[1]), "appended paths differ from the rebuilt tree's"
        with L.ZkTree(gpu, leaves[:at_count], depth=tree.depth) as old:
            want = old.open(picks)
            assert snap.root == old.root, "snapshot root differs from the tree of the snapshot's leaves"
            assert np.array_equal(sib_at, want[0]) and np.array_equal(pos_at, want[1]), "paths at the snapshot differ from that tree's"
        depth = tree.depth
        tree.close()
        # the kernels alone
        tree, snap, _ = follow(gpu, False, profile=True)
        for _ in range(a.reps):
            tree.open(picks, at=snap)
        tree.close()
        for _ in range(a.reps):
            L.ZkTree(gpu, leaves).close()
        append_k_ms, n_appends = gpu.profile_read("zk_tree_append")
        open_k_ms, n_opens = gpu.profile_read("zk_tree_open_at")
        levels_ms, n_builds = gpu.profile_read("zk_tree_levels")
        gpu.profile(False)
        assert n_appends == a.back + a.reps and n_opens == a.reps and n_builds == a.reps

    dirty = sum(-(-a.leaves // 4 ** l) - (a.leaves - a.block) // 4 ** l for l in range(1, depth + 1))      # the last block's
    inner = sum(-(-a.leaves // 4 ** l) for l in range(1, depth + 1))
    res = {"leaves": a.leaves, "depth": depth, "block": a.block, "blocks_back": a.back, "paths_opened": a.open, "reps": a.reps,
           "append_nodes_hashed": dirty, "rebuild_nodes_hashed": inner, "append_upload_bytes": 32 * a.block, "rebuild_upload_bytes": 32 * a.leaves,
           "append_ms": round(med(append_ms), 3), "append_all_ms": [round(v, 3) for v in append_ms],
           "append_kernels_ms": round(append_k_ms / n_appends, 4),
           "open_at_ms": round(med(open_at_ms), 3), "open_at_all_ms": [round(v, 3) for v in open_at_ms],
           "open_at_kernel_ms": round(open_k_ms / n_opens, 4),
           "rebuild_ms": round(med(rebuild_ms), 3), "rebuild_all_ms": [round(v, 3) for v in rebuild_ms],
           "rebuild_levels_kernels_ms": round(levels_ms / n_builds, 4),
           "rebuild_over_append": round(med(rebuild_ms) / med(append_ms), 1), "roots_and_paths_equal": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("  python tools/zk_tree_append_time.py --leaves %d --block %d --open %d --back %d --reps %d\n  %s\n"
                    % (a.leaves, a.block, a.open, a.back, a.reps, line))


if __name__ == "__main__":
    main()
