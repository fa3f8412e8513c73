"""Device build and open of the chain's 4-ary ZK Merkle tree against the host fold of the same leaves.

  zk_tree_time.py [--leaves N] [--open M] [--reps R] [--out profiles/zk_tree.txt]

N random canonical leaf hashes (default 4^10) become a resident tree (leaf.ZkTree: qpgpu_zk_tree_build, upload of the leaves included, a
host timer around the synchronous call), M random leaves (default 4096) are opened in one call (qpgpu_zk_tree_open), and the same leaves are
folded on the host one node per qpgpu_zk_hash_node call (what tests/leaf_cases.py::shared_tree_inputs does), with M host paths through
qpgpu_zk_proof_from_unsorted. The device root is compared with the host's before anything is reported. Medians of R repetitions after one
warm-up build; the kernels' share of a build (every level, leaf check included) and of an open is the library's own profile regions
zk_tree_levels / zk_tree_open (HIP events on the context's stream), taken in R further repetitions of their own. Prints one JSON line and
appends it, with the command, to --out. No GPU: it fails, it does not fall back."""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=4 ** 10)
    ap.add_argument("--open", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    L = pkg.leaf
    lib = L._lib()
    rng = np.random.default_rng(410)
    leaves = rng.integers(0, 256, (a.leaves, 32), dtype=np.uint8)
    leaves[:, 7::8] &= 0x7F
    picks = rng.integers(0, a.leaves, a.open).astype(np.uint64)
    med = lambda v: float(np.median(v))

    with pkg.QpGpu(0) as gpu:
        L.ZkTree(gpu, leaves).close()                                          # warm-up: code objects, the parameter block
        build_ms, open_ms = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); tree = L.ZkTree(gpu, leaves); t1 = time.perf_counter()
            sib, pos = tree.open(picks); t2 = time.perf_counter()
            build_ms.append(1e3 * (t1 - t0)); open_ms.append(1e3 * (t2 - t1))
            root, depth = tree.root, tree.depth
            tree.close()
        gpu.profile(True)
        for _ in range(a.reps):
            with L.ZkTree(gpu, leaves) as tree:
                tree.open(picks)
        levels_ms, n_builds = gpu.profile_read("zk_tree_levels")
        paths_ms, n_opens = gpu.profile_read("zk_tree_open")
        gpu.profile(False)
        assert n_builds == a.reps and n_opens == a.reps

    # the host fold: one ctypes call per node, a missing child is the empty hash
    lib.qpgpu_zk_hash_node.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    out = ctypes.create_string_buffer(32)
    t0 = time.perf_counter()
    levels = [[r.tobytes() for r in leaves]]
    nodes = 0
    for _ in range(depth):
        cur = levels[-1]; nxt = []
        for g in range(0, len(cur), 4):
            assert lib.qpgpu_zk_hash_node(b"".join((cur[g:g + 4] + [bytes(32)] * 3)[:4]), out) == 0
            nxt.append(out.raw)
        nodes += len(nxt); levels.append(nxt)
    host_fold_s = time.perf_counter() - t0
    assert levels[-1][0] == root, "device root differs from the host fold"
    t0 = time.perf_counter()
    for row, i in enumerate(picks.tolist()):
        sibs, idx = [], i
        for lvl in levels[:-1]:
            g = idx - idx % 4
            group = (lvl[g:g + 4] + [bytes(32)] * 3)[:4]
            sibs.append([group[k] for k in range(4) if k != idx % 4]); idx //= 4
        s, p, r = L.zk_proof_from_unsorted(levels[0][i], sibs)
        assert s == sib[row].tobytes() and p == pos[row].tolist() and r == root, "device path differs from the host's"
    host_open_s = time.perf_counter() - t0
    res = {"leaves": a.leaves, "depth": depth, "inner_nodes": nodes, "permutations": 3 * nodes, "paths_opened": a.open, "reps": a.reps,
           "device_build_ms": round(med(build_ms), 3), "device_build_all_ms": [round(v, 3) for v in build_ms],
           "device_levels_kernels_ms": round(levels_ms / n_builds, 4), "permutations_per_s": round(3 * nodes / (1e-3 * levels_ms / n_builds)),
           "device_open_kernel_ms": round(paths_ms / n_opens, 4),
           "device_open_ms": round(med(open_ms), 3), "device_open_all_ms": [round(v, 3) for v in open_ms],
           "host_fold_s": round(host_fold_s, 3), "host_open_s": round(host_open_s, 3),
           "build_speedup": round(1e3 * host_fold_s / med(build_ms), 1), "roots_and_paths_equal": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("  python tools/zk_tree_time.py --leaves %d --open %d --reps %d\n  %s\n" % (a.leaves, a.open, a.reps, line))


if __name__ == "__main__":
    main()
