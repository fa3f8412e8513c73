"""Child process of tests/test_mx_small_trees_gpu.py: builds the small Merkle trees of that test under the hashing-kernel routing the
parent put into the environment (the routing is read once per process, so each routing needs a process of its own) and stores
every digest in an .npz file.  usage: mx_forced_trees_child.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

P = 0xFFFFFFFF00000001
LOG_LEAVES, RATE_BITS = 10, 3
WIDTHS = (5, 8, 9, 16, 17, 135)
CAP_HEIGHTS = (0, 4)
BATCH = 9


def leaves_of(width):
    """[BATCH, 2^10, width], the same in every process; every 37th leaf carries extreme elements."""
    rng = np.random.default_rng(7100 + width)
    n = 1 << LOG_LEAVES
    a = rng.integers(0, P, (BATCH, n, width), dtype=np.uint64)
    ext = np.array([0, 1, P - 1, 2**32 - 1, 2**32, P - 2**32, 2**63], dtype=np.uint64)
    for b in range(BATCH):
        for j in range(b, n, 37):
            k = int(rng.integers(1, width + 1))
            a[b, j, rng.choice(width, k, replace=False)] = rng.choice(ext, k)
    return a


def main(out_path):
    pkg = ge.load_package()
    out = {}
    n = 1 << LOG_LEAVES
    with pkg.QpGpu(0) as gpu:
        for width in WIDTHS:
            leaves = leaves_of(width)
            for cap_h in CAP_HEIGHTS:
                # one tree: the digest array holds the leaf digests and every level down to the cap
                d_dig = gpu.alloc(gpu.merkle_digest_count(LOG_LEAVES, cap_h) * 32)
                d_cols = gpu.to_device(np.ascontiguousarray(leaves[0].T))
                cap = gpu.merkle_build_dev(d_cols, n, width, LOG_LEAVES, cap_h, d_dig)
                out["b1_w%d_c%d_digests" % (width, cap_h)] = d_dig.download().reshape(-1, 4)
                out["b1_w%d_c%d_cap" % (width, cap_h)] = cap
                d_cols.free(); d_dig.free()
                # nine trees in lockstep: the commitment of nine proofs' polynomial matrices (2^7 values x width, rate 3: 2^10
                # leaves each); the Merkle paths of all leaves hold every digest of every level below the cap
                polys = [np.ascontiguousarray(leaves[b, :n >> RATE_BITS].T) for b in range(BATCH)]
                orc = pkg.PolyOracle.commit_batch(gpu, polys, rate_bits=RATE_BITS, cap_height=cap_h)
                idx = np.tile(np.arange(n, dtype=np.uint64), (BATCH, 1))
                rows, paths = orc.open(idx)
                out["b9_w%d_c%d_rows" % (width, cap_h)] = rows
                out["b9_w%d_c%d_paths" % (width, cap_h)] = paths
                out["b9_w%d_c%d_cap" % (width, cap_h)] = orc.cap()
                orc.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
