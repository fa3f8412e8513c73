"""Child process of tests/test_mx_mds_gemm_gpu.py: builds that test's small Merkle trees and one 2^8-row proof under the
hashing-kernel routing the parent put into the environment (the routing is read once per process) and stores every digest, the
opened rows and paths and the proof bytes in an .npz file.  usage: mx_mds_gemm_child.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from mx_digits_child import EDGES, P, PROOF_CIRCUIT  # noqa: E402,F401

LOG_LEAVES, RATE_BITS, CAP_HEIGHT = 10, 3, 4
# one block with the digest ending; a ragged block behind a full one; two full blocks (capacity-only ending); both endings; wires
WIDTHS = (8, 9, 16, 17, 135)
# three 2^8-leaf trees in lockstep: 768 leaf hashes, a half-filled workgroup and clamped lanes on the levels above
LOCK_LOG_LEAVES, LOCK_BATCH, LOCK_WIDTH = 8, 3, 9


def leaves_of(width):
    """[2^10, width], the same in every process: about every third element is one of EDGES, the rest random; leaf 0 is made of edge
    values only, leaf 1 + k of EDGES[k] alone."""
    rng = np.random.default_rng(9700 + width)
    a = rng.integers(0, P, (1 << LOG_LEAVES, width), dtype=np.uint64)
    edge = np.array(EDGES, dtype=np.uint64)
    a = np.where(rng.random(a.shape) < 1 / 3, rng.choice(edge, a.shape), a)
    a[0] = rng.choice(edge, width)
    for k in range(len(EDGES)):
        a[1 + k] = edge[k]
    return a


def lockstep_polys():
    """LOCK_BATCH matrices [LOCK_WIDTH, 2^5] of values (rate 3: 2^8 leaves each), edge values mixed in."""
    rng = np.random.default_rng(9799)
    shape = (LOCK_BATCH, LOCK_WIDTH, 1 << (LOCK_LOG_LEAVES - RATE_BITS))
    a = rng.integers(0, P, shape, dtype=np.uint64)
    return np.where(rng.random(shape) < 1 / 3, rng.choice(np.array(EDGES, dtype=np.uint64), shape), a)


def main(out_path):
    pkg = ge.load_package()
    out = {}
    n = 1 << LOG_LEAVES
    with pkg.QpGpu(0) as gpu:
        for width in WIDTHS:
            d_dig = gpu.alloc(gpu.merkle_digest_count(LOG_LEAVES, CAP_HEIGHT) * 32)
            d_cols = gpu.to_device(np.ascontiguousarray(leaves_of(width).T))
            cap = gpu.merkle_build_dev(d_cols, n, width, LOG_LEAVES, CAP_HEIGHT, d_dig)
            out["w%d_digests" % width] = d_dig.download().reshape(-1, 4)
            out["w%d_cap" % width] = cap
            d_cols.free(); d_dig.free()
        polys = lockstep_polys()
        orc = pkg.PolyOracle.commit_batch(gpu, [np.ascontiguousarray(p) for p in polys], rate_bits=RATE_BITS, cap_height=CAP_HEIGHT)
        rows, paths = orc.open(np.tile(np.arange(1 << LOCK_LOG_LEAVES, dtype=np.uint64), (LOCK_BATCH, 1)))
        out["lock_rows"], out["lock_paths"], out["lock_cap"] = rows, paths, orc.cap()
        orc.close()
        # one whole proof at 2^8 rows: its trees, its transcript and its proof-of-work search (the nonce is in the bytes)
        pack, wires, pis = pkg.synth_circuit(8, **PROOF_CIRCUIT)
        circ = pkg.Circuit(gpu, pack)
        out["proof"] = np.frombuffer(circ.prove(wires, pis), dtype=np.uint8)
        circ.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
