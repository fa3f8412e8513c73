"""Child process of tests/test_mx_digits_gpu.py: builds that test's small Merkle trees and one 2^8-row proof under the hashing-kernel
routing the parent put into the environment (the routing is read once per process) and stores every digest and the proof bytes
in an .npz file.  usage: mx_digits_child.py <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

P = 0xFFFFFFFF00000001
LOG_LEAVES, RATE_BITS, CAP_HEIGHT = 10, 3, 4
WIDTHS = (9, 17, 135)
BATCH = 3
# the byte edges of the digit conversion (poseidon_mfma.hpp: to_digits), reduced mod p where they are not canonical
EDGES = [v % P for v in (0, 1, 0x7F7F7F7F7F7F7F7F, 0x8080808080808080, 0x8080808080808080 - 1, P - 1, P, 2**64 - 1)]
PROOF_CIRCUIT = dict(seed=4, poseidon=True, base_sum=True, poseidon2=True)


def leaves_of(width):
    """[BATCH, 2^10, width], the same in every process: about every third element is one of EDGES, the rest random; leaf b is
    made of edge values only, leaf BATCH + k of EDGES[k] alone."""
    rng = np.random.default_rng(9300 + width)
    n = 1 << LOG_LEAVES
    a = rng.integers(0, P, (BATCH, n, width), dtype=np.uint64)
    edge = np.array(EDGES, dtype=np.uint64)
    pick = rng.choice(edge, a.shape)
    a = np.where(rng.random(a.shape) < 1 / 3, pick, a)
    for b in range(BATCH):
        a[b, b] = rng.choice(edge, width)
        for k in range(len(EDGES)):
            a[b, BATCH + k] = edge[k]
    return a


def main(out_path):
    pkg = ge.load_package()
    out = {}
    n = 1 << LOG_LEAVES
    with pkg.QpGpu(0) as gpu:
        for width in WIDTHS:
            leaves = leaves_of(width)
            d_dig = gpu.alloc(gpu.merkle_digest_count(LOG_LEAVES, CAP_HEIGHT) * 32)
            d_cols = gpu.to_device(np.ascontiguousarray(leaves[0].T))
            cap = gpu.merkle_build_dev(d_cols, n, width, LOG_LEAVES, CAP_HEIGHT, d_dig)
            out["b1_w%d_digests" % width] = d_dig.download().reshape(-1, 4)
            out["b1_w%d_cap" % width] = cap
            d_cols.free(); d_dig.free()
            # three trees in lockstep: the commitment of three polynomial matrices (2^7 values x width, rate 3: 2^10 leaves each);
            # the Merkle paths of all leaves hold every digest below the cap
            polys = [np.ascontiguousarray(leaves[b, :n >> RATE_BITS].T) for b in range(BATCH)]
            orc = pkg.PolyOracle.commit_batch(gpu, polys, rate_bits=RATE_BITS, cap_height=CAP_HEIGHT)
            rows, paths = orc.open(np.tile(np.arange(n, dtype=np.uint64), (BATCH, 1)))
            out["b3_w%d_rows" % width] = rows
            out["b3_w%d_paths" % width] = paths
            out["b3_w%d_cap" % width] = orc.cap()
            orc.close()
        # one whole proof at 2^8 rows: its trees, its transcript and its proof-of-work search (the nonce is in the bytes)
        pack, wires, pis = pkg.synth_circuit(8, **PROOF_CIRCUIT)
        circ = pkg.Circuit(gpu, pack)
        out["proof"] = np.frombuffer(circ.prove(wires, pis), dtype=np.uint8)
        circ.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
