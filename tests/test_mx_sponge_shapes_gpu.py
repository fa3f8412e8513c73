"""The leaf sponge of the matrix-pipe hashing build (merkle_kernels_mx.hip) ends a block's permutation in one of three ways: the
capacity rows alone before a full block, every row before a ragged last block (the rate lanes that block does not fill stay in
the state), the digest rows after the last block. Widths 5, 8, 9, 16 and 17 on 2^18 leaves (the smallest launch the matrix build
takes) put a ragged and a full block first-and-last, a full block before a one-element and before a full last block, and all
three endings in one leaf. Digests, every level and the cap against the oracle; every 997th leaf carries extreme elements."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
LOG_LEAVES, CAP_H = 18, 4


@pytest.mark.parametrize("width", [5, 8, 9, 16, 17])
def test_leaf_sponge_block_shapes_vs_oracle(gpu, orc, width):
    n = 1 << LOG_LEAVES
    rng = np.random.default_rng(9000 + width)
    leaves = rng.integers(0, P, (n, width), dtype=np.uint64)
    ext = np.array([0, P - 1, 2**32 - 1, 2**63, 2**32, P - 2**32], dtype=np.uint64)
    for j in range(0, n, 997):
        k = int(rng.integers(1, width + 1))
        leaves[j, rng.choice(width, k, replace=False)] = rng.choice(ext, k)
    dig_want, cap_want = orc.merkle(leaves, CAP_H)
    d_dig = gpu.alloc(gpu.merkle_digest_count(LOG_LEAVES, CAP_H) * 32)
    d_cols = gpu.to_device(np.ascontiguousarray(leaves.T))
    cap = gpu.merkle_build_dev(d_cols, n, width, LOG_LEAVES, CAP_H, d_dig)
    got = d_dig.download().reshape(-1, 4)
    d_cols.free(); d_dig.free()
    assert np.array_equal(got[:n], dig_want[:n]), "leaf digests"
    assert np.array_equal(got, dig_want), "tree levels"
    assert np.array_equal(cap, cap_want), "cap"
