"""The chain's 4-ary ZK Merkle tree on the device (qpgpu_zk_tree_*, qpgpu_zk_leaf_hash_batch; csrc/zk_tree.cpp, zk_tree_kernels.hip)
against the host functions of include/qpgpu_leaf.h, byte for byte: every level and the root at the group boundaries and at depths above
the minimum, the paths of every leaf, the byte-string child order where it differs from the order of the limbs, ties, every refusal, the
batch leaf hash, a tree wider than one workgroup, and eight spends of one device tree proven in one lockstep batch. The oracle is not
involved: the host functions are the specification (pinned by the reference's KATs, tests/test_zk_merkle.py).

Reference scenarios carried here: wormhole/tests/src/prover/prover_tests.rs builds random trees with a private builder of its own
(build_4ary_tree and generate_proof, lines 130-214) in its test_random_tree_* tests: 4, 16 and 64 random leaves, every path verified
natively, one random leaf proven. The device tree is that builder; the scenarios are test_levels_and_root_at_the_group_boundaries
(counts 4, 16 and 64 among them), test_paths_of_every_leaf and test_spends_of_a_device_tree_into_proofs."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc

pytestmark = pytest.mark.gpu

P = lc.P
ZERO = bytes(32)
EINVAL, EUNSAT = -1, -4


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def H(pkg):
    """the host functions, through a handle of this module's own (its argtypes are nobody else's)"""
    lib = ctypes.CDLL(pkg.lib_path())
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    lib.qpgpu_zk_leaf_hash.argtypes = [cp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, cp]
    lib.qpgpu_zk_hash_node.argtypes = [cp, cp]
    lib.qpgpu_zk_hash_node_presorted.argtypes = [cp, cp]
    lib.qpgpu_zk_proof_verify.argtypes = [cp, cp, cp, sz, cp]
    return lib


def canonical_leaves(rng, count):
    b = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    b[:, 7::8] &= 0x7F
    return [row.tobytes() for row in b]


def limbs(*values):
    return b"".join(int(v).to_bytes(8, "little") for v in values)


def hash_node(H, children, presorted=False):
    out = ctypes.create_string_buffer(32)
    assert (H.qpgpu_zk_hash_node_presorted if presorted else H.qpgpu_zk_hash_node)(b"".join(children), out) == 0
    return out.raw


def host_levels(H, leaves, depth):
    """the reference's test builder: groups of four, a missing child is the empty hash; depth levels, however few nodes are left"""
    levels = [list(leaves)]
    for _ in range(depth):
        cur = levels[-1]
        levels.append([hash_node(H, (cur[g:g + 4] + [ZERO] * 3)[:4]) for g in range(0, len(cur), 4)])
    return levels


def min_depth(count):
    d = 1
    while 4 ** d < count:
        d += 1
    return d


def host_path(L, levels, index):
    """qpgpu_zk_proof_from_unsorted on the unsorted siblings taken from the host levels: (sorted siblings, positions, root)"""
    sibs, idx = [], index
    for lvl in levels[:-1]:
        g = idx - idx % 4
        group = (lvl[g:g + 4] + [ZERO] * 3)[:4]
        sibs.append([group[k] for k in range(4) if k != idx % 4])
        idx //= 4
    return L.zk_proof_from_unsorted(levels[0][index], sibs)


def assert_levels(tree, levels):
    assert tree.depth == len(levels) - 1 and tree.leaf_count == len(levels[0])
    for l, want in enumerate(levels):
        assert tree.level_size(l) == len(want)
        assert tree.level(l).tobytes() == b"".join(want), "level %d" % l
    assert tree.root == levels[-1][0] and len(levels[-1]) == 1


def assert_paths(L, H, tree, levels, indices):
    sib, pos = tree.open(indices)
    for row, i in enumerate(indices):
        want_sibs, want_pos, want_root = host_path(L, levels, i)
        assert sib[row].tobytes() == want_sibs and pos[row].tolist() == want_pos and want_root == tree.root, i
        assert H.qpgpu_zk_proof_verify(levels[0][i], sib[row].tobytes(), pos[row].tobytes(), tree.depth, tree.root) == 1, i
    return sib, pos


@pytest.mark.parametrize("count", [1, 2, 4, 5, 16, 17, 63, 64, 65, 257])
def test_levels_and_root_at_the_group_boundaries(gpu, L, H, count):
    leaves = canonical_leaves(np.random.default_rng(100 + count), count)
    with L.ZkTree(gpu, leaves) as tree:
        assert tree.depth == min_depth(count)
        assert_levels(tree, host_levels(H, leaves, tree.depth))
        assert tree.level(1, 0, 0).shape == (0, 32) and tree.level(0, count - 1, 1).tobytes() == leaves[-1]


@pytest.mark.parametrize("count,depth", [(5, 4), (1, 16)])
def test_depth_above_the_minimum(gpu, L, H, count, depth):
    leaves = canonical_leaves(np.random.default_rng(7 * depth), count)
    with L.ZkTree(gpu, leaves, depth=depth) as tree:
        levels = host_levels(H, leaves, depth)
        assert [len(v) for v in levels[min_depth(count):]] == [1] * (depth - min_depth(count) + 1)      # [node, 0, 0, 0] from there on
        assert_levels(tree, levels)
        assert_paths(L, H, tree, levels, [count - 1])


def test_paths_of_every_leaf(gpu, L, H):
    count = 65
    leaves = canonical_leaves(np.random.default_rng(65), count)
    with L.ZkTree(gpu, leaves) as tree:
        levels = host_levels(H, leaves, tree.depth)
        sib, pos = assert_paths(L, H, tree, levels, list(range(count)))
        order = np.random.default_rng(3).integers(0, count, 150)                 # shuffled, with repeats
        assert len(set(order.tolist())) < order.size
        sib2, pos2 = tree.open(order)
        assert np.array_equal(sib2, sib[order]) and np.array_equal(pos2, pos[order])
        assert tree.open([])[0].shape == (0, tree.depth, 3, 32)


def test_children_sort_as_byte_strings_not_as_limbs(gpu, L, H):
    """Children that differ in one limb only, chosen so that the order of the 32 bytes is the reverse of the order of that limb as a
    little-endian integer: 01 00 .. 00 (the integer 1) sorts last as bytes, 00 .. 00 01 (2^56) first."""
    base = canonical_leaves(np.random.default_rng(4), 2)
    variants = [limbs(1), limbs(1 << 56), limbs(1 << 8), limbs(1 << 48)]
    assert variants[0] == bytes([1, 0, 0, 0, 0, 0, 0, 0]) and variants[1] == bytes([0, 0, 0, 0, 0, 0, 0, 1])
    in_limb_0 = [v + base[0][8:] for v in variants]
    in_limb_3 = [base[1][:24] + v for v in variants]
    leaves = in_limb_0 + in_limb_3
    with L.ZkTree(gpu, leaves) as tree:
        levels = host_levels(H, leaves, 2)
        assert_levels(tree, levels)
        assert_paths(L, H, tree, levels, list(range(8)))
        got = tree.level(1)
        for g, group in enumerate((in_limb_0, in_limb_3)):
            by_bytes = sorted(group)
            by_limbs = sorted(group, key=lambda h: [int.from_bytes(h[8 * i:8 * i + 8], "little") for i in range(4)])
            assert by_limbs == by_bytes[::-1]
            right, wrong = hash_node(H, by_bytes, presorted=True), hash_node(H, by_limbs, presorted=True)
            assert right != wrong                                              # a numeric-limb sort could not pass by accident
            assert got[g].tobytes() == right == levels[1][g]
        assert tree.open([0])[1][0, 0] == 3 and tree.open([1])[1][0, 0] == 0      # 01 00 .. sorts last, 00 .. 01 first


def test_ties(gpu, L, H):
    x, y, z, w = canonical_leaves(np.random.default_rng(12), 4)
    leaves = [x, y, x, z] + [w] * 4 + [ZERO]                                   # two equal, four equal, a real all-zero leaf beside missing children
    with L.ZkTree(gpu, leaves) as tree:
        levels = host_levels(H, leaves, 2)
        assert_levels(tree, levels)
        sib, pos = assert_paths(L, H, tree, levels, list(range(9)))
        assert pos[0, 0] == pos[2, 0] and sib[0, 0].tobytes() == sib[2, 0].tobytes()      # the first match, for either copy
        assert pos[4:8, 0].tolist() == [0] * 4 and pos[8, 0] == 0
        assert levels[1][2] == hash_node(H, [ZERO] * 4)


def raw_build(gpu, data, count, depth=0, flags=0):
    h = ctypes.c_void_p(0x5A5A)
    err = ctypes.create_string_buffer(160)
    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    rc = gpu.lib.qpgpu_zk_tree_build(gpu.ctx, buf, count, depth, flags, ctypes.byref(h), err)
    if rc == 0:
        gpu.lib.qpgpu_zk_tree_free(h)
    return rc, h.value, err.value.decode()


def test_refusals(pkg, gpu, L):
    leaves = canonical_leaves(np.random.default_rng(6), 20)
    with_p = leaves[5][:16] + limbs(P) + leaves[5][24:]
    with_max = limbs(2 ** 64 - 1) + leaves[9][8:]
    for bad_at, want in (({5: with_p}, 5), ({11: with_max}, 11), ({9: with_max, 3: with_p}, 3), ({0: with_p, 19: with_p}, 0)):
        data = b"".join(bad_at.get(i, h) for i, h in enumerate(leaves))
        rc, handle, msg = raw_build(gpu, data, 20)
        assert rc == EINVAL and handle is None and ("leaf %d:" % want) in msg and "noncanonical" in msg, msg
        assert gpu.last_error() == msg
        with pytest.raises(pkg.QpGpuError) as e:
            L.ZkTree(gpu, data)
        assert e.value.code == EINVAL and ("leaf %d:" % want) in str(e.value)
    # the largest canonical limb is accepted
    rc, handle, msg = raw_build(gpu, limbs(P - 1, P - 1, P - 1, P - 1) + b"".join(leaves[1:]), 20)
    assert rc == 0 and msg == ""
    data = b"".join(leaves)
    for count, depth, flags, needle in ((0, 0, 0, "count"), (20, 17, 0, "depth"), (20, 2, 0, "depth"), (17, 2, 0, "depth"), (20, 0, 2, "flag"), (20, 0, 0x80000001, "flag"),
                                        ((1 << 24) + 1, 0, 0, "count")):
        rc, handle, msg = raw_build(gpu, data, count, depth, flags)
        assert rc == EINVAL and handle is None and needle in msg, (count, depth, flags, msg)
    assert raw_build(gpu, data, 16, 2)[0] == 0 and raw_build(gpu, data, 20, 3)[0] == 0 and raw_build(gpu, data, 20, 16)[0] == 0
    with L.ZkTree(gpu, leaves) as tree:
        for indices in ([20], [0, 19, 20], [2 ** 64 - 1]):
            with pytest.raises(pkg.QpGpuError) as e:
                tree.open(indices)
            assert e.value.code == EINVAL and "index" in str(e.value)
        out = ctypes.create_string_buffer(64)
        lib = gpu.lib
        assert lib.qpgpu_zk_tree_read_level(tree.h, tree.depth + 1, 0, 1, out) == EINVAL and "level" in gpu.last_error()
        assert lib.qpgpu_zk_tree_read_level(tree.h, 17, 0, 0, out) == EINVAL
        assert lib.qpgpu_zk_tree_read_level(tree.h, 0, 19, 2, out) == EINVAL and lib.qpgpu_zk_tree_read_level(tree.h, 1, 6, 0, out) == EINVAL
        assert lib.qpgpu_zk_tree_read_level(tree.h, 0, 19, 1, out) == 0 and out.raw[:32] == leaves[19]
        assert tree.open([19])[1].shape == (1, 3)                                # and the handle still serves


def test_leaf_hashes(gpu, L, H):
    rng = np.random.default_rng(300)
    accounts = canonical_leaves(rng, 300)
    accounts[7] = limbs(P - 1, 0, P - 1, 5)
    counts = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1] + [int(v) for v in rng.integers(0, 2 ** 63, 296)]
    words = [0, 2 ** 32 - 1]
    transfers = [(accounts[i], counts[i], words[(i >> 2) & 1] if i < 16 else int(rng.integers(0, 2 ** 32)),
                  words[(i >> 3) & 1] if i < 16 else int(rng.integers(0, 2 ** 32))) for i in range(300)]
    assert {(t[2], t[3]) for t in transfers[:16]} == {(a, b) for a in words for b in words}
    want = []
    for acct, tc, asset, amount in transfers:
        out = ctypes.create_string_buffer(32)
        assert H.qpgpu_zk_leaf_hash(acct, tc, asset, amount, out) == 0
        want.append(out.raw)
    got = L.zk_leaf_hash_batch(gpu, transfers)
    assert got.shape == (300, 32) and got.tobytes() == b"".join(want)
    with L.ZkTree(gpu, transfers=transfers) as from_transfers, L.ZkTree(gpu, want) as from_hashes:
        assert from_transfers.depth == from_hashes.depth == 5 and from_transfers.root == from_hashes.root
        assert from_transfers.level(0).tobytes() == b"".join(want)
        assert from_transfers.root == host_levels(H, want, 5)[-1][0]


def test_tree_past_one_workgroup(gpu, L, H):
    """4^7 + 3 leaves: levels 1 to 3 have more parents than a workgroup has threads (one launch each), levels 4 to 8 run fused."""
    count = 4 ** 7 + 3
    leaves = canonical_leaves(np.random.default_rng(47), count)
    with L.ZkTree(gpu, leaves) as tree:
        assert tree.depth == 8
        levels = host_levels(H, leaves, 8)
        assert [len(v) for v in levels] == [16387, 4097, 1025, 257, 65, 17, 5, 2, 1]
        assert tree.root == levels[-1][0]
        for l in (1, 3, 4, 7):
            assert tree.level(l).tobytes() == b"".join(levels[l]), l
        picks = [0, count - 1, count - 3, 4 ** 7] + np.random.default_rng(48).integers(0, count, 28).tolist()
        assert len(picks) == 32
        assert_paths(L, H, tree, levels, picks)


def test_spends_of_a_device_tree_into_proofs(pkg, gpu, L):
    """Eight spends of one block among 70 leaves of a device tree (depth 4), built as leaf_cases.shared_tree_inputs builds them but
    with the tree, its root and the paths from the device: the constraints hold on the host, one lockstep batch on the restated leaf
    circuit proves them, the host verifier accepts, and the public inputs carry the hash of the header that commits to the device root."""
    rng = np.random.default_rng(70)

    def canon32():
        b = rng.integers(0, 256, 32, dtype=np.uint8); b[7::8] &= 0x7F
        return b.tobytes()

    slots = [0, 3, 17, 18, 31, 64, 66, 69]
    leaves = [canon32() for _ in range(70)]
    spends = []
    for slot in slots:
        secret, tc = canon32(), int(rng.integers(1, 1000))
        unsp = L.unspendable_account(secret)
        leaves[slot] = L.zk_leaf_hash(unsp, tc, 0, 300)
        spends.append((secret, tc, unsp))
    tree = L.ZkTree(gpu, leaves, depth=4)
    hk = lc.header_kat(1)
    bh = L.block_hash(hk[0], hk[1], hk[2], hk[3], tree.root, hk[5])
    xs = []
    for slot, (secret, tc, unsp) in zip(slots, spends):
        x = L.LeafInputs()
        x.asset_id, x.volume_fee_bps, x.transfer_count, x.input_amount = 0, lc.DEFAULT_VOLUME_FEE_BPS, tc, 300
        x.output_amount_1, x.output_amount_2 = 200, 97
        x.set32("secret", secret).set32("unspendable_account", unsp).set32("nullifier", L.nullifier(secret, tc))
        x.set32("exit_account_1", bytes([4] * 32)).set32("exit_account_2", bytes([7] * 32))
        x.set32("parent_hash", hk[0]).set32("state_root", hk[2]).set32("extrinsics_root", hk[3]).set32("block_hash", bh)
        x.block_number = hk[1]
        ctypes.memmove(x.digest, hk[5], 110)
        x.set_zk_path(tree, slot)
        assert x.zk_merkle_depth == 4 and x.get32("zk_tree_root") == tree.root
        xs.append(x)
    tree.close()
    err = ctypes.create_string_buffer(160)
    check = L._lib().qpgpu_leaf_check_constraints
    for x in xs:
        assert check(ctypes.byref(x), err) == 0, err.value
    leaf = L.LeafCircuit()
    assert leaf.info["degree_bits"] == 8
    h = pkg.pack_header(leaf.pack)
    nw, n = h["num_wires"], 1 << h["degree_bits"]
    circ = pkg.Circuit(gpu, leaf.pack, max_batch=8)
    d = gpu.alloc(8 * nw * n * 8)
    com = [leaf.commit(x) for x in xs]
    cells, pis = com[0][0], np.stack([c[2] for c in com])
    assert circ.generate_witness_partial_batch_dev(cells, np.stack([c[1] for c in com]), pis, d) == [0] * 8
    proofs = circ.prove_batch_dev([d.ptr + 8 * k * nw * n for k in range(8)], list(pis))
    ver = pkg.Verifier(leaf.pack, circuit=circ)
    for k, proof in enumerate(proofs):
        assert ver.verify(proof), (k, ver.reason)
        got = lc.proof_public_inputs(proof, 21)
        assert got.tolist() == pis[k].tolist() and got[16:20].tolist() == lc.digest_felts(bh)
    ver.close()
    # one sibling byte of one spend: that spend alone has no witness
    bad = xs[5].copy()
    bad.zk_merkle_siblings[32 + 4] ^= 1                                         # level 0, second sibling: one of leaves 65 .. 67
    assert check(ctypes.byref(bad), err) == EUNSAT and check(ctypes.byref(xs[5]), err) == 0
    vals = np.stack([(leaf.commit(bad) if k == 5 else com[k])[1] for k in range(8)])
    assert circ.generate_witness_partial_batch_dev(cells, vals, pis, d) == [0, 0, 0, 0, 0, EUNSAT, 0, 0]
    d.free(scrub=True); circ.close()
