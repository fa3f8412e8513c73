"""Appending to the device ZK tree and opening paths at earlier roots (qpgpu_zk_tree_build_reserved, _append, _snapshot, _open_at;
csrc/zk_tree.cpp, zk_tree_kernels.hip). The yardstick is a fresh leaf.ZkTree of the first n leaves at the same depth, which
tests/test_zk_tree_gpu.py pins against the host functions: after every append every level, the root and the paths of every leaf equal
the fresh tree's byte for byte, and so do the paths opened at every kept snapshot after all later appends. Refused appends and
snapshots leave the tree as it was. A spend is proven on the 2^8 leaf circuit against the root of the block it names, two appends back."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc

pytestmark = pytest.mark.gpu

P = lc.P
ZERO = bytes(32)
EINVAL, EUNSAT = -1, -4
CAPACITY, DEPTH = 70, 4
APPENDS = [1, 1, 1, 1, 11, 1, 1, 46, 1, 1]                      # from 1 leaf: the counts 2, 3, 4, 5, 16, 17, 18, 64, 65, 66


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def H(pkg):
    """the host functions, through a handle of this module's own"""
    lib = ctypes.CDLL(pkg.lib_path())
    cp = ctypes.c_char_p
    lib.qpgpu_zk_proof_verify.argtypes = [cp, cp, cp, ctypes.c_size_t, cp]
    return lib


def canonical_leaves(rng, count):
    b = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    b[:, 7::8] &= 0x7F
    return [row.tobytes() for row in b]


def limbs(*values):
    return b"".join(int(v).to_bytes(8, "little") for v in values)


def tree_state(tree, paths=True):
    """(every level's bytes, root, siblings and positions of every leaf)"""
    levels = [tree.level(l).tobytes() for l in range(tree.depth + 1)]
    assert [len(v) // 32 for v in levels] == [tree.level_size(l) for l in range(tree.depth + 1)] and levels[-1] == tree.root
    sib, pos = tree.open(range(tree.leaf_count)) if paths else (None, None)
    return levels, tree.root, sib, pos


def assert_same_tree(got, want, what):
    for l, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, (what, "level", l)
    assert len(got[0]) == len(want[0]) and got[1] == want[1], what
    if want[2] is not None and got[2] is not None:
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what


@pytest.fixture(scope="module")
def leaves70():
    """70 leaves with a group holding two equal hashes (8 and 10), a real all-zero leaf among present siblings (13) and one that opens a
    group (16: beside missing children at count 17)"""
    v = canonical_leaves(np.random.default_rng(7004), CAPACITY)
    v[10] = v[8]
    v[13] = ZERO
    v[16] = ZERO
    return v


@pytest.fixture(scope="module")
def fresh70(gpu, L, leaves70):
    """the yardstick, once per count: fresh ZkTree(leaves[:n], depth=4) -> (levels, root, siblings, positions of every leaf)"""
    cache = {}

    def at(n):
        if n not in cache:
            with L.ZkTree(gpu, leaves70[:n], depth=DEPTH) as tree:
                cache[n] = tree_state(tree)
        return cache[n]
    return at


@pytest.fixture(scope="module")
def grown(gpu, L, leaves70):
    """a tree of 1 leaf with room for 70 at depth 4 (above the minimum for most of its life: the [node, 0, 0, 0] levels are rehashed
    too) taken through APPENDS; after the build and after each append: (count, state, returned snapshot, snapshot())"""
    tree = L.ZkTree(gpu, leaves70[:1], depth=DEPTH, capacity=CAPACITY)
    assert (tree.depth, tree.leaf_count, tree.capacity) == (DEPTH, 1, CAPACITY)
    steps = [(1, tree_state(tree), None, tree.snapshot())]
    n = 1
    for k in APPENDS:
        returned = tree.append(leaves70[n:n + k])
        n += k
        assert tree.leaf_count == n and gpu.lib.qpgpu_zk_tree_leaf_count(tree.h) == n and tree.capacity == CAPACITY
        steps.append((n, tree_state(tree), returned, tree.snapshot()))
    yield tree, steps
    tree.close()


def test_appends_across_the_group_boundaries(grown, fresh70):
    tree, steps = grown
    assert [s[0] for s in steps] == [1, 2, 3, 4, 5, 16, 17, 18, 64, 65, 66]
    for n, state, returned, snap in steps:
        want = fresh70(n)
        assert_same_tree(state, want, n)
        assert (snap.count, snap.depth, snap.reserved) == (n, DEPTH, 0) and snap.root == want[1], n
        assert returned is None or bytes(returned) == bytes(snap), n
        for l in range(1, DEPTH + 1):                           # the last node of every level above the leaves, the rest zero
            assert bytes(snap.last[l - 1]) == want[0][l][-32:], (n, l)
        assert bytes(snap.last)[32 * DEPTH:] == bytes(32 * (16 - DEPTH))


def test_paths_at_every_earlier_root(grown, fresh70, leaves70, H):
    tree, steps = grown
    assert tree.leaf_count == 66
    for n, _, _, snap in steps:
        want = fresh70(n)
        sib, pos = tree.open(range(n), at=snap)
        assert np.array_equal(sib, want[2]) and np.array_equal(pos, want[3]), n
        if n in (17, 65):
            for i in range(n):
                assert H.qpgpu_zk_proof_verify(leaves70[i], sib[i].tobytes(), pos[i].tobytes(), DEPTH, snap.root) == 1, (n, i)
            assert H.qpgpu_zk_proof_verify(leaves70[0], sib[0].tobytes(), pos[0].tobytes(), DEPTH, tree.root) == 0
    # the first matching position, for either of two equal leaves and for an all-zero leaf, at an earlier root
    snap = steps[6][3]
    assert snap.count == 17
    sib, pos = tree.open([8, 10, 13, 16, 16, 0], at=snap)              # shuffled, with a repeat
    assert pos[0, 0] == pos[1, 0] and sib[0, 0].tobytes() == sib[1, 0].tobytes()
    assert pos[2, 0] == 0 and pos[3, 0] == 0 and sib[3, 0].tobytes() == bytes(96)      # [zero leaf, missing x 3]: the first slot
    assert np.array_equal(sib[3], sib[4]) and np.array_equal(sib[5], fresh70(17)[2][0])
    assert tree.open([], at=snap)[0].shape == (0, DEPTH, 3, 32)
    # the paths of the tree as it stands are untouched by all of this
    assert_same_tree(tree_state(tree), fresh70(66), "current")


def test_wide_dirty_range_and_transfers(gpu, L):
    """5 + 1100 leaves: 276 dirty parents at level 1 (more than one workgroup: the ranged node kernel), 70 at level 2 (the fused kernel)."""
    rng = np.random.default_rng(2048)
    hashes = canonical_leaves(rng, 1106)
    transfers = [(acct, int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))) for acct in canonical_leaves(rng, 37)]
    transfers[3] = (limbs(P - 1, 0, P - 1, 5), 2 ** 64 - 1, 2 ** 32 - 1, 0)
    hashed = [L.zk_leaf_hash(*t) for t in transfers]

    def fresh(n, paths):
        with L.ZkTree(gpu, (hashes + hashed)[:n], depth=6) as f:
            return tree_state(f, paths)

    with L.ZkTree(gpu, hashes[:5], depth=6, capacity=2048) as tree, L.ZkTree(gpu, hashes[:5], depth=6, capacity=2048) as twin:
        snap5 = tree.snapshot()
        snap = tree.append(hashes[5:1105])
        assert tree.leaf_count == 1105 and tree.level_size(1) == 277 and snap.count == 1105
        want = fresh(1105, True)
        assert_same_tree(tree_state(tree), want, 1105)
        assert snap.root == want[1] and bytes(snap) == bytes(tree.snapshot())
        tree.append(hashes[1105:1106])
        assert_same_tree(tree_state(tree, False), fresh(1106, False), 1106)
        s_t = tree.append(transfers=transfers)
        twin.append(hashes[5:1106])
        s_h = twin.append(hashed)
        assert tree.leaf_count == twin.leaf_count == 1143 and bytes(s_t) == bytes(s_h)
        got = tree_state(tree)
        assert_same_tree(got, tree_state(twin), "transfers against their host hashes")
        assert_same_tree(got, fresh(1143, False), 1143)
        assert got[0][0][32 * 1106:] == b"".join(hashed)
        # the 1105-leaf tree and the 5-leaf tree out of the 1143-leaf one
        sib, pos = tree.open(range(1105), at=snap)
        assert np.array_equal(sib, want[2]) and np.array_equal(pos, want[3])
        with L.ZkTree(gpu, hashes[:5], depth=6) as f5:
            sib, pos = tree.open(range(5), at=snap5)
            assert np.array_equal(sib, f5.open(range(5))[0]) and np.array_equal(pos, f5.open(range(5))[1]) and snap5.root == f5.root


def test_refusals_leave_the_tree_as_it_was(pkg, gpu, L):
    leaves = canonical_leaves(np.random.default_rng(40), 40)
    lib = gpu.lib
    with L.ZkTree(gpu, leaves[:20], capacity=40) as tree:
        assert tree.depth == 3 and tree.capacity == 40
        before, snap = tree_state(tree), tree.snapshot()

        def unchanged(what):
            assert tree.leaf_count == 20 and lib.qpgpu_zk_tree_leaf_count(tree.h) == 20, what
            assert_same_tree(tree_state(tree), before, what)
            assert bytes(tree.snapshot()) == bytes(snap), what

        def refused(needle, **kw):
            with pytest.raises(pkg.QpGpuError) as e:
                tree.append(**kw)
            assert e.value.code == EINVAL and needle in gpu.last_error() and str(e.value).endswith(gpu.last_error()), str(e.value)
            unchanged(needle)

        refused("capacity", leaves=leaves[:21])
        refused("k is 0", leaves=[])
        with_p = leaves[25][:16] + limbs(P) + leaves[25][24:]
        nine = leaves[20:25] + [with_p] + leaves[26:29]
        refused("leaf 25:", leaves=nine)
        refused("leaf 22:", leaves=leaves[20:22] + [limbs(2 ** 64 - 1) + leaves[22][8:]] + leaves[23:25] + [with_p])      # the lowest index
        buf = ctypes.create_string_buffer(b"".join(leaves[20:22]))
        err = ctypes.create_string_buffer(160)
        out = L.ZkSnapshot()
        for flags in (2, 0x80000001):
            assert lib.qpgpu_zk_tree_append(tree.h, buf, 2, flags, ctypes.addressof(out), err) == EINVAL and b"flag" in err.value
        assert lib.qpgpu_zk_tree_append(tree.h, None, 2, 0, ctypes.addressof(out), err) == EINVAL and b"null" in err.value
        assert bytes(out) == bytes(528)
        unchanged("flags and null")
        # refused snapshots, and an index that is a leaf of the tree but not of the snapshot
        half = L.ZkSnapshot.from_buffer_copy(bytes(snap))
        for count, depth, needle in ((0, 3, "count"), (21, 3, "count"), (2 ** 64 - 1, 3, "count"), (20, 2, "depth"), (20, 4, "depth")):
            half.count, half.depth = count, depth
            with pytest.raises(pkg.QpGpuError) as e:
                tree.open([0], at=half)
            assert e.value.code == EINVAL and needle in str(e.value), str(e.value)
        snap12 = None
        with L.ZkTree(gpu, leaves[:12], depth=3, capacity=40) as small:
            snap12 = small.snapshot()
        for indices, entry in (([0, 11, 12], 2), ([19], 0), ([3, 2 ** 64 - 1, 40], 1)):
            with pytest.raises(pkg.QpGpuError) as e:
                tree.open(indices, at=snap12)
            assert e.value.code == EINVAL and "index" in str(e.value) and ("entry %d:" % entry) in str(e.value), str(e.value)
        assert tree.open([11], at=snap12)[1].shape == (1, 3)
        # the next valid append, over the slots the refused ones wrote to
        after = tree.append(leaves[20:29])
        with L.ZkTree(gpu, leaves[:29], depth=3) as f:
            assert_same_tree(tree_state(tree), tree_state(f), "after the refusals")
            assert after.root == f.root and after.count == 29
        tree.append(leaves[29:40])
        with pytest.raises(pkg.QpGpuError) as e:                            # full
            tree.append(leaves[:1])
        assert "capacity" in str(e.value) and tree.leaf_count == 40
    # a tree from qpgpu_zk_tree_build has no room: its capacity is its count
    with L.ZkTree(gpu, leaves[:20], depth=3) as plain:
        assert plain.capacity == 20
        before = tree_state(plain)
        with pytest.raises(pkg.QpGpuError) as e:
            plain.append(leaves[20:21])
        assert e.value.code == EINVAL and "qpgpu_zk_tree_build" in str(e.value) and "capacity" in str(e.value)
        assert plain.leaf_count == 20
        assert_same_tree(tree_state(plain), before, "unreserved")
        assert bytes(plain.snapshot().last[2]) == plain.root              # snapshots and open_at serve any tree
        assert np.array_equal(plain.open([7], at=plain.snapshot())[0], plain.open([7])[0])
    # reserved builds: the refusals of the plan
    for count, capacity, depth, needle in ((5, 4, 0, "capacity"), (1, 2 ** 24 + 1, 0, "capacity"), (4, 17, 2, "depth"), (4, 16, 17, "depth")):
        with pytest.raises(pkg.QpGpuError) as e:
            L.ZkTree(gpu, leaves[:count], depth=depth, capacity=capacity)
        assert e.value.code == EINVAL and needle in str(e.value), str(e.value)
    with pytest.raises(pkg.QpGpuError) as e:
        L.ZkTree(gpu, leaves[:3] + [with_p], capacity=9)
    assert "leaf 3:" in str(e.value)


def test_spend_proven_at_the_root_of_its_block(pkg, gpu, L):
    """The tree at the block of a spend (20 leaves), two blocks appended, the spend's path opened at the kept snapshot: the constraints
    hold against the header that commits to the snapshot's root, the 2^8 leaf circuit proves it and the host verifier accepts. The same
    path under a header that commits to the newest root has no witness."""
    rng = np.random.default_rng(71)

    def canon32():
        b = rng.integers(0, 256, 32, dtype=np.uint8); b[7::8] &= 0x7F
        return b.tobytes()

    leaves = [canon32() for _ in range(70)]
    slot, secret, tc = 17, canon32(), int(rng.integers(1, 1000))
    unsp = L.unspendable_account(secret)
    leaves[slot] = L.zk_leaf_hash(unsp, tc, 0, 300)
    tree = L.ZkTree(gpu, leaves[:20], depth=4, capacity=70)
    snap = tree.snapshot()
    tree.append(leaves[20:45]); tree.append(leaves[45:70])
    assert snap.root != tree.root and tree.leaf_count == 70
    hk = lc.header_kat(1)

    def inputs(root):
        bh = L.block_hash(hk[0], hk[1], hk[2], hk[3], root, hk[5])
        x = L.LeafInputs()
        x.asset_id, x.volume_fee_bps, x.transfer_count, x.input_amount = 0, lc.DEFAULT_VOLUME_FEE_BPS, tc, 300
        x.output_amount_1, x.output_amount_2 = 200, 97
        x.set32("secret", secret).set32("unspendable_account", unsp).set32("nullifier", L.nullifier(secret, tc))
        x.set32("exit_account_1", bytes([4] * 32)).set32("exit_account_2", bytes([7] * 32))
        x.set32("parent_hash", hk[0]).set32("state_root", hk[2]).set32("extrinsics_root", hk[3]).set32("block_hash", bh)
        x.block_number = hk[1]
        ctypes.memmove(x.digest, hk[5], 110)
        return x, bh

    good, bh = inputs(snap.root)
    good.set_zk_path(tree, slot, at=snap)
    assert good.zk_merkle_depth == 4 and good.get32("zk_tree_root") == snap.root
    stale, _ = inputs(tree.root)                                               # the newest header, the old path
    stale.set_zk_path(tree, slot, at=snap).set32("zk_tree_root", tree.root)
    newest, _ = inputs(tree.root)                                              # (and the newest path under the newest header holds)
    newest.set_zk_path(tree, slot)
    assert newest.get32("zk_tree_root") == tree.root
    tree.close()
    err = ctypes.create_string_buffer(160)
    check = L._lib().qpgpu_leaf_check_constraints
    assert check(ctypes.byref(good), err) == 0, err.value
    assert check(ctypes.byref(newest), err) == 0, err.value
    assert check(ctypes.byref(stale), err) == EUNSAT
    leaf = L.LeafCircuit()
    assert leaf.info["degree_bits"] == 8
    h = pkg.pack_header(leaf.pack)
    nw, n = h["num_wires"], 1 << h["degree_bits"]
    circ = pkg.Circuit(gpu, leaf.pack, max_batch=2)
    d = gpu.alloc(2 * nw * n * 8)
    com = [leaf.commit(good), leaf.commit(stale)]
    cells, pis = com[0][0], np.stack([c[2] for c in com])
    assert circ.generate_witness_partial_batch_dev(cells, np.stack([c[1] for c in com]), pis, d) == [0, EUNSAT]
    proof = circ.prove_batch_dev([d.ptr], [pis[0]])[0]
    ver = pkg.Verifier(leaf.pack, circuit=circ)
    assert ver.verify(proof), ver.reason
    got = lc.proof_public_inputs(proof, 21)
    assert got.tolist() == pis[0].tolist() and got[16:20].tolist() == lc.digest_felts(bh)
    ver.close()
    d.free(scrub=True); circ.close()
