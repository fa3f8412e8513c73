"""The device ZK tree at earlier counts without kept snapshots, paths at many roots per call, and reorgs (qpgpu_zk_tree_snapshots_at,
_snapshot_check, _open_at_counts, _truncate; csrc/zk_tree.cpp, zk_tree_kernels.hip). The yardstick is the one of
tests/test_zk_tree_append_gpu.py: a fresh leaf.ZkTree of the first n leaves at the same depth, which tests/test_zk_tree_gpu.py pins
against the host functions. Derived snapshots equal the fresh trees' and the ones the appends returned, byte for byte; one open call
over every (count, index) equals the fresh trees' paths and roots; a truncated and regrown tree equals the fresh tree of its leaves at
every level; refusals leave the outputs and the tree as they were. A spend is proven on the 2^8 leaf circuit against the root of an
earlier block of the new fork, its path opened by count."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc

pytestmark = pytest.mark.gpu

ZERO = bytes(32)
EINVAL, EUNSAT = -1, -4
CAPACITY, DEPTH = 70, 4
APPENDS = [1, 1, 1, 1, 11, 1, 1, 46, 1, 1, 4]                   # from 1 leaf: the counts 2, 3, 4, 5, 16, 17, 18, 64, 65, 66, 70


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


def tree_state(tree, paths=True):
    """(every level's bytes, root, siblings and positions of every leaf, snapshot())"""
    levels = [tree.level(l).tobytes() for l in range(tree.depth + 1)]
    assert [len(v) // 32 for v in levels] == [tree.level_size(l) for l in range(tree.depth + 1)] and levels[-1] == tree.root
    sib, pos = tree.open(range(tree.leaf_count)) if paths else (None, None)
    return levels, tree.root, sib, pos, bytes(tree.snapshot())


def assert_same_tree(got, want, what):
    assert len(got[0]) == len(want[0]), what
    for l, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, (what, "level", l)
    assert got[1] == want[1] and got[4] == want[4], what
    if want[2] is not None and got[2] is not None:
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what


def fresh_state(gpu, L, leaves, depth, paths=True):
    with L.ZkTree(gpu, leaves, depth=depth) as tree:
        return tree_state(tree, paths)


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
    """the yardstick, once per count 1 .. 70: fresh ZkTree(leaves[:n], depth=4) -> tree_state"""
    return {n: fresh_state(gpu, L, leaves70[:n], DEPTH) for n in range(1, CAPACITY + 1)}


@pytest.fixture(scope="module")
def grown(gpu, L, leaves70):
    """a tree of 1 leaf with room for 70 at depth 4 (above the minimum for most counts: the [node, 0, 0, 0] levels are derived too) taken
    through APPENDS to 70 leaves; kept: {count: the snapshot the build or the append gave}"""
    tree = L.ZkTree(gpu, leaves70[:1], depth=DEPTH, capacity=CAPACITY)
    kept = {1: tree.snapshot()}
    n = 1
    for k in APPENDS:
        kept[n + k] = tree.append(leaves70[n:n + k])
        n += k
    assert tree.leaf_count == CAPACITY
    yield tree, kept
    tree.close()


def test_snapshots_at_every_count(grown, fresh70, L):
    tree, kept = grown
    snaps = tree.snapshots_at(range(1, CAPACITY + 1))
    assert len(snaps) == CAPACITY and sorted(kept) == [1, 2, 3, 4, 5, 16, 17, 18, 64, 65, 66, 70]
    for n, snap in zip(range(1, CAPACITY + 1), snaps):
        want = fresh70[n]
        assert (snap.count, snap.depth, snap.reserved) == (n, DEPTH, 0), n
        for l in range(1, DEPTH + 1):                           # the last node of every level above the leaves, the rest zero
            assert bytes(snap.last[l - 1]) == want[0][l][-32:], (n, l)
        assert bytes(snap) == want[4] and snap.root == want[1], n
        if n in kept:
            assert bytes(snap) == bytes(kept[n]), n
        assert tree.check(snap) is True, n
    assert tree.snapshots_at([]) == []
    # counts in any order, with repeats
    again = tree.snapshots_at([70, 17, 17, 1, 64])
    assert [bytes(s) for s in again] == [fresh70[n][4] for n in (70, 17, 17, 1, 64)]
    # a snapshot with one node changed, at the top and at the bottom, does not check; neither does one with the reserved word set
    for level in (1, DEPTH):
        forged = L.ZkSnapshot.from_buffer_copy(bytes(kept[17]))
        forged.last[level - 1][5] ^= 1
        assert tree.check(forged) is False and ("level %d" % level) in tree.gpu.last_error()
    forged = L.ZkSnapshot.from_buffer_copy(bytes(kept[17]))
    forged.reserved = 1
    assert tree.check(forged) is False
    assert bytes(tree.snapshot()) == fresh70[CAPACITY][4]       # the tree itself is untouched by all of this


def test_snapshots_at_depth_16(gpu, L):
    """capacity 6 at depth 16: the whole 16-level chain, fourteen levels of [node, 0, 0, 0]"""
    leaves = canonical_leaves(np.random.default_rng(1606), 6)
    leaves[4] = ZERO                                            # an all-zero leaf that opens a group
    with L.ZkTree(gpu, leaves[:1], depth=16, capacity=6) as tree:
        kept = {1: tree.snapshot()}
        kept[3] = tree.append(leaves[1:3]); kept[5] = tree.append(leaves[3:5]); kept[6] = tree.append(leaves[5:6])
        snaps = tree.snapshots_at([1, 2, 3, 4, 5, 6])
        for n, snap in zip(range(1, 7), snaps):
            want = fresh_state(gpu, L, leaves[:n], 16, paths=False)
            assert (snap.count, snap.depth, snap.reserved) == (n, 16, 0) and bytes(snap) == want[4] and snap.root == want[1], n
            assert n not in kept or bytes(kept[n]) == bytes(snap), n
            assert tree.check(snap) is True, n


def test_paths_at_many_roots_in_one_call(grown, fresh70, leaves70, H):
    tree, kept = grown
    counts = list(range(1, CAPACITY + 1))                       # every count, every index below it: 2485 paths, 9940 threads
    pairs = [(c, i) for c in counts for i in range(c)]
    order = np.random.default_rng(99).permutation(len(pairs))   # the counts interleaved: a path's snapshot is found by its own entry
    cnt = np.array([pairs[j][0] for j in order], dtype=np.uint64)
    idx = np.array([pairs[j][1] for j in order], dtype=np.uint64)
    sib, pos, roots = tree.open(idx, at=cnt, roots=True)
    assert sib.shape == (len(pairs), DEPTH, 3, 32) and pos.shape == (len(pairs), DEPTH) and roots.shape == (len(pairs), 32) and len(pairs) == 2485
    for j in range(len(pairs)):
        c, i = int(cnt[j]), int(idx[j])
        want = fresh70[c]
        assert sib[j].tobytes() == want[2][i].tobytes() and pos[j].tobytes() == want[3][i].tobytes() and roots[j].tobytes() == want[1], (c, i)
        assert H.qpgpu_zk_proof_verify(leaves70[i], sib[j].tobytes(), pos[j].tobytes(), DEPTH, roots[j].tobytes()) == 1, (c, i)
    for c, snap in kept.items():                                # what open_at gives with the kept snapshots
        s_at, p_at = tree.open(range(c), at=snap)
        mine = [int(np.flatnonzero((cnt == c) & (idx == i))[0]) for i in range(c)]
        assert np.array_equal(sib[mine], s_at) and np.array_equal(pos[mine], p_at) and all(roots[j].tobytes() == snap.root for j in mine), c
    # one count for all paths, without the roots; no paths at all
    s17, p17 = tree.open([8, 10, 13, 16, 16, 0], at=17)
    w = fresh70[17]
    assert np.array_equal(s17, w[2][[8, 10, 13, 16, 16, 0]]) and np.array_equal(p17, w[3][[8, 10, 13, 16, 16, 0]])
    assert p17[2, 0] == 0 and p17[3, 0] == 0 and s17[3, 0].tobytes() == bytes(96)      # [zero leaf, missing x 3]: the first slot
    empty = tree.open([], at=[], roots=True)
    assert empty[0].shape == (0, DEPTH, 3, 32) and empty[2].shape == (0, 32)
    assert_same_tree(tree_state(tree), fresh70[CAPACITY], "current")


def test_refusals_leave_outputs_and_tree_as_they_were(pkg, gpu, L):
    leaves = canonical_leaves(np.random.default_rng(40), 40)
    lib = gpu.lib
    with L.ZkTree(gpu, leaves[:20], capacity=40) as tree:
        assert tree.depth == 3
        before = tree_state(tree)

        def unchanged(what):
            assert tree.leaf_count == 20 and lib.qpgpu_zk_tree_leaf_count(tree.h) == 20, what
            assert_same_tree(tree_state(tree), before, what)

        def refused(call, *needles):
            with pytest.raises(pkg.QpGpuError) as e:
                call()
            assert e.value.code == EINVAL and all(s in str(e.value) for s in needles) and str(e.value).endswith(gpu.last_error()), str(e.value)
            unchanged(needles)

        refused(lambda: tree.snapshots_at([20, 0, 21]), "entry 1:", "count is 0")
        refused(lambda: tree.snapshots_at([1, 20, 21]), "entry 2:", "exceeds")
        refused(lambda: tree.snapshots_at([2 ** 64 - 1]), "entry 0:", "exceeds")
        refused(lambda: tree.open([0, 0, 0], at=[5, 0, 5]), "entry 1:", "count is 0")
        refused(lambda: tree.open([0, 0, 0], at=[5, 20, 21]), "entry 2:", "exceeds")
        refused(lambda: tree.open([4, 5, 0], at=[5, 5, 0]), "entry 1:", "index")          # an index equal to its count, before a later count of 0
        refused(lambda: tree.open([0, 19, 20], at=20), "entry 2:", "index")
        refused(lambda: tree.open([3], at=0), "entry 0:", "count is 0")
        refused(lambda: tree.truncate(0), "n is 0")
        refused(lambda: tree.truncate(21), "exceeds")
        refused(lambda: tree.truncate(40), "exceeds")                                     # within the capacity, above the count
        half = tree.snapshot()
        for count, depth, needle in ((0, 3, "count"), (21, 3, "count"), (20, 2, "depth")):
            half.count, half.depth = count, depth
            refused(lambda: tree.check(half), needle)
        # through the C interface: outputs are untouched, NULL pointers are refused, nothing to do is not an error
        fill = bytes([0xA5])
        snaps = ctypes.create_string_buffer(fill * (3 * 528), 3 * 528)
        sib = ctypes.create_string_buffer(fill * (3 * 3 * 96), 3 * 3 * 96); pos = ctypes.create_string_buffer(fill * 9, 9)
        roots = ctypes.create_string_buffer(fill * 96, 96)
        err = ctypes.create_string_buffer(160)
        u64x3 = ctypes.c_uint64 * 3
        assert lib.qpgpu_zk_tree_snapshots_at(tree.h, u64x3(20, 0, 21), 3, snaps) == EINVAL and "entry 1:" in gpu.last_error()
        assert lib.qpgpu_zk_tree_snapshots_at(tree.h, None, 3, snaps) == EINVAL and "null" in gpu.last_error()
        assert lib.qpgpu_zk_tree_snapshots_at(tree.h, u64x3(1, 2, 3), 3, None) == EINVAL and "null" in gpu.last_error()
        assert lib.qpgpu_zk_tree_snapshots_at(tree.h, None, 0, None) == 0
        assert lib.qpgpu_zk_tree_snapshot_check(tree.h, None) == EINVAL and "null" in gpu.last_error()
        assert lib.qpgpu_zk_tree_open_at_counts(tree.h, u64x3(5, 5, 21), u64x3(0, 4, 0), 3, sib, pos, roots) == EINVAL and "entry 2:" in gpu.last_error()
        assert lib.qpgpu_zk_tree_open_at_counts(tree.h, u64x3(5, 5, 5), u64x3(0, 5, 0), 3, sib, pos, roots) == EINVAL and "entry 1:" in gpu.last_error()
        for args in ((None, u64x3(), sib, pos), (u64x3(1, 1, 1), None, sib, pos), (u64x3(1, 1, 1), u64x3(), None, pos), (u64x3(1, 1, 1), u64x3(), sib, None)):
            assert lib.qpgpu_zk_tree_open_at_counts(tree.h, args[0], args[1], 3, args[2], args[3], roots) == EINVAL and "null" in gpu.last_error()
        assert lib.qpgpu_zk_tree_open_at_counts(tree.h, None, None, 0, None, None, None) == 0
        out = L.ZkSnapshot()
        assert lib.qpgpu_zk_tree_truncate(tree.h, 0, ctypes.addressof(out), err) == EINVAL and b"n is 0" in err.value
        assert lib.qpgpu_zk_tree_truncate(tree.h, 21, ctypes.addressof(out), err) == EINVAL and b"exceeds" in err.value
        assert lib.qpgpu_zk_tree_truncate(tree.h, 21, None, None) == EINVAL
        assert snaps.raw == fill * (3 * 528) and sib.raw == fill * (3 * 3 * 96) and pos.raw == fill * 9 and roots.raw == fill * 96
        assert bytes(out) == bytes(528)
        unchanged("the C interface")
        # roots_out may be NULL
        assert lib.qpgpu_zk_tree_open_at_counts(tree.h, u64x3(5, 20, 1), u64x3(4, 19, 0), 3, sib, pos, None) == 0 and roots.raw == fill * 96
        want = tree.open([4, 19, 0], at=[5, 20, 1])
        assert sib.raw == want[0].tobytes() and pos.raw == want[1].tobytes()
        # the next valid calls
        assert tree.truncate(20).count == 20
        unchanged("a truncate to the count")
        tree.append(leaves[20:29])
        assert_same_tree(tree_state(tree), fresh_state(gpu, L, leaves[:29], 3), "after the refusals")


@pytest.fixture(scope="module")
def forks(L):
    """fork A: 50 leaves; fork B: A's first 20, then 35 others, among them (tree index 27) the leaf of a spend"""
    rng = np.random.default_rng(7005)
    a = canonical_leaves(rng, 50)
    a[13] = ZERO
    a[16] = ZERO                                                # the truncate to 20 cuts a group that an all-zero leaf opens
    b = canonical_leaves(rng, 35)
    b[1] = ZERO                                                 # tree index 21, among present siblings
    secret, tc = canonical_leaves(rng, 1)[0], 77
    unsp = L.unspendable_account(secret)
    b[7] = L.zk_leaf_hash(unsp, tc, 0, 300)
    return a, b, (27, secret, tc, unsp)


@pytest.fixture(scope="module")
def reorged(gpu, L, forks):
    """10 leaves with room for 70 at depth 4; fork A to 25, 40, 50; truncate(20); fork B to 35, 55. Every step's state is recorded."""
    a, b, _ = forks
    tree = L.ZkTree(gpu, a[:10], depth=DEPTH, capacity=CAPACITY)
    rec = {"snap10": tree.snapshot()}
    rec["a25"] = tree.append(a[10:25]); rec["a40"] = tree.append(a[25:40]); rec["a50"] = tree.append(a[40:50])
    rec["a25_checked_on_a"] = tree.check(rec["a25"])
    rec["cut"] = tree.truncate(20)
    rec["count_after_cut"] = (tree.leaf_count, int(gpu.lib.qpgpu_zk_tree_leaf_count(tree.h)), tree.capacity)
    rec["state_after_cut"] = tree_state(tree)
    rec["snap10_checked"] = tree.check(rec["snap10"])
    rec["open_at_snap10"] = tree.open(range(10), at=rec["snap10"])
    rec["open_at_10"] = tree.open(range(10), at=10, roots=True)
    rec["b35"] = tree.append(b[:15])
    rec["state_b35"] = tree_state(tree)
    rec["b55"] = tree.append(b[15:])
    rec["state_b55"] = tree_state(tree)
    yield tree, rec
    tree.close()


def test_reorg_truncate_then_another_fork(pkg, gpu, L, forks, reorged):
    a, b, _ = forks
    tree, rec = reorged
    assert rec["a25_checked_on_a"] is True
    want20 = fresh_state(gpu, L, a[:20], DEPTH)
    assert rec["count_after_cut"] == (20, 20, CAPACITY)
    assert_same_tree(rec["state_after_cut"], want20, "truncated to 20")
    assert bytes(rec["cut"]) == want20[4] and rec["cut"].root == want20[1]
    want10 = fresh_state(gpu, L, a[:10], DEPTH)
    assert rec["snap10_checked"] is True and bytes(rec["snap10"]) == want10[4]
    for got in (rec["open_at_snap10"], rec["open_at_10"]):
        assert np.array_equal(got[0], want10[2]) and np.array_equal(got[1], want10[3])
    assert all(r.tobytes() == want10[1] for r in rec["open_at_10"][2])
    # fork B
    fork_b = a[:20] + b
    assert_same_tree(rec["state_b35"], fresh_state(gpu, L, fork_b[:35], DEPTH), "fork B at 35")
    want55 = fresh_state(gpu, L, fork_b, DEPTH)
    assert_same_tree(rec["state_b55"], want55, "fork B at 55")
    assert bytes(rec["b55"]) == want55[4] and tree.leaf_count == 55
    # fork A's snapshots pass the count and depth checks of open_at and are no snapshots of this tree any more
    for name, n in (("a25", 25), ("a40", 40), ("a50", 50)):
        stale = rec[name]
        assert stale.count == n and tree.check(stale) is False and "snapshot differs" in gpu.last_error(), n
        now = tree.snapshots_at([n])[0]
        assert bytes(now) != bytes(stale) and now.root != stale.root, n
        assert bytes(now) == fresh_state(gpu, L, fork_b[:n], DEPTH, paths=False)[4], n
    assert tree.check(rec["snap10"]) is True and tree.check(rec["cut"]) is True and tree.check(rec["b35"]) is True
    assert bytes(tree.snapshots_at([35])[0]) == bytes(rec["b35"])
    # a truncate to the leaf count changes nothing
    same = tree.truncate(55)
    assert bytes(same) == want55[4] and tree.leaf_count == 55
    assert_same_tree(tree_state(tree), want55, "truncate(55)")
    # a tree from the plain build truncates, and still refuses appends
    with L.ZkTree(gpu, a[:20], depth=DEPTH) as plain:
        cut = plain.truncate(13)
        want13 = fresh_state(gpu, L, a[:13], DEPTH)
        assert plain.leaf_count == 13 and plain.capacity == 20 and bytes(cut) == want13[4]
        assert_same_tree(tree_state(plain), want13, "plain, truncated")
        with pytest.raises(pkg.QpGpuError) as e:
            plain.append(a[13:14])
        assert e.value.code == EINVAL and "qpgpu_zk_tree_build" in str(e.value) and "capacity" in str(e.value)
        with pytest.raises(pkg.QpGpuError) as e:
            plain.truncate(14)
        assert e.value.code == EINVAL and "exceeds" in str(e.value)
        assert_same_tree(tree_state(plain), want13, "plain, after the refusals")


def test_truncate_below_a_wide_dirty_range(gpu, L):
    """5000 leaves at depth 7, back to 1300, 3000 others appended: 750 dirty parents at level 1 go through the ranged node kernel and
    188 at level 2 through the fused one, over nodes that the truncate left behind"""
    rng = np.random.default_rng(5000)
    old = canonical_leaves(rng, 5000)
    new = canonical_leaves(rng, 3000)
    with L.ZkTree(gpu, old, capacity=5000) as tree:
        assert tree.depth == 7
        cut = tree.truncate(1300)
        assert tree.leaf_count == 1300 and cut.count == 1300
        assert_same_tree(tree_state(tree, False), fresh_state(gpu, L, old[:1300], 7, paths=False), "truncated to 1300")
        grown = tree.append(new)
        assert tree.leaf_count == 4300 and tree.level_size(1) - 1300 // 4 == 750
        with L.ZkTree(gpu, old[:1300] + new, depth=7) as fresh:
            want = tree_state(fresh, False)
            assert_same_tree(tree_state(tree, False), want, "4300 leaves")
            assert bytes(grown) == want[4]
            sample = [0, 4299] + [int(i) for i in np.random.default_rng(64).integers(0, 4300, 62)]
            got, ref = tree.open(sample), fresh.open(sample)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            # and the tree at the cut, out of the regrown one
            at_cut = tree.open([0, 1299, 1296], at=1300, roots=True)
            assert all(r.tobytes() == cut.root for r in at_cut[2]) and bytes(tree.snapshots_at([1300])[0]) == bytes(cut)


def test_spend_proven_at_an_earlier_block_of_the_new_fork(pkg, gpu, L, forks, reorged):
    """After the reorg, the spend of fork B's first block (leaf 27, in the tree since count 35) is proven against that block's root with
    the tree at 55 leaves and no snapshot kept: the path and the root come from set_zk_path(tree, 27, at=35). The same path under a header
    that commits to the newest root has no witness."""
    _, _, (slot, secret, tc, unsp) = forks
    tree, rec = reorged
    assert tree.leaf_count == 55
    root35 = tree.open([slot], at=35, roots=True)[2][0].tobytes()
    assert root35 == rec["b35"].root and root35 != tree.root
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

    good, bh = inputs(root35)
    good.set_zk_path(tree, slot, at=35)
    assert good.zk_merkle_depth == DEPTH and good.get32("zk_tree_root") == root35
    by_snapshot, _ = inputs(root35)                                            # the kept snapshot gives the same inputs
    by_snapshot.set_zk_path(tree, slot, at=rec["b35"])
    assert bytes(by_snapshot) == bytes(good)
    stale, _ = inputs(tree.root)                                               # the newest header, the old path
    stale.set_zk_path(tree, slot, at=35).set32("zk_tree_root", tree.root)
    err = ctypes.create_string_buffer(160)
    check = L._lib().qpgpu_leaf_check_constraints
    assert check(ctypes.byref(good), err) == 0, err.value
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
