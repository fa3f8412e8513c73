"""Host-side mirror of the reference's leaf prover surface over include/qpgpu_leaf.h (ctypes only; the work is in libqpgpu.so):

    WormholeCircuit::new(config).build_prover()   wormhole/circuit/src/circuit.rs:115-152,210-212   -> LeafCircuit(config=...)
    WormholeProver::new(config)                   wormhole/prover/src/lib.rs:137-149                -> LeafProver(pkg, gpu, LeafCircuit(config=...))
    WormholeProver::commit(&inputs)               wormhole/prover/src/lib.rs:156-163,187-221        -> LeafCircuit.commit(inputs)
    WormholeProver::prove()                       wormhole/prover/src/lib.rs:171-175                -> LeafProver.prove(inputs)

`CircuitInputs` is `LeafInputs` (the C struct qpgpu_leaf_inputs). The circuit is the reference's statement restated on the
library's native builder (csrc/builder.hpp, csrc/leaf_circuit.cpp); see the header for what cannot match the fork offline.
"""
import ctypes
import weakref

import numpy as np

from .binding import CONFIG_ERR_CAP, QpGpuError, as_circuit_config, load_library

EINVAL = -1                            # QPGPU_EINVAL (include/qpgpu.h)

MAX_DEPTH, DIGEST_LEN, LT_COUNT, PUBLIC_INPUTS = 16, 110, 299, 21
HASH_HINTS = 12 * 61 + 4 * 16          # QPGPU_LEAF_HASH_HINTS: 61 sponge states + the Merkle walk's running hash per level
FRAGMENT_FULL, FRAGMENT_BLOCK_HEADER, FRAGMENT_UNSPENDABLE_ACCOUNT, FRAGMENT_NULLIFIER, FRAGMENT_FAKE_LEAF = 0, 1, 2, 3, 4
NO_CELL = 0xFFFFFFFFFFFFFFFF
INFO_FIELDS = ("degree_bits", "rows_before_padding", "gates_after_targets", "gates_unspendable_account", "gates_zk_merkle_proof",
               "gates_block_number_range_check", "gates_connect_shared_targets", "rows_arithmetic", "rows_base_sum", "rows_poseidon2",
               "rows_poseidon", "rows_constant", "rows_public_input", "rows_noop", "free_standing_generators", "selector_polynomials")


class LeafInputs(ctypes.Structure):
    """qpgpu_leaf_inputs = CircuitInputs (wormhole/circuit/src/inputs.rs:30-83)."""
    _fields_ = [("asset_id", ctypes.c_uint32), ("output_amount_1", ctypes.c_uint32), ("output_amount_2", ctypes.c_uint32),
                ("volume_fee_bps", ctypes.c_uint32),
                ("nullifier", ctypes.c_uint8 * 32), ("exit_account_1", ctypes.c_uint8 * 32), ("exit_account_2", ctypes.c_uint8 * 32),
                ("block_hash", ctypes.c_uint8 * 32), ("block_number", ctypes.c_uint32),
                ("secret", ctypes.c_uint8 * 32), ("transfer_count", ctypes.c_uint64),
                ("unspendable_account", ctypes.c_uint8 * 32), ("parent_hash", ctypes.c_uint8 * 32), ("state_root", ctypes.c_uint8 * 32),
                ("extrinsics_root", ctypes.c_uint8 * 32), ("digest", ctypes.c_uint8 * DIGEST_LEN), ("input_amount", ctypes.c_uint32),
                ("zk_tree_root", ctypes.c_uint8 * 32), ("zk_merkle_depth", ctypes.c_uint32),
                ("zk_merkle_siblings", ctypes.c_uint8 * (MAX_DEPTH * 3 * 32)), ("zk_merkle_positions", ctypes.c_uint8 * MAX_DEPTH)]

    def set32(self, name, data):
        data = bytes(data)
        assert len(data) == 32, name
        ctypes.memmove(getattr(self, name), data, 32)
        return self

    def get32(self, name):
        return bytes(getattr(self, name))

    def copy(self):
        other = LeafInputs()
        ctypes.memmove(ctypes.byref(other), ctypes.byref(self), ctypes.sizeof(LeafInputs))
        return other

    def set_zk_path(self, tree, index, at=None):
        """The Merkle path of leaf `index` of a ZkTree: zk_tree_root, zk_merkle_depth, the sorted siblings and the positions (levels past
        the depth zeroed). at: a ZkSnapshot of the tree, or the leaf count it had then — the path and the root are those of the tree as
        it stood then."""
        root = None
        if at is None or isinstance(at, ZkSnapshot):
            siblings, positions = tree.open([index], at=at)
        else:
            siblings, positions, roots = tree.open([index], at=at, roots=True)
            root = roots[0].tobytes()
        ctypes.memset(self.zk_merkle_siblings, 0, MAX_DEPTH * 96)
        ctypes.memset(self.zk_merkle_positions, 0, MAX_DEPTH)
        ctypes.memmove(self.zk_merkle_siblings, siblings.ctypes.data, tree.depth * 96)
        ctypes.memmove(self.zk_merkle_positions, positions.ctypes.data, tree.depth)
        self.zk_merkle_depth = tree.depth
        return self.set32("zk_tree_root", root if root is not None else tree.root if at is None else at.root)


def _lib():
    L = load_library()
    if not getattr(L, "_leaf_sigs", False):
        c = ctypes
        L.qpgpu_leaf_circuit_build.restype = c.c_int
        L.qpgpu_leaf_circuit_build.argtypes = [c.c_uint, c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t),
                                               c.c_void_p, c.c_void_p, c.c_char_p]
        L.qpgpu_leaf_circuit_build_cfg.restype = c.c_int
        L.qpgpu_leaf_circuit_build_cfg.argtypes = [c.c_uint, c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t),
                                                   c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L.qpgpu_leaf_circuit_hash_hint_cells_cfg.restype = c.c_int
        L.qpgpu_leaf_circuit_hash_hint_cells_cfg.argtypes = [c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L.qpgpu_leaf_circuit_build_dense.restype = c.c_int
        L.qpgpu_leaf_circuit_build_dense.argtypes = [c.c_uint, c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t),
                                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L.qpgpu_leaf_circuit_hash_hint_cells_dense.restype = c.c_int
        L.qpgpu_leaf_circuit_hash_hint_cells_dense.argtypes = [c.c_uint, c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L.qpgpu_leaf_commit_dense.restype = c.c_int
        L.qpgpu_leaf_commit_dense.argtypes = [c.c_void_p, c.c_uint, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.c_char_p]
        L.qpgpu_leaf_commit.restype = c.c_int
        L.qpgpu_leaf_commit.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.c_char_p]
        L.qpgpu_leaf_check_constraints.restype = c.c_int
        L.qpgpu_leaf_check_constraints.argtypes = [c.c_void_p, c.c_char_p]
        L.qpgpu_leaf_unspendable_account.argtypes = [c.c_void_p, c.c_size_t, c.c_char_p, c.c_void_p]
        L.qpgpu_leaf_nullifier.argtypes = [c.c_void_p, c.c_size_t, c.c_char_p, c.c_uint64, c.c_void_p]
        L.qpgpu_leaf_block_hash.argtypes = [c.c_void_p, c.c_size_t, c.c_char_p, c.c_uint32, c.c_char_p, c.c_char_p, c.c_char_p, c.c_char_p, c.c_void_p]
        L.qpgpu_zk_leaf_hash.argtypes = [c.c_char_p, c.c_uint64, c.c_uint32, c.c_uint32, c.c_void_p]
        L.qpgpu_zk_proof_from_unsorted.argtypes = [c.c_char_p, c.c_char_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_char_p]
        L.qpgpu_leaf_circuit_hash_hint_cells.restype = c.c_int
        L.qpgpu_leaf_circuit_hash_hint_cells.argtypes = [c.c_uint, c.c_int, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L.qpgpu_leaf_hash_hints.restype = c.c_int
        L.qpgpu_leaf_hash_hints.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_char_p]
        L._leaf_sigs = True
    return L


# ---- the hash-deriving helpers of qpgpu_leaf.h (KAT-pinned Poseidon2 sponge), as bytes -> bytes ----
def unspendable_account(secret):
    out = ctypes.create_string_buffer(32)
    assert _lib().qpgpu_leaf_unspendable_account(None, 0, bytes(secret), out) == 0
    return out.raw


def nullifier(secret, transfer_count):
    out = ctypes.create_string_buffer(32)
    assert _lib().qpgpu_leaf_nullifier(None, 0, bytes(secret), transfer_count, out) == 0
    return out.raw


def block_hash(parent_hash, block_number, state_root, extrinsics_root, zk_tree_root, digest):
    out = ctypes.create_string_buffer(32)
    assert _lib().qpgpu_leaf_block_hash(None, 0, bytes(parent_hash), block_number, bytes(state_root), bytes(extrinsics_root), bytes(zk_tree_root),
                                        bytes(digest), out) == 0
    return out.raw


def zk_leaf_hash(to_account, transfer_count, asset_id, input_amount):
    out = ctypes.create_string_buffer(32)
    assert _lib().qpgpu_zk_leaf_hash(bytes(to_account), transfer_count, asset_id, input_amount, out) == 0
    return out.raw


def zk_proof_from_unsorted(leaf_hash, unsorted_siblings):
    """ZkMerkleProof::from_unsorted: (sorted siblings [depth][3][32] as bytes, positions, root)."""
    depth = len(unsorted_siblings)
    flat = b"".join(bytes(s) for lvl in unsorted_siblings for s in lvl)
    so = ctypes.create_string_buffer(max(96 * depth, 1)); po = ctypes.create_string_buffer(max(depth, 1)); root = ctypes.create_string_buffer(32)
    err = ctypes.create_string_buffer(160)
    if _lib().qpgpu_zk_proof_from_unsorted(bytes(leaf_hash), flat, depth, so, po, root, err) != 0:
        raise ValueError(err.value.decode())
    return so.raw[:96 * depth], list(po.raw[:depth]), root.raw


# qpgpu_zk_leaf: what a leaf of the chain's ZK tree hashes
ZK_LEAF_DTYPE = np.dtype([("to_account", np.uint8, 32), ("transfer_count", "<u8"), ("asset_id", "<u4"), ("input_amount", "<u4")])
ZK_TREE_FROM_TRANSFERS = 1


def _zk_transfers(transfers):
    """[(to_account, transfer_count, asset_id, input_amount), ...] or an array of ZK_LEAF_DTYPE -> contiguous qpgpu_zk_leaf records"""
    if isinstance(transfers, np.ndarray) and transfers.dtype == ZK_LEAF_DTYPE:
        return np.ascontiguousarray(transfers).reshape(-1)
    rec = np.zeros(len(transfers), dtype=ZK_LEAF_DTYPE)
    for i, (acct, tc, asset, amount) in enumerate(transfers):
        acct = bytes(acct)
        assert len(acct) == 32, "to_account is 32 bytes"
        rec[i] = (np.frombuffer(acct, dtype=np.uint8), tc, asset, amount)
    return rec


def _zk_hashes(leaves):
    """bytes (count x 32), an array of that many bytes, or a list of 32-byte strings -> uint8 [count, 32]"""
    if isinstance(leaves, (list, tuple)):
        leaves = b"".join(bytes(h) for h in leaves)
    a = np.frombuffer(leaves, dtype=np.uint8) if isinstance(leaves, (bytes, bytearray, memoryview)) else np.ascontiguousarray(leaves, dtype=np.uint8)
    if a.size % 32:
        raise ValueError("leaf hashes are 32 bytes each")
    return np.ascontiguousarray(a).reshape(-1, 32)


def zk_leaf_hash_batch(gpu, transfers):
    """qpgpu_zk_leaf_hash of every transfer, on the device: uint8 [count, 32]."""
    rec = _zk_transfers(transfers)
    out = np.empty((rec.size, 32), dtype=np.uint8)
    gpu._check(gpu.lib.qpgpu_zk_leaf_hash_batch(gpu.ctx, rec.ctypes.data, rec.size, out.ctypes.data))
    return out


class ZkSnapshot(ctypes.Structure):
    """qpgpu_zk_snapshot: the tree as it stood at `count` leaves — the last node of every level above the leaves. 528 bytes, kept by
    the caller per block; ZkTree.open(indices, at=snapshot) opens paths that lead to its root."""
    _fields_ = [("count", ctypes.c_uint64), ("depth", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("last", (ctypes.c_uint8 * 32) * MAX_DEPTH)]

    @property
    def root(self):
        return bytes(self.last[self.depth - 1]) if 1 <= self.depth <= MAX_DEPTH else None

    def __eq__(self, other):
        return isinstance(other, ZkSnapshot) and bytes(self) == bytes(other)

    __hash__ = None


class ZkTree:
    """The chain's 4-ary ZK Merkle tree of one block, resident on the device (qpgpu_zk_tree_*): built from leaf hashes (`leaves`) or from
    the transfers themselves (`transfers`, hashed on the device too). depth = 0 is the smallest depth that holds the leaves. Raises
    QpGpuError(QPGPU_EINVAL) for arguments the library refuses, a leaf hash with a non-canonical limb among them.
    capacity: room for that many leaves (qpgpu_zk_tree_build_reserved; depth = 0 is then the smallest depth that holds the capacity):
    append() takes each later block's leaves, and open(indices, at=snapshot) opens paths at the root of an earlier block; open(indices,
    at=counts) does so with no snapshot kept, snapshots_at() and check() derive and check snapshots, truncate() follows a reorg."""

    def __init__(self, gpu, leaves=None, transfers=None, depth=0, flags=None, capacity=None):
        if (leaves is None) == (transfers is None):
            raise ValueError("ZkTree: give the leaf hashes or the transfers")
        data = _zk_hashes(leaves) if transfers is None else _zk_transfers(transfers)
        count = data.shape[0]
        if flags is None:
            flags = 0 if transfers is None else ZK_TREE_FROM_TRANSFERS
        self.gpu, self.h = gpu, None
        h = ctypes.c_void_p(); err = ctypes.create_string_buffer(160)
        if capacity is None:
            rc = gpu.lib.qpgpu_zk_tree_build(gpu.ctx, data.ctypes.data if count else None, count, depth, flags, ctypes.byref(h), err)
        else:
            rc = gpu.lib.qpgpu_zk_tree_build_reserved(gpu.ctx, data.ctypes.data if count else None, count, capacity, depth, flags, ctypes.byref(h), err)
        if rc != 0:
            assert not h.value, "a refused build leaves no handle"
            raise QpGpuError(rc, err.value.decode())
        self.h = h
        self.depth = int(gpu.lib.qpgpu_zk_tree_depth(h))
        self.leaf_count = int(gpu.lib.qpgpu_zk_tree_leaf_count(h))
        self.capacity = int(gpu.lib.qpgpu_zk_tree_capacity(h))
        self._root = None

    def append(self, leaves=None, transfers=None):
        """More leaves behind the last (qpgpu_zk_tree_append), as leaf hashes or as transfers: the ZkSnapshot after the append. A refused
        append (QpGpuError(QPGPU_EINVAL): nothing to append, no room, a tree built without capacity, a non-canonical leaf hash) leaves the
        tree as it was."""
        if (leaves is None) == (transfers is None):
            raise ValueError("ZkTree.append: give the leaf hashes or the transfers")
        data = _zk_hashes(leaves) if transfers is None else _zk_transfers(transfers)
        k = data.shape[0]
        snap = ZkSnapshot(); err = ctypes.create_string_buffer(160)
        rc = self.gpu.lib.qpgpu_zk_tree_append(self.h, data.ctypes.data if k else None, k, 0 if transfers is None else ZK_TREE_FROM_TRANSFERS, ctypes.addressof(snap), err)
        if rc != 0:
            raise QpGpuError(rc, err.value.decode())
        self.leaf_count = int(self.gpu.lib.qpgpu_zk_tree_leaf_count(self.h))
        self._root = None
        return snap

    def snapshot(self):
        """The ZkSnapshot of the tree as it stands (qpgpu_zk_tree_snapshot)."""
        snap = ZkSnapshot()
        self.gpu._check(self.gpu.lib.qpgpu_zk_tree_snapshot(self.h, ctypes.addressof(snap)))
        return snap

    @property
    def root(self):
        if self._root is None:
            out = ctypes.create_string_buffer(32)
            self.gpu._check(self.gpu.lib.qpgpu_zk_tree_root(self.h, out))
            self._root = out.raw
        return self._root

    def level_size(self, level):
        return (self.leaf_count + 4 ** level - 1) // 4 ** level

    def level(self, level, first=0, n=None):
        """Nodes first .. first + n (default: to the end) of a level, 0 = the leaves, depth = the root: uint8 [n, 32]."""
        if n is None:
            n = max(self.level_size(level) - first, 0) if level <= self.depth else 0
        out = np.empty((n, 32), dtype=np.uint8)
        self.gpu._check(self.gpu.lib.qpgpu_zk_tree_read_level(self.h, level, first, n, out.ctypes.data))
        return out

    def snapshots_at(self, counts):
        """The ZkSnapshots of the tree as it stood at each of `counts` leaves (1 .. leaf_count), derived on the device from the resident
        nodes in one call (qpgpu_zk_tree_snapshots_at): what append() or snapshot() returned at that count."""
        cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        snaps = (ZkSnapshot * cnt.size)()
        self.gpu._check(self.gpu.lib.qpgpu_zk_tree_snapshots_at(self.h, cnt.ctypes.data, cnt.size, ctypes.addressof(snaps)))
        return [ZkSnapshot.from_buffer_copy(s) for s in snaps]

    def check(self, snapshot):
        """Whether `snapshot` is the one this tree gives at snapshot.count (qpgpu_zk_tree_snapshot_check): False for one kept from a fork
        that truncate() has since abandoned. Raises QpGpuError(QPGPU_EINVAL) for a count of 0 or above leaf_count and for another depth."""
        rc = self.gpu.lib.qpgpu_zk_tree_snapshot_check(self.h, ctypes.addressof(snapshot))
        if rc == EINVAL and "snapshot differs" in self.gpu.last_error():
            return False
        self.gpu._check(rc)
        return True

    def truncate(self, n):
        """A reorg: back to the first n leaves (qpgpu_zk_tree_truncate), the ZkSnapshot at n. Afterwards the tree is the one built from
        those leaves, and appends continue from n. A refused truncate (QpGpuError(QPGPU_EINVAL): n = 0, n above leaf_count) leaves the
        tree as it was."""
        snap = ZkSnapshot(); err = ctypes.create_string_buffer(160)
        rc = self.gpu.lib.qpgpu_zk_tree_truncate(self.h, n, ctypes.addressof(snap), err)
        if rc != 0:
            raise QpGpuError(rc, err.value.decode())
        self.leaf_count = int(self.gpu.lib.qpgpu_zk_tree_leaf_count(self.h))
        self._root = None
        return snap

    def open(self, indices, at=None, roots=False):
        """The paths of many leaves in one call: (siblings uint8 [n, depth, 3, 32] in sorted order, positions uint8 [n, depth]).
        at: a ZkSnapshot of this tree — the paths of the tree as it stood then, leading to at.root (qpgpu_zk_tree_open_at); or a leaf
        count for all paths, or one per index — the paths of the tree as it stood at that count, no snapshot kept
        (qpgpu_zk_tree_open_at_counts). roots=True: also the root each path leads to, uint8 [n, 32]."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        sib = np.empty((idx.size, self.depth, 3, 32), dtype=np.uint8); pos = np.empty((idx.size, self.depth), dtype=np.uint8)
        if at is None:
            self.gpu._check(self.gpu.lib.qpgpu_zk_tree_open(self.h, idx.ctypes.data, idx.size, sib.ctypes.data, pos.ctypes.data))
            root = self.root if roots else None
        elif isinstance(at, ZkSnapshot):
            self.gpu._check(self.gpu.lib.qpgpu_zk_tree_open_at(self.h, ctypes.addressof(at), idx.ctypes.data, idx.size, sib.ctypes.data, pos.ctypes.data))
            root = at.root if roots else None
        else:
            cnt = np.ascontiguousarray(at, dtype=np.uint64).reshape(-1)
            if np.ndim(at) == 0:
                cnt = np.full(idx.size, cnt[0], dtype=np.uint64)
            if cnt.size != idx.size:
                raise ValueError("ZkTree.open: one count for all indices or one per index")
            out = np.empty((idx.size, 32), dtype=np.uint8)
            self.gpu._check(self.gpu.lib.qpgpu_zk_tree_open_at_counts(self.h, cnt.ctypes.data, idx.ctypes.data, idx.size, sib.ctypes.data, pos.ctypes.data,
                                                                      out.ctypes.data if roots else None))
            return (sib, pos, out) if roots else (sib, pos)
        if roots:
            return sib, pos, np.tile(np.frombuffer(root, dtype=np.uint8), (idx.size, 1))
        return sib, pos

    def close(self):
        if self.h:
            self.gpu.lib.qpgpu_zk_tree_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def dummy_circuit_inputs():
    """build_dummy_circuit_inputs (wormhole/aggregator/src/dummy_proof.rs:58-84,125-170): the CircuitInputs of the dummy leaf the
    batch layers pad with, and the reference bench's input (wormhole/prover/benches/prover.rs:31-42). Zero block hash, outputs,
    nullifier and exit accounts (the sentinel), depth-0 Merkle proof; secret / transfer count / state root / digest are the
    reference's DEFAULT_* constants, the unspendable account is derived from the secret."""
    x = LeafInputs()
    secret = bytes.fromhex("4c8587bd422e01d961acdc75e7d66f6761b7af7c9b1864a492f369c9d6724f05")
    x.asset_id, x.output_amount_1, x.output_amount_2, x.volume_fee_bps, x.block_number = 0, 0, 0, 10, 0
    x.transfer_count, x.input_amount, x.zk_merkle_depth = 4, 100, 0
    for name in ("nullifier", "exit_account_1", "exit_account_2", "block_hash", "parent_hash", "extrinsics_root", "zk_tree_root"):
        x.set32(name, bytes(32))
    x.set32("secret", secret).set32("unspendable_account", unspendable_account(secret))
    x.set32("state_root", bytes.fromhex("ae6e4ff0dca1ef5ede9dccc84365cecfab4e431c6f3086216bc3b819cdf0a893"))
    digest = bytes.fromhex("0806706f775f80e9b6b76b9e017313db7efd561ed0b046152db4e5093e5b040635f53430267be105706f775f0101") + bytes(61) + bytes.fromhex("124fe2")
    assert len(digest) == 110
    ctypes.memmove(x.digest, digest, 110)
    return x


class LeafCircuit:
    """WormholeCircuit::new(config) -> build_prover(): the circuit pack and the wire cell of every logical target. Host only.

    config: None (wormhole_leaf_circuit_config), the name of a canonical config ("leaf"; "private_batch" is the zero-knowledge one the
    reference's prover_create_proof_zk bench target uses), a binding.CircuitConfig, or any object / mapping with qpgpu_circuit_config's
    fields. A config the reference's validate_circuit_config refuses raises QpGpuError with its message."""

    def __init__(self, fragment=FRAGMENT_FULL, min_degree_bits=0, inner_hasher=0, p2_layout=None, config=None, copies=1):
        L = _lib()
        n = ctypes.c_size_t(); nb = ctypes.c_size_t()
        err = ctypes.create_string_buffer(CONFIG_ERR_CAP)
        lay = None if p2_layout is None else np.ascontiguousarray(p2_layout, dtype=np.uint64)
        layp = None if lay is None else lay.ctypes.data
        self.config = as_circuit_config(config)
        cfgp = None if self.config is None else ctypes.byref(self.config)
        if copies != 1 and fragment != FRAGMENT_FULL:
            raise QpGpuError(EINVAL, "LeafCircuit: copies other than 1 exist for the full circuit only (fragment must be FRAGMENT_FULL)")

        def build(pack, pack_cap, tmap, info, blind, blind_cap):
            # copies = 1 is qpgpu_leaf_circuit_build_cfg's circuit (word for word through either entry); the dense entry has no fragment
            if copies == 1:
                return L.qpgpu_leaf_circuit_build_cfg(fragment, min_degree_bits, inner_hasher, layp, cfgp, pack, pack_cap, ctypes.byref(n), tmap, info, blind, blind_cap, ctypes.byref(nb), err)
            return L.qpgpu_leaf_circuit_build_dense(copies, min_degree_bits, inner_hasher, layp, cfgp, pack, pack_cap, ctypes.byref(n), tmap, info, blind, blind_cap, ctypes.byref(nb), err)

        rc = build(None, 0, None, None, None, 0)
        if rc != 0:
            raise QpGpuError(rc, err.value.decode())
        self.copies = copies
        self.pack = np.empty(n.value, dtype=np.uint64)
        self.target_map = np.empty(copies * LT_COUNT, dtype=np.uint64)       # copy-major
        self.blinding_cells = np.empty(nb.value, dtype=np.uint64)       # CircuitBuilder::blind's random wires, drawn on the device per proof
        info = np.zeros(len(INFO_FIELDS), dtype=np.uint64)
        rc = build(self.pack.ctypes.data, self.pack.size, self.target_map.ctypes.data, info.ctypes.data, self.blinding_cells.ctypes.data, self.blinding_cells.size)
        if rc != 0:
            raise QpGpuError(rc, err.value.decode())
        self.info = {k: int(v) for k, v in zip(INFO_FIELDS, info)}
        self.fragment = fragment
        self.zero_knowledge = bool(self.pack[14])                       # header word 14 (csrc/circuit.hpp)
        self._build_args = (min_degree_bits, inner_hasher, layp, lay)
        self._hint_cells = None

    @classmethod
    def dense(cls, degree_bits, inner_hasher=0, p2_layout=None, config=None):
        """The density-matched leaf (qpgpu_leaf_circuit_build_dense: a measurement and test object, k statements of which one is public):
        the largest `copies` whose rows, blinding rows included, fit 2^degree_bits, padded to 2^degree_bits. Sizes are asked for with
        pack_out = NULL (a dozen host-only builds)."""
        L = _lib()
        lay = None if p2_layout is None else np.ascontiguousarray(p2_layout, dtype=np.uint64)
        cfg = as_circuit_config(config)

        def fits(k):
            n = ctypes.c_size_t(); info = np.zeros(len(INFO_FIELDS), dtype=np.uint64); err = ctypes.create_string_buffer(CONFIG_ERR_CAP)
            rc = L.qpgpu_leaf_circuit_build_dense(k, 0, inner_hasher, None if lay is None else lay.ctypes.data, None if cfg is None else ctypes.byref(cfg),
                                                  None, 0, ctypes.byref(n), None, info.ctypes.data, None, 0, None, err)
            if rc != 0 and k == 1:
                raise QpGpuError(rc, err.value.decode())
            return rc == 0 and int(info[0]) <= degree_bits

        if not fits(1):
            raise QpGpuError(EINVAL, "LeafCircuit.dense: one copy of the leaf circuit does not fit 2^%d rows" % degree_bits)
        lo, hi = 1, 2                                                   # fits(lo), and hi is the first candidate not known to fit
        while fits(hi):
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        return cls(copies=lo, min_degree_bits=degree_bits, inner_hasher=inner_hasher, p2_layout=p2_layout, config=config)

    @property
    def hash_hint_cells(self):
        """The cells of the 61 Poseidon2 rows' outputs, call sites in tag order, then the Merkle walk's running hashes — per copy, copy-major
        (qpgpu_leaf_circuit_hash_hint_cells_cfg / _dense); full circuit only."""
        if self._hint_cells is None:
            if self.fragment != FRAGMENT_FULL:
                raise ValueError("hash hints exist for the full leaf circuit only")
            cells = np.empty(self.copies * HASH_HINTS, dtype=np.uint64)
            n = ctypes.c_size_t(); err = ctypes.create_string_buffer(CONFIG_ERR_CAP)
            cfgp = None if self.config is None else ctypes.byref(self.config)
            if self.copies == 1:
                rc = _lib().qpgpu_leaf_circuit_hash_hint_cells_cfg(self._build_args[0], self._build_args[1], self._build_args[2], cfgp, cells.ctypes.data, cells.size, ctypes.byref(n), err)
            else:
                rc = _lib().qpgpu_leaf_circuit_hash_hint_cells_dense(self.copies, self._build_args[0], self._build_args[1], self._build_args[2], cfgp,
                                                                     cells.ctypes.data, cells.size, ctypes.byref(n), err)
            if rc != 0:
                raise QpGpuError(rc, err.value.decode())
            self._hint_cells = cells[:n.value].copy()
        return self._hint_cells

    def commit(self, inputs, hash_hints=False, device_blinding=False):
        """WormholeProver::commit: (cells, values, public_inputs[21]); raises ValueError with the reference's message. hash_hints=True
        appends the 732 sponge-state elements of the circuit's hash call sites and the Merkle walk's 16 running hashes, computed on the host (qpgpu_leaf_hash_hints): the same witness,
        with the 61 hash rows generated side by side and checked instead of one after the other. device_blinding=True (zero-knowledge
        circuits): the blinding cells are appended to the cell list WITHOUT values, [logical targets][hash hints][blinding cells] — stage s1
        draws them on the device (n_blinding = self.blinding_cells.size of Circuit.generate_witness_partial_batch_blinded_dev and
        ProvingPool.set_partial_cells).
        A circuit of several copies takes a list of `copies` inputs (qpgpu_leaf_commit_dense: inputs[c] feeds copy c, the public inputs are
        inputs[0]'s; one LeafInputs alone feeds every copy); the lists are copy-major: [logical targets, per copy][hash hints, per copy][blinding cells]."""
        ins = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * self.copies
        if len(ins) != self.copies:
            raise ValueError("commit: %d inputs for a circuit of %d copies" % (len(ins), self.copies))
        cap = self.copies * LT_COUNT
        cells = np.empty(cap, dtype=np.uint64); values = np.empty(cap, dtype=np.uint64); pis = np.empty(PUBLIC_INPUTS, dtype=np.uint64)
        n = ctypes.c_size_t(); err = ctypes.create_string_buffer(160)
        if self.copies == 1:
            rc = _lib().qpgpu_leaf_commit(ctypes.byref(ins[0]), self.target_map.ctypes.data, cells.ctypes.data, values.ctypes.data, LT_COUNT,
                                          ctypes.byref(n), pis.ctypes.data, err)
        else:
            ptrs = (ctypes.c_void_p * self.copies)(*[ctypes.addressof(x) for x in ins])
            rc = _lib().qpgpu_leaf_commit_dense(ptrs, self.copies, self.target_map.ctypes.data, cells.ctypes.data, values.ctypes.data, cap,
                                                ctypes.byref(n), pis.ctypes.data, err)
        if rc != 0:
            raise ValueError(err.value.decode())
        cells, values = [cells[:n.value]], [values[:n.value]]
        if hash_hints:
            hv = np.empty(self.copies * HASH_HINTS, dtype=np.uint64)
            for c, x in enumerate(ins):
                hn = ctypes.c_size_t()
                if _lib().qpgpu_leaf_hash_hints(ctypes.byref(x), hv[c * HASH_HINTS:].ctypes.data, HASH_HINTS, ctypes.byref(hn), err) != 0:
                    raise ValueError(("copy %d: " % c if self.copies > 1 else "") + err.value.decode())
                assert hn.value == HASH_HINTS
            cells.append(self.hash_hint_cells); values.append(hv)
        if device_blinding:
            cells.append(self.blinding_cells)
        return np.concatenate(cells), np.concatenate(values), self.public_inputs(pis)

    def describe(self, finding):
        """binding.format_finding's line for a Circuit.explain_witness finding of this circuit; for a COPY finding, followed by the logical
        targets (indices into target_map: the LT_* numbering of include/qpgpu_leaf.h, plus LT_COUNT per copy) that sit on either of
        its two cells. A reverse lookup of target_map, nothing more."""
        from .binding import FINDING_COPY, format_finding
        line = format_finding(self.pack, finding)
        if finding.kind != FINDING_COPY:
            return line
        nw = int(self.pack[2])                                          # header word 2: num_wires
        for what, cell in (("cell", finding.row * nw + finding.wire), ("source", finding.row_b * nw + finding.wire_b)):
            hits = [int(i) for i in np.nonzero(self.target_map == np.uint64(cell))[0]]
            if hits:
                line += "; %s = logical target%s %s" % (what, "" if len(hits) == 1 else "s", ", ".join(str(i) for i in hits))
        return line

    def public_inputs(self, pis21):
        """The circuit's own public inputs out of the leaf's 21 (a fragment circuit registers only some of them)."""
        if self.fragment == FRAGMENT_FULL:
            return pis21
        if self.fragment == FRAGMENT_BLOCK_HEADER:
            return np.ascontiguousarray(pis21[16:21])
        if self.fragment == FRAGMENT_NULLIFIER:
            return np.ascontiguousarray(pis21[4:8])
        return np.zeros(0, dtype=np.uint64)


class LeafProver:
    """WormholeProver over a loaded LeafCircuit: commit (host) -> stage s1 on the device -> stages s2..s12. For a zero-knowledge
    circuit stage s1 also draws the blinding rows' random wires on the device (fresh OS entropy per proof) and the proof's three
    blinded oracles are salted. blinding_seed (tests only): an integer that fixes both, the salts through
    Circuit.set_blinding_seed and the draw through the per-witness key, so that a proof's bytes can be reproduced."""

    def __init__(self, pkg, gpu, circuit, witness_check=False, hash_hints=False, blinding_seed=None):
        self.pkg, self.gpu, self.circuit, self.hash_hints, self.blinding_seed = pkg, gpu, circuit, hash_hints, blinding_seed
        self.circ = pkg.Circuit(gpu, circuit.pack)
        if witness_check:
            self.circ.set_witness_check(True)
        h = pkg.pack_header(circuit.pack)
        self.shape = (h["num_wires"], 1 << h["degree_bits"])
        self.d_wires = gpu.alloc(self.shape[0] * self.shape[1] * 8)
        self._pools = []

    def generate_witness(self, inputs):
        nb = self.circuit.blinding_cells.size
        cells, values, pis = self.circuit.commit(inputs, hash_hints=self.hash_hints, device_blinding=nb > 0)
        if nb == 0:
            self.circ.generate_witness_partial_dev(cells, values, pis, self.d_wires)
            return pis
        key = None if self.blinding_seed is None else int(self.blinding_seed).to_bytes(32, "little")
        st = self.circ.generate_witness_partial_batch_blinded_dev(cells, values[None], pis[None], self.d_wires, nb, key)
        if st[0] != 0:
            raise QpGpuError(st[0], self.gpu.last_error())
        return pis

    def prove(self, inputs):
        pis = self.generate_witness(inputs)
        if self.circuit.zero_knowledge and self.blinding_seed is not None:
            self.circ.set_blinding_seed(int(self.blinding_seed) & 0xFFFFFFFFFFFFFFFF)
        return self.circ.prove_dev(self.d_wires, pis), pis

    def witness(self):
        return self.d_wires.download().reshape(self.shape)

    def pool(self, workers=2, max_batch=4, devices=None):
        """A ProvingPool over the prover's circuit with its cell list resolved: [logical targets][hash hints, if used][blinding cells],
        the blinding cells (zero-knowledge circuits) drawn on the device per proof. Jobs go in through submit(); the caller closes it."""
        x = dummy_circuit_inputs() if self.circuit.fragment == FRAGMENT_FULL else LeafInputs()
        nb = int(self.circuit.blinding_cells.size)
        cells = self.circuit.commit(x, hash_hints=self.hash_hints, device_blinding=nb > 0)[0]      # the list is the same for every input
        pool = self.pkg.ProvingPool(self.circuit.pack, workers=workers, max_batch=max_batch, devices=devices)
        try:
            pool.set_partial_cells(cells, n_blinding=nb)
        except Exception:
            pool.close()
            raise
        self._pools = [r for r in self._pools if r() is not None and r().h] + [weakref.ref(pool)]     # for scrub(); the caller owns the pool
        return pool

    def scrub(self):
        """Overwrites what the last proofs left on the device: the prover's own circuit workspace and, for every open pool made by
        pool(), each worker's workspace, resident witnesses and partial-witness buffers (ProvingPool.scrub)."""
        self.circ.scrub()
        for r in self._pools:
            p = r()
            if p is not None and p.h:
                p.scrub()

    def submit(self, pool, inputs):
        """commit(inputs) queued on a pool made by pool(): the ticket for pool.wait(), which raises QpGpuError(-4) for inputs the
        circuit has no witness for — that ticket alone."""
        _, values, pis = self.circuit.commit(inputs, hash_hints=self.hash_hints)
        return pool.submit_partial(values, pis)

    def close(self):
        self.d_wires.free(scrub=True)
        self.circ.close()
