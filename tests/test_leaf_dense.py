"""The density-matched leaf circuit on the CPU (include/qpgpu_leaf.h: qpgpu_leaf_circuit_build_dense, qpgpu_leaf_commit_dense,
qpgpu_leaf_circuit_hash_hint_cells_dense): k independent statements of the leaf circuit in one trace, copy 0's 21 targets public, the
others private — a measurement and test object at the reference's row occupancy, not a protocol object. One copy is today's circuit
word for word; three copies share the constant and public-input rows, take three different CircuitInputs through the oracle's
generate_partial_witness, prove and verify; an unsatisfiable copy leaves no witness. tests/test_leaf_dense_gpu.py runs the same
circuits through the device."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc
import oracle_binding as ob

EINVAL = -1
LT, HINTS = 299, 12 * 61 + 4 * 16


def build_dense(pkg, copies, cfg=None, min_degree_bits=0):
    """qpgpu_leaf_circuit_build_dense through ctypes: (rc, err, pack, target_map, info, blinding cells)."""
    L = pkg.leaf._lib()
    n, nb = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(400)
    cp = None if cfg is None else ctypes.byref(cfg)
    rc = L.qpgpu_leaf_circuit_build_dense(copies, min_degree_bits, 0, None, cp, None, 0, ctypes.byref(n), None, None, None, 0, ctypes.byref(nb), err)
    if rc != 0:
        return rc, err.value, None, None, None, None
    pack = np.empty(n.value, dtype=np.uint64); tm = np.empty(copies * LT, dtype=np.uint64); info = np.zeros(16, dtype=np.uint64)
    blind = np.empty(nb.value, dtype=np.uint64)
    rc = L.qpgpu_leaf_circuit_build_dense(copies, min_degree_bits, 0, None, cp, pack.ctypes.data, pack.size, ctypes.byref(n), tm.ctypes.data, info.ctypes.data,
                                          blind.ctypes.data, blind.size, ctypes.byref(nb), err)
    return rc, err.value, pack, tm, info, blind


def build_cfg(pkg, cfg):
    L = pkg.leaf._lib()
    n, nb = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(400)
    cp = None if cfg is None else ctypes.byref(cfg)
    assert L.qpgpu_leaf_circuit_build_cfg(0, 0, 0, None, cp, None, 0, ctypes.byref(n), None, None, None, 0, ctypes.byref(nb), err) == 0, err.value
    pack = np.empty(n.value, dtype=np.uint64); tm = np.empty(LT, dtype=np.uint64); info = np.zeros(16, dtype=np.uint64); blind = np.empty(nb.value, dtype=np.uint64)
    assert L.qpgpu_leaf_circuit_build_cfg(0, 0, 0, None, cp, pack.ctypes.data, pack.size, ctypes.byref(n), tm.ctypes.data, info.ctypes.data,
                                          blind.ctypes.data, blind.size, ctypes.byref(nb), err) == 0, err.value
    return pack, tm, info, blind


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def three(L):
    """The circuit of three copies at its natural size and three different inputs: the dummy, test_inputs_0, a depth-16 spend."""
    return L.LeafCircuit(copies=3), [lc.dummy_inputs(L), lc.test_inputs(L, 0), lc.real_inputs(L, depth=16, seed=9)]


@pytest.mark.parametrize("config", [None, "private_batch"])
def test_one_copy_is_todays_circuit_word_for_word(pkg, L, config):
    cfg = None if config is None else pkg.circuit_config(config)
    want_pack, want_tm, want_info, want_blind = build_cfg(pkg, cfg)
    rc, err, pack, tm, info, blind = build_dense(pkg, 1, cfg)
    assert rc == 0, err
    assert np.array_equal(pack, want_pack) and np.array_equal(tm, want_tm) and np.array_equal(blind, want_blind) and np.array_equal(info, want_info)
    assert (blind.size > 0) == (config is not None)
    c = L.LeafCircuit(copies=1, config=config)
    assert np.array_equal(c.pack, want_pack) and np.array_equal(c.target_map, want_tm) and np.array_equal(c.blinding_cells, want_blind)
    # and the hint cells of one copy through the dense entry are the single circuit's
    n = ctypes.c_size_t(); err = ctypes.create_string_buffer(400); cells = np.empty(HINTS, dtype=np.uint64)
    assert L._lib().qpgpu_leaf_circuit_hash_hint_cells_dense(1, 0, 0, None, None if cfg is None else ctypes.byref(cfg), cells.ctypes.data, cells.size, ctypes.byref(n), err) == 0, err.value
    assert n.value == HINTS and np.array_equal(cells, c.hash_hint_cells)


def test_three_copies_share_the_rows_laid_once(pkg, L, three):
    dense, _ = three
    single = L.LeafCircuit()
    r1, r3 = single.info["rows_before_padding"], dense.info["rows_before_padding"]
    assert 2 * r1 < r3 < 3 * r1, (r1, r3)                       # the constant rows, the public-input hash and the PublicInputGate are laid once
    assert dense.info["rows_constant"] == single.info["rows_constant"] and dense.info["rows_public_input"] == 1
    assert dense.info["rows_poseidon2"] == 3 * 61 and dense.info["rows_poseidon"] == single.info["rows_poseidon"]
    h = pkg.pack_header(dense.pack)
    assert h["num_public_inputs"] == 21 and h["degree_bits"] == dense.info["degree_bits"] == (r3 - 1).bit_length()
    # copy 0 is laid first, exactly as the single circuit lays it: its logical targets sit in the same cells (those a constant row or the
    # public-input rows hold apart: build() lays these after all copies)
    tm = dense.target_map.reshape(3, LT)
    same = tm[0] == single.target_map
    assert same.mean() > 0.9
    sets = [set(row[row != L.NO_CELL].tolist()) for row in tm]
    assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])    # fresh targets: no cell serves two copies
    # (the eight exit-account targets constrain nothing: public inputs in copy 0, in no gate at all in a private copy)
    assert len(sets[0]) == len(set(single.target_map.tolist())) and len(sets[1]) == len(sets[2]) == len(sets[0]) - 8
    assert (tm[1:, 242:250] == L.NO_CELL).all() and np.count_nonzero(tm == L.NO_CELL) == 16
    hc = dense.hash_hint_cells
    assert hc.size == 3 * HINTS and np.unique(hc).size == hc.size
    assert np.array_equal(hc[:HINTS], single.hash_hint_cells)
    rows = (hc // np.uint64(135)).reshape(3, HINTS)
    # copy-major: a copy's first hash row lies after the previous copy's last statement (later cells may be represented in a half-filled
    # arithmetic row the previous copy opened, as the builder packs operations)
    p2 = rows[:, :12 * 61]
    assert p2[0].max() < p2[1][0] and p2[1].max() < p2[2][0]
    assert np.median(p2[0]) < np.median(p2[1]) < np.median(p2[2])


def test_oracle_witness_proof_and_public_inputs(pkg, orc, L, three):
    dense, xs = three
    traces = []
    for hints in (False, True):
        cells, values, pis = dense.commit(xs, hash_hints=hints)
        assert cells.size == values.size == 3 * LT - 16 + (3 * HINTS if hints else 0)      # (a private copy's exit accounts reach no cell)
        rc, wires, bad = orc.generate_witness(dense.pack, cells, values, pis)
        assert rc == orc.WIT_OK, (hints, bad // 135, bad % 135)
        traces.append(wires)
    plain_wires = traces[0]
    assert np.array_equal(traces[1], plain_wires)                   # honest hints change nothing
    # copy-major lists: copy c's assignments are qpgpu_leaf_commit's against its slice of the target map
    cells, values, pis = dense.commit(xs)
    single = L.LeafCircuit()
    tm = dense.target_map.reshape(3, LT)
    at = 0
    for c, x in enumerate(xs):
        c1 = np.empty(LT, dtype=np.uint64); v1 = np.empty(LT, dtype=np.uint64); p1 = np.empty(21, dtype=np.uint64)
        k = ctypes.c_size_t(); err = ctypes.create_string_buffer(160)
        row = np.ascontiguousarray(tm[c])
        assert L._lib().qpgpu_leaf_commit(ctypes.byref(x), row.ctypes.data, c1.ctypes.data, v1.ctypes.data, LT, ctypes.byref(k), p1.ctypes.data, err) == 0
        k = k.value
        assert np.array_equal(values[at:at + k], v1[:k]) and np.array_equal(cells[at:at + k], c1[:k])
        at += k
        if c == 0:
            assert pis.tolist() == p1.tolist()
    assert at == cells.size
    # the public inputs read out of the trace are copy 0's
    h = pkg.pack_header(dense.pack)
    oc = ob.OracleCircuit(orc, dense.pack)
    proof = oc.prove(plain_wires, pis)
    assert lc.proof_public_inputs(proof, 21).tolist() == pis.tolist() == single.commit(xs[0])[2].tolist()
    nul = [int(plain_wires[int(c) % 135, int(c) // 135]) for c in tm[0][:4]]                  # QPGPU_LT_NULLIFIER_HASH of copy 0
    assert nul == pis[4:8].tolist() == lc.digest_felts(xs[0].get32("nullifier"))
    nul2 = [int(plain_wires[int(c) % 135, int(c) // 135]) for c in tm[2][:4]]                 # copy 2's nullifier is in the trace, and private
    assert nul2 == lc.digest_felts(xs[2].get32("nullifier")) and nul2 != nul
    assert oc.verify(proof) == 0
    v = pkg.Verifier(dense.pack)
    assert v.verify(proof), v.reason
    assert h["num_public_inputs"] == 21
    # a proof is bound to copy 0's public inputs only
    flipped = bytearray(proof); flipped[-8 * 21] ^= 1
    assert not v.verify(bytes(flipped))
    v.close(); oc.close()


def test_a_flipped_secret_in_copy_two_alone_leaves_no_witness(orc, L, three):
    dense, xs = three
    bad = xs[2].copy(); bad.secret[3] ^= 1
    for hints in (False, True):
        cells, values, pis = dense.commit([xs[0], xs[1], bad], hash_hints=hints)
        rc, _, cell = orc.generate_witness(dense.pack, cells, values, pis)
        assert rc == orc.WIT_CONFLICT                               # "set twice": the unspendable account is no longer H(H(salt || secret))
        rows = dense.hash_hint_cells.reshape(3, HINTS) // np.uint64(135)
        assert cell // 135 >= int(rows[1].max())                    # the conflict lies in copy 2's rows (or in the shared rows after them)
    # the same flip in copy 0 or 1 is refused as well; all three honest is a witness (test above)
    for k in (0, 1):
        ins = list(xs); ins[k] = xs[k].copy(); ins[k].secret[3] ^= 1
        cells, values, pis = dense.commit(ins)
        assert orc.generate_witness(dense.pack, cells, values, pis)[0] == orc.WIT_CONFLICT
    # where the front-end itself refuses (malformed inputs), the message names the copy
    deep = xs[2].copy(); deep.zk_merkle_depth = 17
    with pytest.raises(ValueError) as e:
        dense.commit([xs[0], xs[1], deep])
    single = L.LeafCircuit()
    with pytest.raises(ValueError) as e1:
        single.commit(deep)
    assert str(e.value) == "copy 2: " + str(e1.value)
    with pytest.raises(ValueError) as e:
        dense.commit([deep, xs[1], xs[2]])
    assert str(e.value).startswith("copy 0: ")
    with pytest.raises(ValueError):
        dense.commit(xs[:2])


def test_bad_copies_are_refused_naming_the_argument(pkg, L):
    rc, err, *_ = build_dense(pkg, 0)
    assert rc == EINVAL and b"copies" in err
    for big in (1 << 20, 0xFFFFFFFF):
        rc, err, *_ = build_dense(pkg, big)
        assert rc == EINVAL and b"copies" in err, (big, err)
    with pytest.raises(pkg.QpGpuError) as e:
        L.LeafCircuit(copies=0)
    assert e.value.code == EINVAL and "copies" in str(e.value)
    with pytest.raises(pkg.QpGpuError) as e:
        L.LeafCircuit(fragment=L.FRAGMENT_NULLIFIER, copies=2)
    assert e.value.code == EINVAL and "fragment" in str(e.value)
    n = ctypes.c_size_t(); err = ctypes.create_string_buffer(400)
    assert L._lib().qpgpu_leaf_circuit_hash_hint_cells_dense(0, 0, 0, None, None, None, 0, ctypes.byref(n), err) == EINVAL and b"copies" in err.value
    # commit_dense: copies = 0, a null input and a short buffer are errors, not faults
    cnt = ctypes.c_size_t(); e160 = ctypes.create_string_buffer(160)
    tm = np.zeros(2 * LT, dtype=np.uint64); cells = np.zeros(2 * LT, dtype=np.uint64); vals = np.zeros(2 * LT, dtype=np.uint64)
    x = lc.dummy_inputs(L)
    ptrs = (ctypes.c_void_p * 2)(ctypes.addressof(x), None)
    f = L._lib().qpgpu_leaf_commit_dense
    assert f(ptrs, 0, tm.ctypes.data, cells.ctypes.data, vals.ctypes.data, 2 * LT, ctypes.byref(cnt), None, e160) == -1 and b"copies" in e160.value
    assert f(ptrs, 2, tm.ctypes.data, cells.ctypes.data, vals.ctypes.data, 2 * LT - 1, ctypes.byref(cnt), None, e160) == -1
    assert f(ptrs, 2, tm.ctypes.data, cells.ctypes.data, vals.ctypes.data, 2 * LT, ctypes.byref(cnt), None, e160) == -1 and e160.value.startswith(b"copy 1: ")
    assert cnt.value == 0 and not vals.any()


def test_hint_cells_of_a_poseidon2_hashed_circuit(L):
    """With the Poseidon2 gate as the inner hasher the public-input hash is made of Poseidon2 rows too; they are no call site of the leaf
    and carry no hint cells."""
    for copies in (1, 2):
        c = L.LeafCircuit(inner_hasher=1, copies=copies)
        assert c.info["rows_poseidon2"] > copies * 61 and c.info["rows_poseidon"] == 0
        hc = c.hash_hint_cells
        assert hc.size == copies * HINTS and np.unique(hc).size == hc.size


def test_dense_picks_the_largest_copies_that_fit(L):
    d = L.LeafCircuit.dense(10)
    assert d.info["degree_bits"] == 10 and d.info["rows_before_padding"] <= 1024
    more = L.LeafCircuit(copies=d.copies + 1)
    assert more.info["degree_bits"] == 11
    single = L.LeafCircuit()
    assert d.copies >= 1024 // single.info["rows_before_padding"]
    assert L.LeafCircuit.dense(single.info["degree_bits"]).copies == 1
    with pytest.raises(Exception):
        L.LeafCircuit.dense(5)
