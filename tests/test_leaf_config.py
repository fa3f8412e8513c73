"""The leaf circuit under a caller's CircuitConfig (include/qpgpu_leaf.h: qpgpu_leaf_circuit_build_cfg,
qpgpu_leaf_circuit_hash_hint_cells_cfg), on the CPU: WormholeProver::new(config) of the reference (wormhole/prover/src/lib.rs:137-149),
whose bench proves the leaf under wormhole_private_batch_circuit_config() — zero knowledge on — as well as under the leaf's own.
The default config gives today's packs word for word; a zero-knowledge config gives CircuitBuilder::blind's rows at the degree the
formula says, and the oracle proves such a circuit; configs the reference's validate_circuit_config refuses are refused in its words.
tests/test_leaf_config_gpu.py runs the same circuits through the device."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc
import oracle_binding as ob

EINVAL = -1
FRAGMENTS = (0, 1, 2, 3, 4)


def smallest_query_rounds(pkg):
    """The smallest fri_config.num_query_rounds qpgpu_validate_circuit_config admits."""
    q = 0
    while pkg.validate_circuit_config(pkg.circuit_config("private_batch", num_query_rounds=q)) is not None:
        q += 1
    return q


def reduced_zk_config(pkg):
    return pkg.circuit_config("private_batch", num_query_rounds=smallest_query_rounds(pkg))


def blind_counts(gates, cfg):
    """CircuitBuilder::blinding_counts restated: the smallest degree estimate 2^k >= the gate count that also holds its own blinding
    rows. Per estimate: ConstantArityBits(arity, final) reductions, D = 2. Returns (k, regular rows, Z row pairs)."""
    k = (gates - 1).bit_length()
    while True:
        d, steps = k, 0
        while d > cfg.reduction_final_poly_bits and d + cfg.rate_bits >= cfg.cap_height + cfg.reduction_arity_bits and d >= cfg.reduction_arity_bits:
            d, steps = d - cfg.reduction_arity_bits, steps + 1
        fri_openings = cfg.num_query_rounds * (1 + 2 * steps * ((1 << cfg.reduction_arity_bits) - 1) + 2 * (1 << d))
        regular, zs = 2 + fri_openings, 4 + fri_openings
        if gates + regular + 2 * zs <= 1 << k:
            return k, regular, zs
        k += 1


def build_cfg(pkg, fragment, cfg, min_degree_bits=0):
    """qpgpu_leaf_circuit_build_cfg through ctypes: (rc, err, pack, target_map, info, blinding cells)."""
    L = pkg.leaf._lib()
    n, nb = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(400)
    cp = None if cfg is None else ctypes.byref(cfg)
    rc = L.qpgpu_leaf_circuit_build_cfg(fragment, min_degree_bits, 0, None, cp, None, 0, ctypes.byref(n), None, None, None, 0, ctypes.byref(nb), err)
    if rc != 0:
        return rc, err.value, None, None, None, None
    pack = np.empty(n.value, dtype=np.uint64); tm = np.empty(299, dtype=np.uint64); info = np.zeros(16, dtype=np.uint64); blind = np.empty(nb.value, dtype=np.uint64)
    rc = L.qpgpu_leaf_circuit_build_cfg(fragment, min_degree_bits, 0, None, cp, pack.ctypes.data, pack.size, ctypes.byref(n), tm.ctypes.data, info.ctypes.data,
                                        blind.ctypes.data, blind.size, ctypes.byref(nb), err)
    return rc, err.value, pack, tm, info, blind


def build_old(pkg, fragment):
    L = pkg.leaf._lib()
    n = ctypes.c_size_t(); err = ctypes.create_string_buffer(160)
    assert L.qpgpu_leaf_circuit_build(fragment, 0, 0, None, None, 0, ctypes.byref(n), None, None, err) == 0
    pack = np.empty(n.value, dtype=np.uint64); tm = np.empty(299, dtype=np.uint64)
    assert L.qpgpu_leaf_circuit_build(fragment, 0, 0, None, pack.ctypes.data, pack.size, ctypes.byref(n), tm.ctypes.data, None, err) == 0
    return pack, tm


@pytest.mark.parametrize("fragment", FRAGMENTS)
def test_default_config_gives_todays_pack(pkg, fragment):
    want_pack, want_tm = build_old(pkg, fragment)
    for cfg in (None, pkg.circuit_config("leaf")):
        rc, err, pack, tm, info, blind = build_cfg(pkg, fragment, cfg)
        assert rc == 0, err
        assert np.array_equal(pack, want_pack) and np.array_equal(tm, want_tm) and blind.size == 0
    c = pkg.leaf.LeafCircuit(fragment=fragment)
    assert np.array_equal(c.pack, want_pack) and not c.zero_knowledge and c.blinding_cells.size == 0


@pytest.mark.parametrize("fragment", FRAGMENTS)
def test_zero_knowledge_pack(pkg, fragment):
    cfg = reduced_zk_config(pkg)
    plain = build_cfg(pkg, fragment, cfg.replace(zero_knowledge=0))
    rc, err, pack, tm, info, blind = build_cfg(pkg, fragment, cfg)
    assert rc == 0 and plain[0] == 0, err
    h = pkg.pack_header(pack)
    assert h["zero_knowledge"] == 1 and h["num_routed_wires"] == 60 and h["num_query_rounds"] == cfg.num_query_rounds
    gates = int(plain[4][1])                                   # rows before padding of the twin without blinding
    assert int(info[1]) == gates and np.array_equal(tm, plain[3])          # blinding rows move no logical target
    k, regular, zs = blind_counts(gates, cfg)
    assert h["degree_bits"] == int(info[0]) == max(5, (gates + regular + 2 * zs - 1).bit_length()) and h["degree_bits"] <= max(5, k)
    assert blind.size == regular * 135 + zs * 60
    assert np.unique(blind).size == blind.size
    rows = blind // np.uint64(135)
    assert int(rows.min()) >= gates and int(rows.max()) < gates + regular + 2 * zs
    # regular rows take every wire, the first row of every pair its routed wires
    assert np.array_equal(blind[:regular * 135], np.arange(gates * 135, (gates + regular) * 135, dtype=np.uint64))
    assert int((blind[regular * 135:] % np.uint64(135)).max()) == 59
    L = pkg.leaf._lib()
    err = ctypes.create_string_buffer(400)
    L.qpgpu_pack_validate.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    assert L.qpgpu_pack_validate(pack.ctypes.data, pack.size, err) == 0, err.value
    # the canonical configs themselves, through the pack header
    L.qpgpu_pack_config_is_canonical.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p]
    if fragment in (0, 4):
        canon = build_cfg(pkg, fragment, pkg.circuit_config("private_batch"))[2]
        assert L.qpgpu_pack_config_is_canonical(canon.ctypes.data, canon.size, 1, err) == 0, err.value
        assert L.qpgpu_pack_config_is_canonical(canon.ctypes.data, canon.size, 0, err) != 0 and b"leaf circuit config does not match" in err.value
        assert L.qpgpu_pack_config_is_canonical(pack.ctypes.data, pack.size, 1, err) != 0 and b"num_query_rounds" in err.value


def test_full_leaf_degree_under_the_canonical_zk_config(pkg):
    """28 queries; at 2^14 rows ConstantArityBits(4, 5) reduces three times (14 -> 10 -> 6 -> 2) and leaves 4 coefficients:
    fri_openings = 28 * (1 + 2 * 45 + 2 * 4) = 2 772, so 2 774 regular rows and 2 776 pairs beside the leaf's own 236 rows (60 routed wires
    hold 15 operations per ArithmeticGate row, not 20) — 8 562 rows, more than 2^13 (where two reductions and 32 coefficients would need
    10 746)."""
    c = pkg.leaf.LeafCircuit(config="private_batch")
    gates = c.info["rows_before_padding"]
    k, regular, zs = blind_counts(gates, c.config)
    assert gates == 236 and (k, regular, zs) == (14, 2774, 2776) and c.info["degree_bits"] == 14 and c.zero_knowledge
    assert c.blinding_cells.size == 2774 * 135 + 2776 * 60 == 541050


def test_refusals_carry_the_references_message(pkg):
    L = pkg.leaf._lib()
    for field, value in (("rate_bits", 9), ("rate_bits", 2), ("cap_height", 9), ("num_query_rounds", 0)):
        for level in ("leaf", "private_batch"):
            cfg = pkg.circuit_config(level, **{field: value})
            want = pkg.validate_circuit_config(cfg)
            assert want is not None, (field, value)
            rc, err, *_ = build_cfg(pkg, 0, cfg)
            assert rc == EINVAL and err == want.encode(), (field, value, err)
            n = ctypes.c_size_t(); e2 = ctypes.create_string_buffer(400)
            assert L.qpgpu_leaf_circuit_hash_hint_cells_cfg(0, 0, None, ctypes.byref(cfg), None, 0, ctypes.byref(n), e2) == EINVAL and e2.value == want.encode()
            with pytest.raises(pkg.QpGpuError) as e:
                pkg.leaf.LeafCircuit(config=cfg)
            assert e.value.code == EINVAL and want in str(e.value)
    # fields the native builder does not model are refused by name, never ignored
    for field, value in (("security_bits", 128), ("use_base_arithmetic_gate", 0)):
        cfg = pkg.circuit_config("leaf", **{field: value})
        assert pkg.validate_circuit_config(cfg) is None
        rc, err, *_ = build_cfg(pkg, 0, cfg)
        assert rc == EINVAL and field.encode() in err, err
    # what the builder cannot lay out is refused with its reason
    rc, err, *_ = build_cfg(pkg, 0, pkg.circuit_config("leaf", max_quotient_degree_factor=7))
    assert rc == EINVAL and b"max_quotient_degree_factor" in err
    with pytest.raises(ValueError):
        pkg.leaf.LeafCircuit(config="no_such_level")


def test_reduction_strategy_knobs(pkg):
    """reduction_arity_bits 1..4 and reduction_final_poly_bits 0..8 are taken, and the pack carries ConstantArityBits' list for
    them; 0, 5 and 9 are refused by the builder and by LeafCircuit with a message naming the field and the value."""
    import fri_schedules as fs
    for ab in (1, 2, 3, 4):
        for fin in (0, 2, 5, 8):
            cfg = pkg.circuit_config("leaf", reduction_arity_bits=ab, reduction_final_poly_bits=fin)
            assert pkg.validate_circuit_config(cfg) is None
            rc, err, pack, *_ = build_cfg(pkg, 0, cfg)
            assert rc == 0, err
            h = pkg.pack_header(pack)
            assert [int(x) for x in pack[18:18 + h["num_arity_rounds"]]] == fs.constant_arity(h["degree_bits"], 3, 4, ab, fin), (ab, fin)
    # the reference's config policy does not look at the reduction strategy; the builder's own range check refuses by name
    for field, value, needle in (("reduction_arity_bits", 0, b"arity_bits (0) must be 1..4"), ("reduction_arity_bits", 5, b"arity_bits (5) must be 1..4"),
                                 ("reduction_final_poly_bits", 9, b"final_poly_bits (9) must be <= 8")):
        cfg = pkg.circuit_config("leaf", **{field: value})
        assert pkg.validate_circuit_config(cfg) is None
        rc, err, *_ = build_cfg(pkg, 0, cfg)
        assert rc == EINVAL and needle in err, (field, value, err)
        with pytest.raises(pkg.QpGpuError) as e:
            pkg.leaf.LeafCircuit(config=cfg)
        assert e.value.code == EINVAL and needle.decode() in str(e.value)


def test_hint_cells_are_those_of_the_plain_circuit(pkg):
    L = pkg.leaf
    cfg = reduced_zk_config(pkg)
    zk = L.LeafCircuit(config=cfg)
    plain = L.LeafCircuit(config=cfg.replace(zero_knowledge=0))          # the twin without blinding (60 routed wires lay the rows out their own way)
    assert zk.hash_hint_cells.size == L.HASH_HINTS == 796 and np.array_equal(zk.hash_hint_cells, plain.hash_hint_cells)
    assert np.array_equal(L.LeafCircuit(config="leaf").hash_hint_cells, L.LeafCircuit().hash_hint_cells)
    assert not np.intersect1d(zk.hash_hint_cells, zk.blinding_cells).size
    # commit: [logical targets][hash hints][blinding cells], the blinding cells without values
    x = lc.real_inputs(L, depth=3)
    cells, values, pis = zk.commit(x, hash_hints=True, device_blinding=True)
    nb = zk.blinding_cells.size
    assert cells.size == values.size + nb and np.array_equal(cells[-nb:], zk.blinding_cells) and np.array_equal(cells[-nb - 796:-nb], zk.hash_hint_cells)
    c0, v0, p0 = plain.commit(x, hash_hints=True)
    assert np.array_equal(cells[:-nb], c0) and np.array_equal(values, v0) and pis.tolist() == p0.tolist()


def test_oracle_proves_the_zero_knowledge_leaf(pkg, orc):
    """generate_partial_witness over commit's assignments plus seeded values for the blinding cells, the proof with seeded salts; the
    library's host verifier and oracle/verify.c accept it and reject it with one public-input word changed."""
    L = pkg.leaf
    zk = L.LeafCircuit(config=reduced_zk_config(pkg))
    h = pkg.pack_header(zk.pack)
    x = lc.dummy_inputs(L)
    cells, values, pis = zk.commit(x, device_blinding=True)
    rnd = np.empty(zk.blinding_cells.size, dtype=np.uint64)
    err = ctypes.create_string_buffer(400)
    rfe = pkg.load_library().qpgpu_random_field_elements
    rfe.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    assert rfe(bytes([7] * 32), rnd.ctypes.data, rnd.size, err) == 0
    rc, wires, _ = orc.generate_witness(zk.pack, cells, np.concatenate([values, rnd]), pis)
    assert rc == orc.WIT_OK
    # everything that is not a blinding row is the plain circuit's witness; the pair rows carry equal routed wires
    plain = L.LeafCircuit(config=zk.config.replace(zero_knowledge=0))
    rc, pw, _ = orc.generate_witness(plain.pack, *plain.commit(x))
    gates = zk.info["rows_before_padding"]
    assert rc == orc.WIT_OK and np.array_equal(wires[:, :gates], pw[:, :gates])
    regular = blind_counts(gates, zk.config)[1]
    assert np.array_equal(wires[:60, gates + regular], wires[:60, gates + regular + 1]) and int(wires[:, gates:gates + regular].min()) > 0
    oc = ob.OracleCircuit(orc, zk.pack)
    proof = oc.prove(wires, pis, seed=11)
    assert proof != oc.prove(wires, pis, seed=12) and lc.proof_public_inputs(proof, 21).tolist() == pis.tolist()
    ver = pkg.Verifier(zk.pack)
    assert oc.verify(proof) == 0 and ver.verify(proof)
    assert h["zero_knowledge"] == 1 and h["degree_bits"] == zk.info["degree_bits"]
    bad = bytearray(proof); bad[len(bad) - 8 * 21 + 8 * 3] ^= 1            # volume_fee_bps
    assert oc.verify(bytes(bad)) != 0 and not ver.verify(bytes(bad))
    ver.close(); oc.close()
