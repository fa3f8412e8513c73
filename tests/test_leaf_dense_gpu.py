"""The density-matched leaf circuit (qpgpu_leaf_circuit_build_dense: k statements of the leaf circuit in one trace, one of them public)
through the device: stage s1's witness equals the oracle's cell for cell and the proof its bytes, without and with hash hints; the
copies are independent, so the dependency levels do not grow with them; in a lockstep batch an unsatisfiable copy fails its witness
alone; the zero-knowledge config and the Poseidon2 proof hasher. Three copies at the circuit's natural size (2^10 rows)."""
import numpy as np
import pytest

import leaf_cases as lc
import oracle_binding as ob
from test_leaf_config import reduced_zk_config

pytestmark = pytest.mark.gpu
SEED = 0xD15E


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def three(L):
    return L.LeafCircuit(copies=3), [lc.dummy_inputs(L), lc.test_inputs(L, 0), lc.real_inputs(L, depth=16, seed=9)]


@pytest.fixture(scope="module")
def oracle_three(orc, three):
    """The oracle's witness and proof of the three inputs, computed once."""
    dense, xs = three
    cells, values, pis = dense.commit(xs)
    rc, wires, _ = orc.generate_witness(dense.pack, cells, values, pis)
    assert rc == orc.WIT_OK
    oc = ob.OracleCircuit(orc, dense.pack)
    proof = oc.prove(wires, pis)
    assert oc.verify(proof) == 0
    oc.close()
    return wires, proof, pis


@pytest.mark.parametrize("hints", [False, True], ids=["plain", "hinted"])
def test_witness_and_proof_equal_the_oracle(pkg, gpu, L, three, oracle_three, hints):
    dense, xs = three
    want_wires, want_proof, want_pis = oracle_three
    assert dense.info["degree_bits"] == 10
    pr = L.LeafProver(pkg, gpu, dense, hash_hints=hints)
    proof, pis = pr.prove(xs)
    assert np.array_equal(pr.witness(), want_wires)
    assert proof == want_proof and pis.tolist() == want_pis.tolist() == lc.proof_public_inputs(proof, 21).tolist()
    # the copies are independent: no more dependency levels than one copy has
    one = L.LeafProver(pkg, gpu, L.LeafCircuit(), hash_hints=hints)
    one.prove(xs[2])
    l1, l3 = one.circ.witness_info()[1], pr.circ.witness_info()[1]
    assert l3 <= l1, (l1, l3)
    assert pr.circ.witness_info()[0] > 2.5 * one.circ.witness_info()[0]          # and about three times the generator instances
    one.close(); pr.close()


def test_lockstep_batch_fails_the_witness_with_an_unsatisfiable_copy_alone(pkg, gpu, orc, L, three):
    dense, xs = three
    bad = xs[1].copy(); bad.secret[3] ^= 1
    sets = [xs, [xs[2], xs[0], xs[1]], [xs[0], bad, xs[2]], [xs[1], xs[1], xs[0]]]          # only witness 2 has an unsatisfiable copy 1
    for hints in (False, True):
        com = [dense.commit(s, hash_hints=hints) for s in sets]
        circ = pkg.Circuit(gpu, dense.pack, max_batch=4)
        nw, n = 135, 1 << dense.info["degree_bits"]
        d = gpu.alloc(4 * nw * n * 8)
        st = circ.generate_witness_partial_batch_dev(com[0][0], np.stack([c[1] for c in com]), np.stack([c[2] for c in com]), d)
        assert st == [0, 0, -4, 0], (hints, st)
        assert "witness 2" in gpu.last_error() and "set twice with different values" in gpu.last_error()
        good = [0, 1, 3]
        proofs = circ.prove_batch_dev([d.ptr + b * nw * n * 8 for b in good], [com[b][2] for b in good])
        oc = ob.OracleCircuit(orc, dense.pack)
        for b, p in zip(good, proofs):
            cells, values, pis = dense.commit(sets[b])
            rc, wires, _ = orc.generate_witness(dense.pack, cells, values, pis)
            assert rc == orc.WIT_OK and p == oc.prove(wires, pis), (hints, b)
        cells, values, pis = dense.commit(sets[2])
        assert orc.generate_witness(dense.pack, cells, values, pis)[0] == orc.WIT_CONFLICT
        oc.close(); circ.close(); d.free(scrub=True)


def zk_parity(pkg, gpu, orc, L, circuit, xs, hasher=0):
    pr = L.LeafProver(pkg, gpu, circuit, hash_hints=True, blinding_seed=SEED)
    ver = pkg.Verifier(circuit.pack, circuit=pr.circ, hasher=hasher)
    proof, pis = pr.prove(xs)
    got = pr.witness()
    b = circuit.blinding_cells
    blind = got[(b % np.uint64(135)).astype(np.int64), (b // np.uint64(135)).astype(np.int64)]
    cells, values, _ = circuit.commit(xs, device_blinding=True)
    rc, wires, _ = orc.generate_witness(circuit.pack, cells, np.concatenate([values, blind]), pis)
    assert rc == orc.WIT_OK and np.array_equal(got, wires)
    oc = ob.OracleCircuit(orc, circuit.pack)
    assert proof == oc.prove(wires, pis, seed=SEED) and oc.verify(proof) == 0
    oc.close()
    assert ver.verify(proof), ver.reason
    assert ver.verify_many([proof], gpu=gpu) == [True], ver.reasons                       # both device verifier heads
    assert ver.verify_many([proof], gpu=gpu, device_head=True) == [True], ver.reasons
    assert lc.proof_public_inputs(proof, 21).tolist() == pis.tolist() == circuit.commit(xs)[2].tolist()
    pr.close(); ver.close()


def test_two_copies_under_the_zero_knowledge_config(pkg, gpu, orc, L):
    c = L.LeafCircuit(copies=2, config=reduced_zk_config(pkg))
    assert c.zero_knowledge and c.blinding_cells.size > 0 and c.target_map.size == 2 * 299
    zk_parity(pkg, gpu, orc, L, c, [lc.real_inputs(L, depth=3), lc.dummy_inputs(L)])


def test_two_copies_under_the_poseidon2_proof_hasher(pkg, orc, L):
    qp = pkg.poseidon2_qp_params()
    pkg.set_hasher_poseidon2(*qp); orc.select_poseidon2(*qp)
    try:
        c = L.LeafCircuit(copies=2, inner_hasher=1)
        xs = [lc.test_inputs(L, 1), lc.real_inputs(L, depth=7, seed=5)]
        g2 = pkg.QpGpu(0)
        pr = L.LeafProver(pkg, g2, c)
        proof, pis = pr.prove(xs)
        cells, values, _ = c.commit(xs)
        rc, wires, _ = orc.generate_witness(c.pack, cells, values, pis)
        assert rc == orc.WIT_OK and np.array_equal(pr.witness(), wires)
        oc = ob.OracleCircuit(orc, c.pack)
        assert proof == oc.prove(wires, pis) and oc.verify(proof) == 0
        oc.close(); pr.close(); g2.close()
    finally:
        pkg.set_hasher_poseidon(); orc.select_poseidon()
