"""The batch layers under a caller's CircuitConfig on the device (tests/test_wrapper_config.py builds the same circuits on the CPU):
fake-leaf proofs made by the device prover, the wrapper's witness by stage s1 (blinding wires drawn on the device), the proof by
stages s2..s12, accepted by the host verifier; public inputs equal to the host restatement's; a flipped byte of an inner proof is
QPGPU_EUNSAT. For the narrowest config and the 143-wire one the proof bytes equal the CPU oracle's of the same witness and seed."""
import numpy as np
import pytest

import oracle_binding as ob
from test_batch_circuits_fake_leaf import EXITS, leaf_pis
from test_wrapper_config import N, NONE, PRE, ROWS, fake_leaf

pytestmark = pytest.mark.gpu

CONFIGS = {
    "default": dict(),
    "routed54": dict(num_routed_wires=54),
    "routed37": dict(num_routed_wires=37),
    "wires143": dict(num_wires=143, num_routed_wires=54),
    "rate4": dict(rate_bits=4, num_query_rounds=21, cap_height=2),
    "challenges3": dict(num_challenges=3, cap_height=0, zero_knowledge=0),
}
ORACLE_BYTES = ("routed37", "wires143")
SEEDS = bytes(range(32))


class Inner:
    """A fake-leaf circuit on the device: proofs of any 21 public inputs."""

    def __init__(self, pkg, gpu, config=None):
        L = pkg.leaf
        self.fake = fake_leaf(pkg) if config is None else L.LeafCircuit(fragment=L.FRAGMENT_FAKE_LEAF, config=config)
        self.circ = pkg.Circuit(gpu, self.fake.pack)
        self.ver = pkg.Verifier(self.fake.pack, circuit=self.circ)
        self.d = gpu.alloc(8 * (int(self.fake.pack[2]) << self.fake.info["degree_bits"]))

    def prove(self, pis):
        self.circ.generate_witness_partial_dev(NONE, NONE, pis, self.d)
        return self.circ.prove_dev(self.d, pis)

    def close(self):
        self.d.free(scrub=True); self.ver.close(); self.circ.close()


@pytest.fixture(scope="module")
def inner(pkg, gpu):
    x = Inner(pkg, gpu)
    proofs = [x.prove(r) for r in ROWS]
    assert all(x.ver.verify(p) for p in proofs)
    yield x, proofs
    x.close()


def prove_wrapper(pkg, gpu, w, wc, d, proofs, pre=PRE, **commit_args):
    """device witness generation (blinding seed set) and proof of one wrapper: (status, public inputs, proof)"""
    com = w.commit(proofs, preimages=pre, device_blinding=True, derive_public_inputs=True, **commit_args)
    st = pkg.recursion.generate_wrapper_witnesses(wc, w, [com], d, SEEDS)
    if st != [0]:
        return st, None, None
    pis = wc.witness_public_inputs_dev(d)[0]
    wc.set_blinding_seed(5)
    return st, pis, wc.prove_dev(d, pis)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_private_batch_under_config(pkg, gpu, orc, inner, name):
    x, proofs = inner
    cfg = pkg.circuit_config("private_batch", **CONFIGS[name])
    assert pkg.validate_circuit_config(cfg) is None
    w = pkg.recursion.WrapperCircuit(x.fake.pack, x.ver, N, logic="private_batch", verify=True, config=cfg)
    h = pkg.pack_header(w.pack)
    assert all(h[k] == int(getattr(cfg, k)) for k in ("num_wires", "num_routed_wires", "num_challenges", "rate_bits", "cap_height", "num_query_rounds", "zero_knowledge"))
    assert (w.blinding_cells.size > 0) == bool(cfg.zero_knowledge)
    wc = pkg.Circuit(gpu, w.pack)
    wc.set_witness_check(True)
    nw, n = w.num_wires, 1 << w.info["degree_bits"]
    d = gpu.alloc(8 * nw * n)
    ver = pkg.Verifier(w.pack, circuit=wc)
    try:
        st, pis, proof = prove_wrapper(pkg, gpu, w, wc, d, proofs)
        assert st == [0], gpu.last_error()
        assert ver.verify(proof), ver.reason
        assert pis.tolist() == pkg.aggregation.private_batch_outputs(np.stack(ROWS), PRE).tolist()
        assert np.frombuffer(proof[-8 * pis.size:], dtype=np.uint64).tolist() == pis.tolist()
        if name in ORACLE_BYTES:
            wires = d.download().reshape(nw, n)
            oc = ob.OracleCircuit(orc, w.pack)
            assert proof == oc.prove(wires, pis, seed=5) and oc.verify(proof) == 0
            oc.close()
        bad = bytearray(proofs[1]); bad[len(bad) // 2] ^= 1
        st, _, _ = prove_wrapper(pkg, gpu, w, wc, d, [proofs[0], bytes(bad)])
        assert st == [-4] and "set twice with different values" in gpu.last_error()
    finally:
        ver.close(); wc.close(); d.free(scrub=True)


def test_non_default_inner_in_a_default_private_batch(pkg, gpu, orc):
    """Nothing of the wrapper assumes the inner proof's 2 challenges, cap 4, 28 queries, 135 wires or 80 routed wires: the inner side is
    read from the inner pack."""
    cfg = pkg.circuit_config("leaf", rate_bits=4, cap_height=2, num_query_rounds=21, num_challenges=3, num_wires=143, num_routed_wires=54,
                             reduction_arity_bits=3, reduction_final_poly_bits=2)
    x = Inner(pkg, gpu, config=cfg)
    h = pkg.pack_header(x.fake.pack)
    assert (h["num_wires"], h["num_routed_wires"], h["num_challenges"], h["num_query_rounds"], h["cap_height"], h["rate_bits"]) == (143, 54, 3, 21, 2, 4)
    assert [int(a) for a in x.fake.pack[18:18 + h["num_arity_rounds"]]] == [3]
    proofs = [x.prove(r) for r in ROWS]
    assert all(x.ver.verify(p) for p in proofs), x.ver.reason
    w = pkg.recursion.WrapperCircuit(x.fake.pack, x.ver, N, logic="private_batch", verify=True, config="private_batch")
    assert w.Q == 21
    wc = pkg.Circuit(gpu, w.pack)
    wc.set_witness_check(True)
    d = gpu.alloc(8 * (w.num_wires << w.info["degree_bits"]))
    ver = pkg.Verifier(w.pack, circuit=wc)
    try:
        st, pis, proof = prove_wrapper(pkg, gpu, w, wc, d, proofs)
        assert st == [0], gpu.last_error()
        assert ver.verify(proof), ver.reason
        assert pis.tolist() == pkg.aggregation.private_batch_outputs(np.stack(ROWS), PRE).tolist()
        bad = bytearray(proofs[0]); bad[len(bad) // 2] ^= 1
        assert prove_wrapper(pkg, gpu, w, wc, d, [bytes(bad), proofs[1]])[0] == [-4]
    finally:
        ver.close(); wc.close(); d.free(scrub=True); x.close()


def test_chain_under_non_default_configs_at_both_levels(pkg, gpu, inner):
    """Two private batches (zero knowledge, 54 routed wires) under one public batch (54 routed of 138 wires, rate 4): the root is
    accepted on the host and by the device verifier, its public inputs are the host restatement's."""
    x, proofs = inner
    A = pkg.aggregation
    rows2 = [leaf_pis(103, out=(30, 0), exits=(EXITS[2], (0, 0, 0, 0))), leaf_pis(104, out=(1, 2), exits=(EXITS[3], EXITS[1]))]
    batches = [(ROWS, proofs), (rows2, [x.prove(r) for r in rows2])]
    w1 = pkg.recursion.WrapperCircuit(x.fake.pack, x.ver, N, logic="private_batch", verify=True, config=pkg.circuit_config("private_batch", num_routed_wires=54))
    c1 = pkg.Circuit(gpu, w1.pack)
    v1 = pkg.Verifier(w1.pack, circuit=c1)
    d1 = gpu.alloc(8 * (w1.num_wires << w1.info["degree_bits"]))
    level1 = []
    for b, (rows, ps) in enumerate(batches):
        st, pis, proof = prove_wrapper(pkg, gpu, w1, c1, d1, ps, pre=PRE + 10 * b)
        assert st == [0], gpu.last_error()
        assert pis.tolist() == A.private_batch_outputs(np.stack(rows), PRE + 10 * b).tolist() and v1.verify(proof), v1.reason
        level1.append((pis, proof))
    w2 = pkg.recursion.WrapperCircuit(w1.pack, v1, 2, logic="public_batch", verify=True, config=pkg.circuit_config("public_batch", num_routed_wires=54, num_wires=138, rate_bits=4))
    assert (w2.num_wires, pkg.pack_header(w2.pack)["rate_bits"]) == (138, 4)
    c2 = pkg.Circuit(gpu, w2.pack)
    v2 = pkg.Verifier(w2.pack, circuit=c2)
    d2 = gpu.alloc(8 * (w2.num_wires << w2.info["degree_bits"]))
    addr = bytes([5] * 32)
    try:
        st, pis, root = prove_wrapper(pkg, gpu, w2, c2, d2, [p for _, p in level1], pre=None, aggregator_address=addr)
        assert st == [0], gpu.last_error()
        assert v2.verify(root), v2.reason
        assert v2.verify_many([root], gpu=gpu) == [True], v2.reasons
        assert pis.tolist() == A.public_batch_outputs(np.stack([p for p, _ in level1]), N, addr).tolist()
        bad = bytearray(level1[1][1]); bad[len(bad) // 2] ^= 1
        assert prove_wrapper(pkg, gpu, w2, c2, d2, [level1[0][1], bytes(bad)], pre=None, aggregator_address=addr)[0] == [-4]
    finally:
        for o in (v2, c2, v1, c1):
            o.close()
        d1.free(scrub=True); d2.free(scrub=True)


def test_provers_take_a_config(pkg, gpu):
    """PrivateBatchProver::new(agg_circuit_config, ..) / PublicBatchProver::new(public_batch_circuit_config, ..): one batch through
    new / commit / prove at both levels under configs other than the canonical ones."""
    import leaf_cases as lc
    L, R, A = pkg.leaf, pkg.recursion, pkg.aggregation
    leaf = L.LeafCircuit()
    priv = R.PrivateBatchProver(pkg, gpu, leaf, 2, config=pkg.circuit_config("private_batch", num_routed_wires=54, num_wires=138))
    pub = None
    try:
        assert (priv.circuit.num_wires, pkg.pack_header(priv.circuit.pack)["num_routed_wires"], priv.circuit.zero_knowledge) == (138, 54, True)
        leaf_proof = priv.leaf_prover.prove(lc.real_inputs(L, depth=3, seed=6))[0]
        pb = priv.commit([leaf_proof], seed=bytes([3] * 32)).prove()
        assert priv.verifier.verify(pb), priv.verifier.reason
        src, pre = priv.arrangement
        rows = np.stack([A.proof_public_inputs(leaf_proof if k != 0xFFFFFFFF else priv.dummy_leaf_proof, 21) for k in src.tolist()])
        assert A.proof_public_inputs(pb, 50).tolist() == A.private_batch_outputs(rows, pre).tolist()
        pub = R.PublicBatchProver(pkg, gpu, priv, 2, config=pkg.circuit_config("public_batch", num_routed_wires=60, cap_height=3))
        assert pkg.pack_header(pub.circuit.pack)["cap_height"] == 3
        addr = bytes([9] * 32)
        root = pub.commit([pb], aggregator_address=addr).prove()
        assert pub.verifier.verify(root), pub.verifier.reason
        got = A.proof_public_inputs(root, A.public_batch_pi_len(2, 2))
        dummy = A.proof_public_inputs(pub.dummy_private_batch_proof, 50)
        assert got.tolist() == A.public_batch_outputs(np.stack([A.proof_public_inputs(pb, 50), dummy]), 2, addr).tolist()
    finally:
        if pub is not None:
            pub.close()
        priv.close()
