"""The leaf circuit under other CircuitConfigs on the device (WormholeProver::new(config), wormhole/prover/src/lib.rs:137-149): the
zero-knowledge leaf of the reference's prover_create_proof_zk bench target — stage s1 draws CircuitBuilder::blind's random wires on the
device, stages s2..s12 salt the three blinded oracles — at a reduced query count against the oracle (witness cell for cell, proof
byte for byte under a seeded blinding stream) and at the canonical 28 queries (2^14 rows, 541 050 drawn cells) against the
verifiers; the non-zero-knowledge knobs (rate, cap height, query rounds, proof of work) against the oracle at the leaf's own size."""
import os
import subprocess

import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
import oracle_binding as ob
from test_leaf_config import blind_counts, reduced_zk_config

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def zk(pkg, L):
    """The full leaf under the zero-knowledge config with the fewest query rounds the config policy admits."""
    return L.LeafCircuit(config=reduced_zk_config(pkg))


def oracle_side(orc, circuit, x, blind_values, seed):
    """generate_partial_witness over commit's assignments with the blinding cells as ordinary assignments, then the seeded proof."""
    cells, values, pis = circuit.commit(x, device_blinding=True)
    rc, wires, _ = orc.generate_witness(circuit.pack, cells, np.concatenate([values, blind_values]), pis)
    assert rc == orc.WIT_OK
    oc = ob.OracleCircuit(orc, circuit.pack)
    proof = oc.prove(wires, pis, seed=seed)
    assert oc.verify(proof) == 0
    oc.close()
    return wires, proof


def blind_of(circuit, wires):
    b = circuit.blinding_cells
    return wires[(b % np.uint64(135)).astype(np.int64), (b // np.uint64(135)).astype(np.int64)]


def parity(pkg, gpu, orc, L, circuit, hasher=0):
    pr = L.LeafProver(pkg, gpu, circuit, blinding_seed=SEED)
    ver = pkg.Verifier(circuit.pack, circuit=pr.circ, hasher=hasher)
    nb = circuit.blinding_cells.size
    drawn = []
    for name, x in (("dummy inputs", lc.dummy_inputs(L)), ("spend, depth 3", lc.real_inputs(L, depth=3))):
        proof, pis = pr.prove(x)
        got = pr.witness()
        blind = blind_of(circuit, got)
        assert int(blind.max()) < pkg.P and np.unique(blind).size == nb, name              # fresh draws from 2^64: no repeats
        want_wires, want_proof = oracle_side(orc, circuit, x, blind, SEED)
        assert np.array_equal(got, want_wires), name
        assert proof == want_proof, name
        assert ver.verify(proof), (name, ver.reason)
        assert lc.proof_public_inputs(proof, 21).tolist() == pis.tolist()
        drawn.append(blind)
    assert np.array_equal(drawn[0], drawn[1])                   # one seed, one stream: the draw does not depend on the inputs
    pr.close(); ver.close()


def test_parity_under_a_seeded_blinding_stream(pkg, gpu, orc, L, zk):
    h = pkg.pack_header(zk.pack)
    k, regular, zs = blind_counts(zk.info["rows_before_padding"], zk.config)
    assert h["zero_knowledge"] == 1 and zk.blinding_cells.size == regular * 135 + zs * 60
    parity(pkg, gpu, orc, L, zk)


def test_parity_under_the_poseidon2_hasher(pkg, orc, L):
    qp = pkg.poseidon2_qp_params()
    pkg.set_hasher_poseidon2(*qp); orc.select_poseidon2(*qp)
    try:
        c = L.LeafCircuit(inner_hasher=1, config=reduced_zk_config(pkg))
        g2 = pkg.QpGpu(0)
        parity(pkg, g2, orc, L, c, hasher=1)
        g2.close()
    finally:
        pkg.set_hasher_poseidon(); orc.select_poseidon()


def test_hash_hints_give_the_same_proof_in_fewer_levels(pkg, gpu, L, zk):
    plain = L.LeafProver(pkg, gpu, zk, blinding_seed=SEED)
    hinted = L.LeafProver(pkg, gpu, zk, hash_hints=True, blinding_seed=SEED)
    for x in (lc.dummy_inputs(L), lc.real_inputs(L, depth=3)):
        p0, pis0 = plain.prove(x)
        p1, pis1 = hinted.prove(x)
        assert np.array_equal(plain.witness(), hinted.witness()) and p0 == p1 and pis0.tolist() == pis1.tolist()
    l0, l1 = plain.circ.witness_info()[1], hinted.circ.witness_info()[1]
    assert l1 < l0, (l0, l1)
    # inputs the circuit does not satisfy stay unsatisfiable, with and without hints
    y = lc.real_inputs(L, depth=3); y.secret[3] ^= 1
    for pr in (plain, hinted):
        with pytest.raises(pkg.QpGpuError) as e:
            pr.prove(y)
        assert e.value.code == -4 and "set twice with different values" in str(e.value)
    plain.close(); hinted.close()


def test_canonical_zero_knowledge_config(pkg, gpu, L):
    """wormhole_private_batch_circuit_config(): 28 queries, 2^14 rows, 2 774 regular blinding rows and 2 776 pairs."""
    c = L.LeafCircuit(config="private_batch")
    assert c.info["degree_bits"] == 14 and c.blinding_cells.size == 2774 * 135 + 2776 * 60
    pr = L.LeafProver(pkg, gpu, c)
    ver = pkg.Verifier(c.pack, circuit=pr.circ)
    x = lc.dummy_inputs(L)
    p0, pis0 = pr.prove(x)
    w0 = blind_of(c, pr.witness())
    p1, pis1 = pr.prove(x)
    assert np.unique(w0).size == w0.size and not np.array_equal(w0, blind_of(c, pr.witness()))
    assert len(p0) == len(p1) and p0 != p1 and pis0.tolist() == pis1.tolist() == lc.proof_public_inputs(p1, 21).tolist()
    assert ver.verify(p0) and ver.verify(p1), ver.reason
    assert ver.verify_many([p0, p1], gpu=gpu) == [True, True], ver.reasons
    assert ver.verify_many([p0, p1], gpu=gpu, device_head=True) == [True, True], ver.reasons
    bad = bytearray(p0); bad[len(bad) // 2] ^= 1
    assert not ver.verify(bytes(bad)) and ver.verify_many([bytes(bad)], gpu=gpu, device_head=True) == [False]
    pr.close(); ver.close()


def test_lockstep_pool_fails_the_bad_ticket_alone(pkg, gpu, L, zk):
    pr = L.LeafProver(pkg, gpu, zk, hash_hints=True)
    ver = pkg.Verifier(zk.pack, circuit=pr.circ)
    xs = [lc.dummy_inputs(L), lc.real_inputs(L, depth=3), lc.test_inputs(L, 0), lc.real_inputs(L, depth=7, seed=5), lc.test_inputs(L, 1),
          lc.real_inputs(L, depth=1, seed=2), lc.dummy_inputs(L)]
    bad = lc.real_inputs(L, depth=3); bad.secret[5] ^= 1                # a nullifier secret the nullifier was not made from
    xs.insert(5, bad)
    pool = pr.pool(workers=2, max_batch=4)
    tickets = [pr.submit(pool, x) for x in xs]
    proofs = []
    for k, t in enumerate(tickets):
        if k == 5:
            with pytest.raises(pkg.QpGpuError) as e:
                pool.wait(t)
            assert e.value.code == -4 and "set twice with different values" in str(e.value)
        else:
            proofs.append(pool.wait(t))
    pool.close()
    assert len(proofs) == 7 and len(set(proofs)) == 7
    assert ver.verify_many(proofs) == [True] * 7, ver.reason
    good = [x for k, x in enumerate(xs) if k != 5]
    for p, x in zip(proofs, good):
        assert lc.proof_public_inputs(p, 21).tolist() == zk.commit(x)[2].tolist()
    pr.close(); ver.close()


@pytest.mark.parametrize("knobs", [dict(rate_bits=4), dict(cap_height=2, num_query_rounds=10), dict(proof_of_work_bits=8),
                                   dict(reduction_arity_bits=2), dict(reduction_arity_bits=3, reduction_final_poly_bits=2),
                                   dict(reduction_arity_bits=1, reduction_final_poly_bits=0, cap_height=2)], ids=lambda k: "-".join("%s=%d" % kv for kv in k.items()))
def test_non_zero_knowledge_knobs_match_the_oracle(pkg, gpu, orc, L, knobs):
    c = L.LeafCircuit(config=pkg.circuit_config("leaf", **knobs))
    h = pkg.pack_header(c.pack)
    assert h["degree_bits"] == 8 and all(h[k] == v for k, v in knobs.items() if k in h)
    cfg = c.config
    arity = [int(x) for x in c.pack[18:18 + h["num_arity_rounds"]]]
    assert arity == fs.constant_arity(8, cfg.rate_bits, cfg.cap_height, cfg.reduction_arity_bits, cfg.reduction_final_poly_bits)
    assert arity == {2: [2, 2], 3: [3, 3], 1: [1] * 8}.get(knobs.get("reduction_arity_bits"), [4])
    pr = L.LeafProver(pkg, gpu, c)
    ver = pkg.Verifier(c.pack, circuit=pr.circ)
    oc = ob.OracleCircuit(orc, c.pack)
    for x in (lc.dummy_inputs(L), lc.real_inputs(L, depth=3)):
        cells, values, pis = c.commit(x)
        rc, wires, _ = orc.generate_witness(c.pack, cells, values, pis)
        assert rc == orc.WIT_OK
        proof, _ = pr.prove(x)
        assert np.array_equal(pr.witness(), wires)
        assert proof == oc.prove(wires, pis)
        assert oc.verify(proof) == 0 and ver.verify(proof), ver.reason
        assert ver.verify_many([proof], gpu=gpu, device_head=True) == [True], ver.reasons
    oc.close(); pr.close(); ver.close()


def test_wrapper_over_a_zero_knowledge_inner_circuit_that_is_no_batch(pkg, gpu, L):
    """The recursive verifier over a zero-knowledge inner circuit other than the private batch: the fake leaf (21 free public inputs)
    under the reduced-query zero-knowledge config, its only assignments the blinding cells; wrapped with the transcript and the
    complete verifier in-circuit, proven on the device."""
    fake = L.LeafCircuit(fragment=L.FRAGMENT_FAKE_LEAF, config=reduced_zk_config(pkg))
    h = pkg.pack_header(fake.pack)
    nb = fake.blinding_cells.size
    assert h["zero_knowledge"] == 1 and nb > 0
    circ = pkg.Circuit(gpu, fake.pack)
    d = gpu.alloc(8 * 135 << h["degree_bits"])
    pis = np.zeros(21, dtype=np.uint64); pis[0], pis[1], pis[3], pis[4:8], pis[20] = 1, 100, 10, (5, 6, 7, 8), 42
    assert circ.generate_witness_partial_batch_blinded_dev(fake.blinding_cells, np.zeros((1, 0), dtype=np.uint64), pis[None], d, nb) == [0]
    inner = circ.prove_dev(d, pis)
    ver = pkg.Verifier(fake.pack, circuit=circ)
    assert ver.verify(inner), ver.reason
    w = pkg.recursion.WrapperCircuit(fake.pack, ver, 1, verify=True)
    cells, vals, wpis = w.commit([inner])
    assert wpis.tolist() == pis.tolist()
    wh = pkg.pack_header(w.pack)
    wc = pkg.Circuit(gpu, w.pack)
    dw = gpu.alloc(8 * 135 << wh["degree_bits"])
    wc.generate_witness_partial_dev(cells, vals, wpis, dw)
    outer = wc.prove_dev(dw, wpis)
    wver = pkg.Verifier(w.pack, circuit=wc)
    assert wver.verify(outer), wver.reason
    # a forged inner proof: one opened wire changed (the openings follow the three caps; constants and sigmas come first)
    off = 3 * (32 << h["cap_height"]) + 16 * (h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]) + 16 * 5
    bad = bytearray(inner); bad[off] ^= 1
    assert not ver.verify(bytes(bad))
    cells, vals, _ = w.commit([bytes(bad)], public_inputs=wpis)
    with pytest.raises(pkg.QpGpuError) as e:
        wc.generate_witness_partial_dev(cells, vals, wpis, dw)
    assert e.value.code == -4
    for x in (wver, ver, wc, circ):
        x.close()
    d.free(scrub=True); dw.free(scrub=True)


def test_c_example_zero_knowledge(pkg, tmp_path):
    """examples/leaf_prove_example.c --zk: the pool's blinded entries from plain C; every proof of the last step is verified there."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "qpgpu_leaf_prove_example_zk")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "leaf_prove_example.c"),
                           "-L", os.path.join(root, "qp-zk-circuits_amd"), "-lqpgpu", "-lpthread",
                           "-Wl,-rpath," + os.path.join(root, "qp-zk-circuits_amd"), "-o", out])
    res = subprocess.run([out, "--zk", "0", "0", "2", "2", "1", "1"], capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stderr + res.stdout
    assert "zero knowledge" in res.stdout and "ok devices=1 workers=2 lockstep=2" in res.stdout and "unsatisfiable job alone" in res.stdout
    assert "verified=4" in res.stdout
