"""Proofs at rate_bits above 3, end to end: circuits whose first commitment or whose folded FRI layers are LDEs the pruned full-size
transform plan cannot take (a polynomial shorter than one pass-1 row; more than 2^20 points from less than 1/8 of them) and that
the coset decomposition now carries (csrc/ntt_plan.cpp lde_coset_run). Bytes against the CPU oracle at the small sizes, the host
and device verifiers everywhere, a one-bit tamper rejected by all three.

Before the decomposition qpgpu_circuit_load refused the first seven rows of ROWS (a layer or the first commitment "shorter than one
pass-1 row"), the two large circuits and the 2^13-row leaf at rate 8 ("an LDE beyond 2^20 points needs rate_bits <= 3")."""
import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_batch_gpu import _witnesses
from test_stage_plan_gpu import Flow

pytestmark = pytest.mark.gpu

# degree_bits, rate_bits, cap_height, arity_bits; the last row is a control that loaded before
ROWS = [(8, 8, 4, [2, 2]), (9, 7, 4, [4, 1]), (7, 8, 4, [1, 2, 1]), (8, 8, 0, [4, 3]), (6, 8, 4, [3]), (5, 7, 4, [2]), (4, 8, 4, [1, 1]),
        (6, 5, 4, [3])]
IDS = ["d%d-r%d-cap%d-%s" % (d, r, c, "".join(map(str, a))) for d, r, c, a in ROWS]
NARROW = dict(num_wires=24, num_routed=16, num_public_inputs=3)


def narrow_case(pkg, d, r, cap, arity, seed, **kw):
    pack, wires, pis = pkg.synth_circuit(d, seed=seed, **(kw or NARROW))
    return fs.with_schedule(pack, arity, rate_bits=r, cap_height=cap, num_queries=6, pow_bits=4), wires, pis


def flipped(proof, at):
    bad = bytearray(proof); bad[at] ^= 1
    return bytes(bad)


def assert_verifiers(gpu, ver, proofs, tamper_at=None):
    """Accepted by qpgpu_verifier_verify and by qpgpu_verifier_verify_many_device with the head on the host and on the device;
    the first proof with one bit flipped is rejected by all three."""
    for p in proofs:
        assert ver.verify(p), ver.reason
    assert ver.verify_many(proofs, gpu=gpu) == [True] * len(proofs), ver.reasons
    assert ver.verify_many(proofs, gpu=gpu, device_head=True) == [True] * len(proofs), ver.reasons
    bad = flipped(proofs[0], len(proofs[0]) // 2 if tamper_at is None else tamper_at)
    assert not ver.verify(bad)
    reason = ver.reason
    assert ver.verify_many([bad], gpu=gpu) == [False]
    assert ver.verify_many([bad], gpu=gpu, device_head=True) == [False]
    return reason


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_proof_bytes_equal_the_oracle(pkg, gpu, orc, row):
    d, r, cap, arity = row
    pack, wires, pis = narrow_case(pkg, d, r, cap, arity, seed=800 + ROWS.index(row))
    h = pkg.pack_header(pack)
    assert (h["degree_bits"], h["rate_bits"], h["cap_height"], h["num_query_rounds"], h["proof_of_work_bits"]) == (d, r, cap, 6, 4)
    oc = OracleCircuit(orc, pack); circ = pkg.Circuit(gpu, pack)
    ver = pkg.Verifier(pack, circuit=circ)
    try:
        want = oc.prove(wires, pis)
        got = circ.prove(wires, pis)
        assert len(got) == len(want) == circ.proof_size()
        assert got == want, "proof bytes differ from the oracle at byte %d" % next(i for i in range(len(got)) if got[i] != want[i])
        assert oc.verify(got) == 0
        d_w = gpu.to_device(wires)
        try:
            assert circ.prove_dev(d_w, pis) == want
        finally:
            d_w.free()
        assert_verifiers(gpu, ver, [got])
    finally:
        ver.close(); circ.close(); oc.close()


def test_lockstep_batch_of_three(pkg, gpu, orc):
    """(7, 8) with [1, 2, 1]: three witnesses through qpgpu_prove_batch_dev; the folded layers' LDEs (2^6, 2^4 and 2^3 coefficients
    at rate 8) carry the proofs as strides of the FRI workspace."""
    pack, wires, _ = narrow_case(pkg, 7, 8, 4, [1, 2, 1], seed=830, poseidon=True, base_sum=True)
    pis, ws = _witnesses(pkg, gpu, pack, wires, 3)
    circ = pkg.Circuit(gpu, pack, max_batch=3); oc = OracleCircuit(orc, pack)
    ver = pkg.Verifier(pack, circuit=circ)
    bufs = [gpu.to_device(w) for w in ws]
    try:
        got = circ.prove_batch_dev(bufs, pis)
        assert len(set(got)) == 3
        for b in range(3):
            assert got[b] == oc.prove(ws[b], pis[b]), b
        assert_verifiers(gpu, ver, got)
    finally:
        for x in bufs:
            x.free()
        ver.close(); circ.close(); oc.close()


def test_stage_flow_gives_the_same_bytes(pkg, gpu, orc):
    """(8, 8) with [2, 2] through qpgpu_oracle_commit -> stage plan -> qpgpu_fri_prove: the bytes of qpgpu_prove_dev."""
    pack, wires, pis = narrow_case(pkg, 8, 8, 4, [2, 2], seed=840)
    circ = pkg.Circuit(gpu, pack)
    d_w = gpu.to_device(wires)
    try:
        want = circ.prove_dev(d_w, pis)
    finally:
        d_w.free(); circ.close()
    fl = Flow(pkg, gpu, orc, pack)
    try:
        got = fl.prove(wires, pis)[0]
    finally:
        fl.close()
    assert got == want


def test_zero_knowledge_with_a_seeded_blinding(pkg, gpu, orc):
    """(6, 8) with [3] and salted oracles: the oracle takes the same seed, so the bytes are equal; the host verifier accepts."""
    pack, wires, pis = narrow_case(pkg, 6, 8, 4, [3], seed=850)
    pack[14] = 1
    oc = OracleCircuit(orc, pack); circ = pkg.Circuit(gpu, pack)
    ver = pkg.Verifier(pack, circuit=circ)
    try:
        circ.set_blinding_seed(0xBEEF)
        got = circ.prove(wires, pis)
        assert got == oc.prove(wires, pis, seed=0xBEEF)
        assert oc.verify(got) == 0
        assert_verifiers(gpu, ver, [got])
    finally:
        ver.close(); circ.close(); oc.close()


def wires_row_offset(pkg, pack):
    """Byte of the first query's opened wires row: caps and openings, the FRI round caps, then the constants/sigmas row with its
    sibling count and path."""
    h = pkg.pack_header(pack)
    nch = h["num_challenges"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    n_open = ncs + h["num_wires"] + 2 * nch + nch * h["num_partial_products"] + nch * h["quotient_degree_factor"]
    capw = 4 << h["cap_height"]
    plen = h["degree_bits"] + h["rate_bits"] - h["cap_height"]
    return 8 * (3 * capw + 2 * n_open) + h["num_arity_rounds"] * 8 * capw + 8 * ncs + 1 + 32 * plen


@pytest.mark.parametrize("d,r", [(13, 8), (16, 5)])
def test_large_sizes_on_the_device(pkg, gpu, d, r):
    """2^21 leaves, on the device only (the oracle would take minutes over the Merkle trees): the 24-wire circuit proves; the host
    verifier (constants/sigmas cap from the loaded circuit) and the device verifier accept; a bit flipped in an opened wires row
    fails that query's Merkle check."""
    arity = fs.constant_arity(d, r, 4, 4, 5)
    pack, wires, pis = narrow_case(pkg, d, r, 4, arity, seed=860 + d)
    circ = pkg.Circuit(gpu, pack)
    ver = pkg.Verifier(pack, circuit=circ)
    try:
        d_w = gpu.to_device(wires)
        try:
            proof = circ.prove_dev(d_w, pis)
        finally:
            d_w.free()
        reason = assert_verifiers(gpu, ver, [proof], tamper_at=wires_row_offset(pkg, pack) + 8 * 5)
        assert "Merkle path of initial oracle 1" in reason, reason
    finally:
        ver.close(); circ.close()


def test_leaf_at_its_own_size(pkg, gpu, orc):
    """The leaf circuit (2^8 rows) at rate 8 with arity 4 and a 4-coefficient final polynomial: layers of 2^6 and 2^4 coefficients.
    Dummy inputs and one real spend, bytes against the oracle."""
    L = pkg.leaf
    c = L.LeafCircuit(config=pkg.circuit_config("leaf", rate_bits=8, reduction_arity_bits=2, reduction_final_poly_bits=2))
    h = pkg.pack_header(c.pack)
    assert (h["degree_bits"], h["rate_bits"]) == (8, 8)
    assert [int(x) for x in c.pack[18:18 + h["num_arity_rounds"]]] == [2, 2, 2]
    pr = L.LeafProver(pkg, gpu, c)
    ver = pkg.Verifier(c.pack, circuit=pr.circ)
    oc = OracleCircuit(orc, c.pack)
    try:
        proofs = []
        for x in (lc.dummy_inputs(L), lc.real_inputs(L, depth=3)):
            cells, values, pis = c.commit(x)
            rc, wires, _ = orc.generate_witness(c.pack, cells, values, pis)
            assert rc == orc.WIT_OK
            proof, _ = pr.prove(x)
            assert np.array_equal(pr.witness(), wires)
            assert proof == oc.prove(wires, pis)
            assert oc.verify(proof) == 0
            proofs.append(proof)
        assert_verifiers(gpu, ver, proofs)
    finally:
        oc.close(); pr.close(); ver.close()


def test_leaf_at_bench_size_and_rate_8(pkg, gpu):
    """LeafCircuit(min_degree_bits=13) at rate 8: 2^21-point oracles. It loads and proves the dummy inputs; the host and device
    verifiers accept. No oracle at this size."""
    L = pkg.leaf
    c = L.LeafCircuit(min_degree_bits=13, config=pkg.circuit_config("leaf", rate_bits=8))
    h = pkg.pack_header(c.pack)
    assert (h["degree_bits"], h["rate_bits"]) == (13, 8)
    pr = L.LeafProver(pkg, gpu, c)
    ver = pkg.Verifier(c.pack, circuit=pr.circ)
    try:
        proof, pis = pr.prove(lc.dummy_inputs(L))
        assert lc.proof_public_inputs(proof, 21).tolist() == pis.tolist()
        assert_verifiers(gpu, ver, [proof])
    finally:
        pr.close(); ver.close()
