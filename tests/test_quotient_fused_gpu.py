"""The quotient stage's one-pass kernel (csrc/quotient_kernels.hip: quotient_perm_gates_kernel, the permutation terms and the
Constant / PublicInput / Arithmetic / BaseSum<2> gates in one walk over the routed wires, workgroups placed by csrc/quotient_map.hpp)
against the two kernels it stands in for and against the CPU oracle. Every case proves the same witnesses with the switch off
(qpgpu_circuit_set_quotient_fused(0): quotient_perm_kernel + quotient_gates_kernel) and on, in one process, and compares proof bytes;
the oracle's proof of the same witness must be those bytes too. Exact arithmetic: no tolerance anywhere. Shapes: the leaf circuit at
its own 2^8 rows (8 tiles of quotient points) alone and in lockstep batches of 3 and 9 (fewer and more proofs than XCDs, no multiple
of 8); synthetic circuits with 60 routed wires (the last chunk holds 4) and 80, with hash gates (the kernel leaves running sums)
and without (it stores the finished quotient), down to 2^5 and 2^6 rows (1 and 2 tiles: the padded last group of the workgroup
map); the zero-knowledge leaf; the recursion gate set, where the launcher must keep the two kernels; the witness check, which
runs the gate kernels on the trace rows. The workgroup map itself is tests/test_quotient_map_host.py."""
import numpy as np
import pytest

import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_leaf_circuit_gpu import oracle_side
from test_leaf_config import reduced_zk_config
from test_leaf_config_gpu import SEED, blind_of
from test_leaf_config_gpu import oracle_side as zk_oracle_side
from test_quotient_fold_gpu import batch_witnesses, prove_batch

pytestmark = pytest.mark.gpu
HASH = dict(poseidon=True, poseidon2=True)


def off_and_on(circ, run):
    """run() with the switch off, then on: the two results, and what the info call said the stage would run each time."""
    out, sel = [], []
    for on in (False, True):
        circ.set_quotient_fused(on)
        sel.append(circ.quotient_info())
        out.append(run())
    return out, sel


@pytest.fixture(scope="module")
def leaf(pkg):
    return pkg.leaf.LeafCircuit(min_degree_bits=8)


@pytest.fixture(scope="module")
def leaf_inputs(pkg):
    L = pkg.leaf
    return [lc.dummy_inputs(L), lc.test_inputs(L, 0), lc.test_inputs(L, 1)] + [lc.real_inputs(L, depth=1 + k, seed=20 + k) for k in range(6)]


@pytest.fixture(scope="module")
def leaf_oracle_proofs(orc, leaf, leaf_inputs):
    """The oracle's proof of each of the nine inputs, made once and left alone."""
    return [oracle_side(orc, leaf, x)[1] for x in leaf_inputs]


@pytest.mark.parametrize("nb", [1, 3, 9])
def test_leaf_circuit_batches(pkg, gpu, leaf, leaf_inputs, leaf_oracle_proofs, nb):
    assert pkg.pack_header(leaf.pack)["degree_bits"] == 8
    com = [leaf.commit(x) for x in leaf_inputs[:nb]]
    circ = pkg.Circuit(gpu, leaf.pack, max_batch=nb)
    nw, n = 135, 1 << 8
    d = gpu.alloc(nb * nw * n * 8)
    try:
        circ.witness_partial_prepare(com[0][0], nb)
        assert circ.generate_witness_partial_batch_dev(com[0][0], np.stack([c[1] for c in com]), np.stack([c[2] for c in com]), d) == [0] * nb
        ptrs, pis = [d.ptr + k * nw * n * 8 for k in range(nb)], [c[2] for c in com]
        (off, on), sel = off_and_on(circ, lambda: circ.prove_batch_dev(ptrs, pis) if nb > 1 else [circ.prove_dev(ptrs[0], pis[0])])
        assert sel == [(False, False), (True, True)]
        assert on == off == leaf_oracle_proofs[:nb]
        assert len(set(on)) == nb
    finally:
        d.free(scrub=True); circ.close()


@pytest.mark.parametrize("d,num_routed,hash_gates,nb", [(8, 60, True, 1), (8, 80, True, 3), (8, 60, False, 3), (8, 80, False, 1),
                                                        (5, 80, False, 3), (6, 60, True, 9)])
def test_synthetic_circuits(pkg, gpu, orc, d, num_routed, hash_gates, nb):
    pack, wires, pis = pkg.synth_circuit(d, num_routed=num_routed, seed=30 + d + num_routed, base_sum=True, **(HASH if hash_gates else {}))
    circ = pkg.Circuit(gpu, pack, max_batch=nb); oc = OracleCircuit(orc, pack)
    try:
        ws, ps = batch_witnesses(circ, wires, pis, nb)
        (off, on), sel = off_and_on(circ, lambda: prove_batch(gpu, circ, ws, ps))
        assert sel == [(False, False), (True, True)]
        want = [oc.prove(w, p) for w, p in zip(ws, ps)]
        assert on == off == want and len(set(want)) == nb
        assert oc.verify(on[-1]) == 0
    finally:
        circ.close(); oc.close()


def test_zero_knowledge_leaf(pkg, gpu, orc):
    """The leaf under the private-batch (zero-knowledge) config at the fewest query rounds it admits, salts and blinding draw seeded."""
    L = pkg.leaf
    zk = L.LeafCircuit(config=reduced_zk_config(pkg))
    assert pkg.pack_header(zk.pack)["zero_knowledge"] == 1 and pkg.pack_header(zk.pack)["num_routed_wires"] == 60
    pr = L.LeafProver(pkg, gpu, zk, blinding_seed=SEED)
    try:
        x = lc.real_inputs(L, depth=3)
        (off, on), sel = off_and_on(pr.circ, lambda: pr.prove(x)[0])
        assert sel == [(False, False), (True, True)]
        assert on == off == zk_oracle_side(orc, zk, x, blind_of(zk, pr.witness()), SEED)[1]
    finally:
        pr.close()


def test_recursion_gate_set_keeps_the_two_kernels(pkg, gpu, orc):
    pack, wires, pis = pkg.synth_circuit(8, seed=44, base_sum=True, recursion=True, **HASH)
    circ = pkg.Circuit(gpu, pack); oc = OracleCircuit(orc, pack)
    try:
        (off, on), sel = off_and_on(circ, lambda: circ.prove(wires, pis))
        assert sel == [(False, False), (True, False)]          # switched on, not selected
        assert on == off == oc.prove(wires, pis)
    finally:
        circ.close(); oc.close()


def test_witness_check_alongside(pkg, gpu, leaf, leaf_inputs, leaf_oracle_proofs):
    """The witness check runs the gate kernels on the trace rows (no permutation terms): it passes a good witness and names a bad
    one's row, with the quotient itself from the one-pass kernel."""
    pr = pkg.leaf.LeafProver(pkg, gpu, leaf, witness_check=True)
    try:
        assert pr.circ.quotient_info() == (True, True)
        proof, pis = pr.prove(leaf_inputs[3])
        assert proof == leaf_oracle_proofs[3]
        w = pr.witness().copy()
        cell = int(leaf.target_map[237])                       # asset_id
        w[cell % 135, cell // 135] ^= 1
        with pytest.raises(pkg.QpGpuError) as e:
            pr.circ.prove(w, pis)
        assert e.value.code == -4
    finally:
        pr.close()


def test_environment_default(pkg, gpu, leaf, monkeypatch):
    for env, want in (("0", (False, False)), ("1", (True, True)), (None, (True, True))):
        if env is None:
            monkeypatch.delenv("QPGPU_QUOTIENT_FUSED", raising=False)
        else:
            monkeypatch.setenv("QPGPU_QUOTIENT_FUSED", env)
        circ = pkg.Circuit(gpu, leaf.pack)
        try:
            assert circ.quotient_info() == want
        finally:
            circ.close()
