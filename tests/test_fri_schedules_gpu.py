"""Prover byte parity under FRI reduction schedules other than ConstantArityBits(4, 5): every row of fri_schedules.SCHEDULES
through the whole hot path (qpgpu_prove, qpgpu_prove_dev), against the CPU oracle byte for byte; two rows again with the full
gate mix and zero knowledge, two as lockstep batches, one under the Poseidon2 hasher. The arity-generic device code this
reaches: the fold, interleave and leaf-row kernels, the no-hash leaves of arity 2, per-round gathers with a running shift, a
2-coefficient per-round LDE, zero-length Merkle paths and the proof layout that sizes them."""
import numpy as np
import pytest

import fri_schedules as fs
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu

# different witnesses of one circuit come from its public-input cells, a trailer only packs with Poseidon rows carry (135 wires)
WITH_PI_CELLS = dict(poseidon=True, base_sum=True)
FULL_MIX = dict(poseidon=True, base_sum=True, ext_arith=True, recursion=True)


def assert_parity(gpu, circ, oc, wires, pis, seed=None):
    assert circ.proof_size() == oc.proof_size()
    if seed is not None:
        circ.set_blinding_seed(seed)
    got = circ.prove(wires, pis)
    want = oc.prove(wires, pis, seed=seed or 0)
    assert len(got) == len(want)
    if got != want:
        first = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError(f"proof bytes differ from the oracle at byte {first} of {len(got)}")
    assert oc.verify(got) == 0
    d_w = gpu.to_device(wires)
    try:
        if seed is not None:
            circ.set_blinding_seed(seed)
        assert circ.prove_dev(d_w, pis) == want
    finally:
        d_w.free()


@pytest.mark.parametrize("label", fs.LABELS)
def test_schedule_proof_bytes_match_oracle(pkg, gpu, orc, label):
    row = fs.BY_LABEL[label]
    pack, wires, pis = fs.synth_case(pkg, row, seed=700 + fs.LABELS.index(label))
    assert [int(x) for x in pack[18:18 + int(pack[17])]] == row["arity_bits"]
    oc = OracleCircuit(orc, pack); circ = pkg.Circuit(gpu, pack)
    try:
        assert_parity(gpu, circ, oc, wires, pis)
    finally:
        circ.close(); oc.close()


@pytest.mark.parametrize("label", ["twos", "falling"])
def test_schedule_full_gate_mix_and_zero_knowledge(pkg, gpu, orc, label):
    """Default widths (135 wires, 80 routed), all synthetic gate families, degree_bits 8; then the same circuit with salted oracles
    under a seed both sides share."""
    row = fs.BY_LABEL[label]
    assert row["degree_bits"] == 8
    pack, wires, pis = fs.synth_case(pkg, row, seed=720, **FULL_MIX)
    zk = pack.copy(); zk[14] = 1
    for p, seed in ((pack, None), (zk, 0xF00D)):
        oc = OracleCircuit(orc, p); circ = pkg.Circuit(gpu, p)
        try:
            assert_parity(gpu, circ, oc, wires, pis, seed=seed)
        finally:
            circ.close(); oc.close()


@pytest.mark.parametrize("label", ["ones", "falling"])
def test_schedule_lockstep_batch(pkg, gpu, orc, label):
    """Three different witnesses in one lockstep batch (qpgpu_prove_batch_dev): the per-proof strides of the fold, interleave and
    gather kernels under the schedule. Each proof equals the oracle's."""
    from test_batch_gpu import _witnesses
    row = fs.BY_LABEL[label]
    pack, wires, _ = fs.synth_case(pkg, row, seed=730, **WITH_PI_CELLS)
    pis, ws = _witnesses(pkg, gpu, pack, wires, 3)
    circ = pkg.Circuit(gpu, pack, max_batch=3)
    oc = OracleCircuit(orc, pack)
    bufs = [gpu.to_device(w) for w in ws]
    try:
        got = circ.prove_batch_dev(bufs, pis)
        assert len(set(got)) == 3
        for b in range(3):
            assert got[b] == oc.prove(ws[b], pis[b]), b
            assert oc.verify(got[b]) == 0
    finally:
        for x in bufs:
            x.free()
        circ.close(); oc.close()


def test_schedule_under_poseidon2_hasher(pkg, gpu, orc):
    """`threes` with Poseidon2 (the qp set) as the proof-system hasher: FRI leaves of 16 elements through the other sponge."""
    row = fs.BY_LABEL["threes"]
    prm = pkg.poseidon2_qp_params()
    g2 = pkg.QpGpu(0, hasher=prm)
    pkg.set_hasher_poseidon2(*prm)              # the synthetic witness hashes its public inputs under the process default
    orc.select_poseidon2(*prm)
    try:
        pack, wires, pis = fs.synth_case(pkg, row, seed=740)
        oc = OracleCircuit(orc, pack); circ = pkg.Circuit(g2, pack)
        try:
            assert_parity(g2, circ, oc, wires, pis)
        finally:
            circ.close(); oc.close()
    finally:
        orc.select_poseidon()
        pkg.set_hasher_poseidon()
        g2.close()


def test_prover_refuses_a_schedule_below_the_cap(pkg, gpu, orc):
    """degree_bits 8, rate 3, cap 4, [4, 4]: the second round's tree (2^3 leaves) is smaller than the cap. The circuit loader
    refuses it (it used to load, and the proof layout sized a Merkle path as 3 - 4); the context keeps proving."""
    row = fs.BY_LABEL["twos"]
    pack, wires, pis = fs.synth_case(pkg, row, seed=750)
    with pytest.raises(pkg.QpGpuError) as e:
        pkg.Circuit(gpu, fs.with_schedule(pack, [4, 4]))
    assert "cap height" in str(e.value)
    oc = OracleCircuit(orc, pack); circ = pkg.Circuit(gpu, pack)
    try:
        assert circ.prove(wires, pis) == oc.prove(wires, pis)
    finally:
        circ.close(); oc.close()
