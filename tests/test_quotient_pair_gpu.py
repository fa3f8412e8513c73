"""Both folded hash gates of the quotient stage from one kernel (quotient_hash_pair_kernel: a PoseidonGate and a Poseidon2 gate on the
same wires share the wire pass, the target wires' S-boxes and the linear term; qfold::pairable decides) against the one-launch-per-gate
form (QPGPU_QUOTIENT_PAIR=0, read at circuit load) and against the CPU oracle, at the shapes of tests/test_quotient_fold_gpu.py: 2^5
and 2^6 rows (one and two workgroups of quotient points per proof at rate 3), rate_bits 4 (q_n < lde_n), lockstep batches of 1 and 3
with their own alphas, two challenges. Exact arithmetic: bytes are compared, no tolerance anywhere. qpgpu_circuit_quotient_pair_info
says which form a circuit runs. The host side is tests/test_quotient_pair_host.py."""
import numpy as np
import pytest

import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_leaf_circuit_gpu import oracle_side
from test_leaf_config import reduced_zk_config
from test_leaf_config_gpu import SEED, blind_of
from test_leaf_config_gpu import oracle_side as zk_oracle_side
from test_quotient_fold_gpu import (BROKEN_P1_ROW, BROKEN_P2_ROW, FRW_LAYOUT, KW, P, SHAPES, _first_bad_row, batch_witnesses, prove_batch,
                                    quotient_cap_of_trace, small_case)
from test_stage_batch_gpu import BatchFlow
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu


def _pair_on_and_off(monkeypatch, run):
    """run() under QPGPU_QUOTIENT_PAIR=1 and =0 (read at circuit load): {"1": result, "0": result}."""
    out = {}
    for pair in ("1", "0"):
        monkeypatch.setenv("QPGPU_QUOTIENT_PAIR", pair)
        out[pair] = run()
    return out


@pytest.mark.parametrize("d,rate_bits", SHAPES)
@pytest.mark.parametrize("nb", [1, 3])
def test_pair_on_equals_pair_off_equals_the_oracle(pkg, gpu, orc, d, rate_bits, nb, monkeypatch):
    pack, wires, pis = small_case(pkg, d, rate_bits, seed=170 + d)
    h = parse_pack(pack)
    assert h["num_challenges"] == 2 and h["rate_bits"] == rate_bits
    made = {}

    def run():
        circ = pkg.Circuit(gpu, pack, max_batch=nb)
        try:
            made["w"] = batch_witnesses(circ, wires, pis, nb)
            return circ.quotient_pair_info(), prove_batch(gpu, circ, *made["w"])
        finally:
            circ.close()

    got = _pair_on_and_off(monkeypatch, run)
    assert got["1"][0] == (True, True) and got["0"][0] == (False, False)
    ws, ps = made["w"]
    oc = OracleCircuit(orc, pack)
    try:
        cap_bytes = (1 << h["cap_height"]) * 32
        for b in range(nb):
            want = oc.prove(ws[b], ps[b])
            # proof bytes begin with the caps of the wires, Z / partial-product and quotient oracles
            assert got["1"][1][b][2 * cap_bytes:3 * cap_bytes] == quotient_cap_of_trace(pkg, gpu, oc, h), (d, rate_bits, b)
            assert got["1"][1][b] == want and got["0"][1][b] == want, (d, rate_bits, b)
    finally:
        oc.close()
    assert len(set(got["1"][1])) == nb                        # every proof of the batch ran under its own alphas


def test_default_is_the_pair_and_the_switch_is_read_at_load(pkg, gpu, monkeypatch):
    pack, _, _ = small_case(pkg, 5, 3, seed=175)
    monkeypatch.delenv("QPGPU_QUOTIENT_PAIR", raising=False)
    circ = pkg.Circuit(gpu, pack)
    try:
        assert circ.quotient_pair_info() == (True, True)
        monkeypatch.setenv("QPGPU_QUOTIENT_PAIR", "0")        # later changes do not reach a loaded circuit
        assert circ.quotient_pair_info() == (True, True)
    finally:
        circ.close()
    import ctypes
    a = ctypes.c_int()
    assert gpu.lib.qpgpu_circuit_quotient_pair_info(None, ctypes.byref(a), ctypes.byref(a)) == -1      # QPGPU_EINVAL


def test_not_selected_without_the_swap(pkg, gpu, orc, monkeypatch):
    monkeypatch.delenv("QPGPU_QUOTIENT_PAIR", raising=False)
    pack, wires, pis = pkg.synth_circuit(6, seed=191, p2_alt_layout=True, **KW)
    assert pkg.pack_p2_layout(pack)["w_swap"] == pkg.P2_NO_SWAP
    circ = pkg.Circuit(gpu, pack, max_batch=3); oc = OracleCircuit(orc, pack)
    try:
        assert circ.quotient_pair_info() == (True, False)
        ws, ps = batch_witnesses(circ, wires, pis, 3)
        assert prove_batch(gpu, circ, ws, ps) == [oc.prove(w, p) for w, p in zip(ws, ps)]
    finally:
        circ.close(); oc.close()


def test_not_selected_with_first_round_wires(pkg, gpu, orc, monkeypatch):
    monkeypatch.delenv("QPGPU_QUOTIENT_PAIR", raising=False)
    L = pkg.leaf
    c = L.LeafCircuit(p2_layout=FRW_LAYOUT, config=pkg.circuit_config("leaf").replace(num_wires=143))
    assert pkg.pack_p2_layout(c.pack)["first_round_wires"] == 1
    x = lc.dummy_inputs(L)
    pr = L.LeafProver(pkg, gpu, c)
    try:
        assert pr.circ.quotient_pair_info() == (True, False)
        assert pr.prove(x)[0] == oracle_side(orc, c, x)[1]
    finally:
        pr.close()


def test_not_selected_without_the_fold(pkg, gpu, orc, monkeypatch):
    monkeypatch.delenv("QPGPU_QUOTIENT_PAIR", raising=False)
    monkeypatch.setenv("QPGPU_QUOTIENT_FOLD", "0")
    pack, wires, pis = small_case(pkg, 6, 3, seed=176)
    circ = pkg.Circuit(gpu, pack); oc = OracleCircuit(orc, pack)
    try:
        assert circ.quotient_pair_info() == (True, False)
        assert circ.prove(wires, pis) == oc.prove(wires, pis)
    finally:
        circ.close(); oc.close()


def test_leaf_circuit_pair_on_equals_pair_off_equals_the_oracle(pkg, gpu, orc, monkeypatch):
    """The restated leaf circuit at its own 2^8 rows, the bench's dummy input and a real spend."""
    L = pkg.leaf
    c = L.LeafCircuit()
    cases = (("dummy", lc.dummy_inputs(L)), ("spend, depth 5", lc.real_inputs(L, depth=5, seed=3)))

    def run():
        pr = L.LeafProver(pkg, gpu, c)
        try:
            return pr.circ.quotient_pair_info()[1], [pr.prove(x)[0] for _, x in cases]
        finally:
            pr.close()

    got = _pair_on_and_off(monkeypatch, run)
    assert got["1"][0] is True and got["0"][0] is False
    want = [oracle_side(orc, c, x)[1] for _, x in cases]
    assert got["1"][1] == want and got["0"][1] == want


def test_zero_knowledge_leaf_pair_on_equals_pair_off_equals_the_oracle(pkg, gpu, orc, monkeypatch):
    """The zero-knowledge leaf under a seeded blinding stream: the same draw either way, so the same bytes, and the oracle's."""
    L = pkg.leaf
    zk = L.LeafCircuit(config=reduced_zk_config(pkg))
    assert pkg.pack_header(zk.pack)["zero_knowledge"] == 1
    x = lc.dummy_inputs(L)

    def run():
        pr = L.LeafProver(pkg, gpu, zk, blinding_seed=SEED)
        try:
            sel = pr.circ.quotient_pair_info()[1]
            proof, _ = pr.prove(x)
            return sel, proof, blind_of(zk, pr.witness())
        finally:
            pr.close()

    got = _pair_on_and_off(monkeypatch, run)
    assert got["1"][0] is True and got["0"][0] is False
    assert np.array_equal(got["1"][2], got["0"][2])
    want = zk_oracle_side(orc, zk, x, got["1"][2], SEED)[1]
    assert got["1"][1] == want and got["0"][1] == want


def test_witness_check_reports_the_same_row(pkg, gpu, monkeypatch):
    """Unsatisfied hash-gate rows: the witness check runs the pair kernel on the trace rows and names the same first row."""
    pack, wires, pis = pkg.synth_circuit(7, seed=24, **KW)
    lay = pkg.pack_p2_layout(pack)
    p2_row, p1_row = BROKEN_P2_ROW, BROKEN_P1_ROW

    def run():
        circ = pkg.Circuit(gpu, pack)
        try:
            circ.set_witness_check(True)
            circ.prove(wires, pis)                            # the satisfied witness passes
            rows = []
            # Poseidon2 gate row: a partial-round S-box input, a second-half one, a delta, an output; PoseidonGate row: the same kinds
            for row, cols in ((p2_row, (lay["w_partial"] + 7, lay["w_full1"] + 30, lay["w_delta"] + 1, lay["w_output"] + 2)),
                              (p1_row, (65 + 9, 29 + 14, 25 + 2, 12 + 3))):
                for col in cols:
                    bad = wires.copy()
                    bad[col, row] = (int(bad[col, row]) + 1) % P
                    rows.append(_first_bad_row(pkg, circ, bad, pis))
            return circ.quotient_pair_info()[1], rows
        finally:
            circ.close()

    got = _pair_on_and_off(monkeypatch, run)
    assert got["1"][0] is True and got["0"][0] is False
    assert got["1"][1] == got["0"][1] == [p2_row] * 4 + [p1_row] * 4


def test_stage_abi_quotient_words(pkg, gpu, orc, monkeypatch):
    """The stage-level route: one quotient call of a stage plan on a lockstep batch of 3 gives the same words with the pair and
    without it (the plan reads the switch when it is made), and the proofs assembled from them are the oracle's."""
    pack, wires, pis = small_case(pkg, 6, 3, seed=177)
    circ = pkg.Circuit(gpu, pack)
    try:
        ws, ps = batch_witnesses(circ, wires, pis, 3)
    finally:
        circ.close()

    def run():
        fl = BatchFlow(pkg, gpu, orc, pack, 3)
        try:
            proofs, _, q = fl.prove_batch(ws, ps)
            return proofs, q
        finally:
            fl.close()

    got = _pair_on_and_off(monkeypatch, run)
    assert np.array_equal(got["1"][1], got["0"][1])
    oc = OracleCircuit(orc, pack)
    try:
        want = [oc.prove(w, p) for w, p in zip(ws, ps)]
    finally:
        oc.close()
    assert got["1"][0] == want and got["0"][0] == want
