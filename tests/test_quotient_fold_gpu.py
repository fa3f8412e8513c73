"""The hash gates of the quotient stage in their folded form (csrc/quotient_fold.hpp: linear layers folded into the alpha weights by
quotient_fold_sweep_kernel, per-point kernels that compute S-boxes and weighted sums only) against the CPU oracle, at the smallest
shapes where they can go wrong: 2^5 and 2^6 rows (one and two workgroups of quotient points per proof at rate 3), rate_bits 4
(q_n < lde_n: the q_shift store path), lockstep batches of 1 and 3 with their own alphas, two challenges. The quotient stage's
output is held to the oracle's `quotient_chunk_coeffs` trace through the staged API: the cap the proof carries for the quotient
oracle must be the cap of that trace committed by qpgpu_oracle_*; the whole proof must equal the oracle's bytes as well. Exact
arithmetic: no tolerance anywhere. The round-by-round form of the hash gates (QPGPU_QUOTIENT_FOLD=0: one kernel over the forward
walk of the same schedule, qfold::walk) is held to the same bytes for every schedule shape: with and without the swap, with and
without round 0's wires. The host side of the fold is tests/test_quotient_fold_host.py."""
import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_leaf_circuit_gpu import oracle_side
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
KW = dict(poseidon=True, poseidon2=True, base_sum=True)
# (degree_bits, rate_bits): rate 4 once, so that the quotient coset is a strict subset of the LDE
SHAPES = [(5, 3), (6, 3), (6, 4)]


def small_case(pkg, d, rate_bits, seed):
    pack, wires, pis = pkg.synth_circuit(d, seed=seed, **KW)
    h = parse_pack(pack)
    if rate_bits != h["rate_bits"]:
        pack = fs.with_schedule(pack, h["arity_bits"], rate_bits=rate_bits)
    return pack, wires, pis


def batch_witnesses(circ, wires, pis, nb):
    """nb different satisfied witnesses of the circuit (other public inputs, so other transcripts and alphas)."""
    mask = circ.witness_free_mask(*wires.shape)
    part = np.where(mask == 1, wires, 0).astype(np.uint64)
    ps = [(pis + np.uint64(b)) % np.uint64(P) for b in range(nb)]
    return [circ.generate_witness(part.copy(), p) for p in ps], ps


def prove_batch(gpu, circ, ws, ps):
    if len(ws) == 1:
        return [circ.prove(ws[0], ps[0])]
    d_w = gpu.to_device(np.stack(ws))
    out = circ.prove_batch_dev([d_w.ptr + b * ws[0].nbytes for b in range(len(ws))], ps)
    d_w.free(scrub=True)
    return out


def quotient_cap_of_trace(pkg, gpu, oc, h):
    """The Merkle cap of the oracle's quotient chunk coefficients, committed through the staged API."""
    n = 1 << h["degree_bits"]
    o_q = pkg.PolyOracle(gpu, oc.trace("quotient_chunk_coeffs").reshape(-1, n), coeffs=True, rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    cap = np.ascontiguousarray(o_q.cap(), dtype=np.uint64).tobytes()
    o_q.close()
    return cap


@pytest.mark.parametrize("d,rate_bits", SHAPES)
@pytest.mark.parametrize("nb", [1, 3])
def test_quotient_output_equals_the_oracle_trace(pkg, gpu, orc, d, rate_bits, nb):
    pack, wires, pis = small_case(pkg, d, rate_bits, seed=70 + d)
    h = parse_pack(pack)
    assert h["num_challenges"] == 2 and h["rate_bits"] == rate_bits and h["quotient_degree_factor"] == 8    # rate 4: q_n = lde_n / 2
    circ = pkg.Circuit(gpu, pack, max_batch=nb); oc = OracleCircuit(orc, pack)
    try:
        ws, ps = batch_witnesses(circ, wires, pis, nb)
        got = prove_batch(gpu, circ, ws, ps)
        cap_bytes = (1 << h["cap_height"]) * 32
        alphas = set()
        for b in range(nb):
            want = oc.prove(ws[b], ps[b])                     # fills the stage trace for this witness
            alphas.add(tuple(oc.trace("alphas")))
            # proof bytes begin with the caps of the wires, Z / partial-product and quotient oracles
            assert got[b][2 * cap_bytes:3 * cap_bytes] == quotient_cap_of_trace(pkg, gpu, oc, h), (d, rate_bits, b)
            assert got[b] == want, (d, rate_bits, b)
        assert len(alphas) == nb                              # every proof of the batch ran under its own alphas
    finally:
        circ.close(); oc.close()


@pytest.mark.parametrize("d,rate_bits", SHAPES)
def test_fold_on_equals_fold_off(pkg, gpu, d, rate_bits, monkeypatch):
    """QPGPU_QUOTIENT_FOLD=0 (read at circuit load) keeps the round-by-round hash-gate kernels: same proofs, byte for byte, for a
    single proof and a lockstep batch of three."""
    pack, wires, pis = small_case(pkg, d, rate_bits, seed=80 + d)
    proofs = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("QPGPU_QUOTIENT_FOLD", fold)
        circ = pkg.Circuit(gpu, pack, max_batch=3)
        try:
            ws, ps = batch_witnesses(circ, wires, pis, 3)
            proofs[fold] = prove_batch(gpu, circ, ws[:1], ps[:1]) + prove_batch(gpu, circ, ws, ps)
        finally:
            circ.close()
    assert proofs["1"] == proofs["0"]
    assert proofs["1"][0] == proofs["1"][1] and len(set(proofs["1"])) == 3


def _fold_on_and_off(monkeypatch, run):
    """run() under QPGPU_QUOTIENT_FOLD=1 and =0 (read at circuit load): {"1": proofs, "0": proofs}."""
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("QPGPU_QUOTIENT_FOLD", fold)
        out[fold] = run()
    return out


def test_fold_on_equals_fold_off_without_swap(pkg, gpu, orc, monkeypatch):
    """The Poseidon2 layout without a swap wire (q0 = 0: the walk's first constraint is a target wire's) through the round-by-round
    kernel: a single proof and a lockstep batch of three at 2^6 rows, fold on == fold off == the oracle, byte for byte."""
    pack, wires, pis = pkg.synth_circuit(6, seed=91, p2_alt_layout=True, **KW)
    assert pkg.pack_p2_layout(pack)["w_swap"] == pkg.P2_NO_SWAP
    made = {}

    def run():
        circ = pkg.Circuit(gpu, pack, max_batch=3)
        try:
            ws, ps = batch_witnesses(circ, wires, pis, 3)
            made["w"] = (ws, ps)
            return prove_batch(gpu, circ, ws[:1], ps[:1]) + prove_batch(gpu, circ, ws, ps)
        finally:
            circ.close()

    proofs = _fold_on_and_off(monkeypatch, run)
    ws, ps = made["w"]
    oc = OracleCircuit(orc, pack)
    try:
        want = [oc.prove(w, p) for w, p in zip(ws, ps)]
    finally:
        oc.close()
    assert proofs["1"] == proofs["0"] == want[:1] + want
    assert len(set(want)) == 3


def test_fold_on_equals_fold_off_with_first_round_wires(pkg, gpu, orc, monkeypatch):
    """The layout that records round 0's S-box inputs too (HEAD_RAW: 31 segments, 118 target wires, no swap) through the
    round-by-round kernel: the leaf circuit at its own 2^8 rows, one proof, fold on == fold off == the oracle."""
    L = pkg.leaf
    c = L.LeafCircuit(p2_layout=FRW_LAYOUT, config=pkg.circuit_config("leaf").replace(num_wires=143))
    lay = pkg.pack_p2_layout(c.pack)
    assert lay["first_round_wires"] == 1 and lay["w_swap"] == pkg.P2_NO_SWAP
    x = lc.dummy_inputs(L)

    def run():
        pr = L.LeafProver(pkg, gpu, c)
        try:
            return pr.prove(x)[0]
        finally:
            pr.close()

    proofs = _fold_on_and_off(monkeypatch, run)
    assert proofs["1"] == proofs["0"] == oracle_side(orc, c, x)[1]


def test_leaf_circuit_proof_bytes(pkg, gpu, orc):
    """The restated leaf circuit at its own 2^8 rows, the bench's dummy input and a real spend."""
    L = pkg.leaf
    c = L.LeafCircuit()
    pr = L.LeafProver(pkg, gpu, c)
    try:
        for name, x in (("dummy", lc.dummy_inputs(L)), ("spend, depth 5", lc.real_inputs(L, depth=5, seed=3))):
            proof, _ = pr.prove(x)
            assert proof == oracle_side(orc, c, x)[1], name
    finally:
        pr.close()


def test_poseidon2_layout_without_swap(pkg, gpu, orc):
    pack, wires, pis = pkg.synth_circuit(6, seed=91, p2_alt_layout=True, **KW)
    assert pkg.pack_p2_layout(pack)["w_swap"] == pkg.P2_NO_SWAP
    circ = pkg.Circuit(gpu, pack); oc = OracleCircuit(orc, pack)
    try:
        assert circ.prove(wires, pis) == oc.prove(wires, pis)
    finally:
        circ.close(); oc.close()


# Poseidon2 gate with the S-box inputs of round 0 on wires as well: 12 in, 12 out, 48 + 22 + 48 S-box inputs, no swap: 142 wires
FRW_LAYOUT = [0, 12, 0xFFFFFFFF, 0, 24, 72, 94, 1, 0, 142]


def test_poseidon2_layout_with_first_round_wires(pkg, gpu, orc):
    L = pkg.leaf
    c = L.LeafCircuit(p2_layout=FRW_LAYOUT, config=pkg.circuit_config("leaf").replace(num_wires=143))
    lay = pkg.pack_p2_layout(c.pack)
    assert lay["first_round_wires"] == 1 and lay["w_swap"] == pkg.P2_NO_SWAP
    pr = L.LeafProver(pkg, gpu, c)
    try:
        x = lc.dummy_inputs(L)
        proof, _ = pr.prove(x)
        assert proof == oracle_side(orc, c, x)[1]
    finally:
        pr.close()


# first failing row the witness check reports for the seeded witnesses below, as the commit before the fold reported it (its
# kernels are the ones QPGPU_QUOTIENT_FOLD=0 selects, and the test runs them too): row 3 of the first Poseidon2 site's gate rows
BROKEN_P2_ROW = 11
BROKEN_P1_ROW = 112


def _first_bad_row(pkg, circ, bad, pis):
    with pytest.raises(pkg.QpGpuError) as e:
        circ.prove(bad, pis)
    assert e.value.code == -4
    msg = str(e.value)
    return int(msg.split("fail at row ")[1].split()[0])


def test_witness_check_reports_the_same_row(pkg, gpu, monkeypatch):
    """Unsatisfied hash-gate rows: the witness check (the gate kernels on the trace rows) names the first of them, as before."""
    pack, wires, pis = pkg.synth_circuit(7, seed=24, **KW)
    lay = pkg.pack_p2_layout(pack)
    sites = pkg.synth_p2_sites(7, 21, **KW)
    p2_row = 8 * sites[0][2] + 3
    h = parse_pack(pack)
    gates = np.asarray(pack[18 + h["num_arity_rounds"]:18 + h["num_arity_rounds"] + 8 * h["num_gates"]]).reshape(-1, 8)
    assert 4 in gates[:, 0].tolist() and 14 in gates[:, 0].tolist()
    # the PoseidonGate rows: where the gate's selector column holds the gate's index
    gi = gates[:, 0].tolist().index(4)
    p1_rows = np.nonzero(h["constants_sigmas"][int(gates[gi, 3])] == np.uint64(gi))[0]
    p1_row = int(p1_rows[-1])
    assert len(p1_rows) >= 1 and p1_row == BROKEN_P1_ROW
    seen = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("QPGPU_QUOTIENT_FOLD", fold)
        circ = pkg.Circuit(gpu, pack)
        try:
            circ.set_witness_check(True)
            circ.prove(wires, pis)                            # the satisfied witness passes
            rows = []
            # a partial-round S-box input, a second-half one, a delta of the Poseidon2 gate row; then the same row and a later one
            for cols, extra in (((lay["w_partial"] + 7,), ()), ((lay["w_full1"] + 30,), ()), ((lay["w_delta"] + 1,), ()),
                                ((lay["w_full0"] + 5,), (p2_row + 8,))):
                bad = wires.copy()
                for col in cols:
                    for row in (p2_row,) + extra:
                        bad[col, row] = (int(bad[col, row]) + 1) % P
                rows.append(_first_bad_row(pkg, circ, bad, pis))
            # PoseidonGate (wires of plonky2's layout): a partial-round S-box input, a first-half one, an output, a delta
            for col in (65 + 9, 29 + 14, 12 + 3, 25 + 2):
                bad = wires.copy()
                bad[col, p1_row] = (int(bad[col, p1_row]) + 1) % P
                rows.append(_first_bad_row(pkg, circ, bad, pis))
            seen[fold] = rows
        finally:
            circ.close()
    assert seen["1"] == seen["0"] == [p2_row] * 4 + [p1_row] * 4
    assert p2_row == BROKEN_P2_ROW
