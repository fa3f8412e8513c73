"""The FRI schedule helpers (tests/fri_schedules.py) and the host side of the schedule table, on the CPU: the restated
ConstantArityBits rule against the packs the library writes, the pack rewriter, the Python-integer FRI replay against proofs of
the CPU oracle (and against tampered ones), and the library's host verifier against oracle/verify.c under every row of the
table. tests/test_fri_schedules_gpu.py and the staged, verifier and wrapper GPU tests run the same rows through the device."""
import numpy as np
import pytest

import fri_schedules as fs
import oracle_binding as ob


def pack_arity(pack):
    return [int(x) for x in pack[18:18 + int(pack[17])]]


def test_table_rows_are_valid_schedules():
    assert len(set(fs.LABELS)) == len(fs.SCHEDULES) == 8
    for s in fs.SCHEDULES:
        L, lvl = s["degree_bits"] + s["rate_bits"], s["degree_bits"] + s["rate_bits"]
        assert all(1 <= a <= 4 for a in s["arity_bits"]) and sum(s["arity_bits"]) <= s["degree_bits"]
        assert L - sum(s["arity_bits"]) >= s["cap_height"], s["label"]
    ones, falling = fs.BY_LABEL["ones"], fs.BY_LABEL["falling"]
    assert ones["degree_bits"] + ones["rate_bits"] - sum(ones["arity_bits"]) == ones["cap_height"]      # last tree is its own cap
    assert sum(falling["arity_bits"]) == falling["degree_bits"]                                       # one coefficient left


def test_constant_arity_is_the_rule_the_library_applies(pkg):
    """Nothing exports fri_reduction_arity_bits, so the rule is compared with the packs it shapes: synthetic packs
    (ConstantArityBits(4, 5) at rate 3, cap 4) over the degrees around every change of round count, and the leaf circuit built
    under configs that move every argument of the rule."""
    from test_leaf_config import build_cfg
    for d in range(3, 15):
        pack, _, _ = pkg.synth_circuit(d, num_wires=8, num_routed=8, num_public_inputs=0, seed=1)
        assert pack_arity(pack) == fs.constant_arity(d, 3, 4, 4, 5), d
    assert fs.constant_arity(5, 3, 4, 4, 5) == [] and fs.constant_arity(6, 3, 4, 4, 5) == [4] and fs.constant_arity(13, 3, 4, 4, 5) == [4, 4]
    assert fs.constant_arity(8, 3, 4, 1, 0) == [1] * 7 and fs.constant_arity(8, 3, 2, 1, 0) == [1] * 8      # the cap stops it; the degree does
    assert fs.constant_arity(8, 3, 8, 4, 0) == [] and fs.constant_arity(3, 3, 0, 4, 0) == []
    for knobs in (dict(), dict(reduction_arity_bits=2), dict(reduction_arity_bits=3, reduction_final_poly_bits=2),
                  dict(reduction_arity_bits=1, reduction_final_poly_bits=0, cap_height=2), dict(reduction_arity_bits=4, reduction_final_poly_bits=8),
                  dict(reduction_arity_bits=1, reduction_final_poly_bits=0, cap_height=8, rate_bits=3)):
        cfg = pkg.circuit_config("leaf", **knobs)
        rc, err, pack, *_ = build_cfg(pkg, 4, cfg)
        assert rc == 0, err
        h = pkg.pack_header(pack)
        assert pack_arity(pack) == fs.constant_arity(h["degree_bits"], cfg.rate_bits, cfg.cap_height, cfg.reduction_arity_bits,
                                                     cfg.reduction_final_poly_bits), knobs


def test_with_schedule_rewrites_only_the_fri_words(pkg):
    pack, _, _ = pkg.synth_circuit(8, num_wires=24, num_routed=16, num_public_inputs=3, seed=2)
    assert pack_arity(pack) == [4]
    same = fs.with_schedule(pack, [4])
    assert np.array_equal(same, pack) and same is not pack
    new = fs.with_schedule(pack, [1, 2, 3], cap_height=2, rate_bits=4, num_queries=9, pow_bits=3)
    assert new.size == pack.size + 2 and pack_arity(new) == [1, 2, 3] and [int(x) for x in new[10:14]] == [4, 2, 3, 9]
    assert np.array_equal(new[:10], pack[:10]) and np.array_equal(new[14:17], pack[14:17]) and np.array_equal(new[21:], pack[19:])
    assert fs.with_schedule(pack, []).size == pack.size - 1
    # the rewriter of tests/test_prove_gpu.py is the special case of the constant-arity-16 rule
    from test_prove_gpu import _with_fri_config
    for knobs in (dict(cap_height=0), dict(cap_height=2, num_queries=1), dict(cap_height=6, pow_bits=0), dict(cap_height=8, pow_bits=8, num_queries=40),
                  dict(pow_bits=18, num_queries=3), dict(rate_bits=5, num_queries=17)):
        big, _, _ = pkg.synth_circuit(9, num_wires=24, num_routed=16, num_public_inputs=3, seed=3)
        cap, rate = knobs.get("cap_height", 4), knobs.get("rate_bits", 3)
        assert np.array_equal(_with_fri_config(big, **knobs), fs.with_schedule(big, fs.constant_arity(9, rate, cap, 4, 5), **knobs)), knobs


@pytest.fixture(scope="module")
def oracle_proofs(pkg, orc):
    """label -> (pack, proof of the CPU oracle, pi_hash, query indices, OracleCircuit) for every row of the table (the oracle's
    stage trace is that of its last proof, so what the tests need from it is copied here)."""
    out = {}
    for i, row in enumerate(fs.SCHEDULES):
        pack, wires, pis = fs.synth_case(pkg, row, seed=700 + i)
        oc = ob.OracleCircuit(orc, pack)
        proof = oc.prove(wires, pis)
        out[row["label"]] = (pack, proof, oc.trace("pi_hash").copy(), [int(x) for x in oc.trace("query_indices")], oc)
    yield out
    for *_, oc in out.values():
        oc.close()


@pytest.mark.parametrize("label", fs.LABELS)
def test_python_replay_accepts_oracle_proofs_and_catches_a_changed_evaluation(pkg, oracle_proofs, label):
    """python_fri_check on a proof of the CPU oracle: every query folds into the final polynomial. One evaluation changed at a
    position other than the queried one passes the continuation check and must fail the interpolation of that round alone."""
    pack, proof, pi_hash, want_indices, oc = oracle_proofs[label]
    ch, fri, lay = fs.fri_of_proof(pkg, pack, proof, pi_hash)
    assert proof.index(fri) + len(fri) + 8 * 3 == len(proof)
    betas, indices = fs.replay_transcript(ch, fri, lay)
    assert indices == want_indices
    assert fs.python_fri_check(fri, lay, betas, indices) == []
    shift = 0
    for r, ab in enumerate(lay.arity_bits):
        q = (5 * r + 3) % lay.num_queries
        other = (((indices[q] >> shift) & ((1 << ab) - 1)) + 1) % (1 << ab)
        pos = lay.queries_pos + q * lay.q_bytes + lay.rounds[r][0] + 16 * other
        b = bytearray(fri); b[pos] ^= 1
        bad = fs.python_fri_check(bytes(b), lay, betas, indices)
        # another query may have drawn the same index and sees the same change; every failure is in this round's fold
        assert bad and all(f[1] == (r + 1 if r + 1 < len(lay.arity_bits) else "final") for f in bad), (r, bad[:3])
        shift += ab
    if lay.final_n:
        b = bytearray(fri); b[lay.final_pos] ^= 1
        bad = fs.python_fri_check(bytes(b), lay, betas, indices)
        assert (len(bad) == lay.num_queries and all(f[1] == "final" for f in bad)) if lay.arity_bits else bad == []


@pytest.mark.parametrize("label", fs.LABELS)
def test_host_verifier_agrees_with_the_oracle_under_every_schedule(pkg, oracle_proofs, label):
    """qpgpu_verifier_verify (barycentric interpolation) and oracle/verify.c (Lagrange form) on the oracle's proof and on one
    tampered copy per region of the FRI part: same verdict for each, and the host's reason names the check the change meets."""
    pack, proof, _, idx, oc = oracle_proofs[label]
    h = pkg.pack_header(pack)
    v = pkg.Verifier(pack)
    try:
        assert v.proof_size() == oc.proof_size() == len(proof)
        assert oc.verify(proof) == 0 and v.verify(proof), v.reason
        _, fri, lay = fs.fri_of_proof(pkg, pack, proof, np.zeros(4, dtype=np.uint64))
        base = proof.index(fri)
        cases, shift = [], 0
        for r, ab in enumerate(lay.arity_bits):
            row = base + lay.queries_pos + 2 * lay.q_bytes + lay.rounds[r][0]
            within = (idx[2] >> shift) & ((1 << ab) - 1)
            cases.append((row + 16 * within, "FRI round %d does not continue the previous evaluation" % r))
            cases.append((row + 16 * ((within + 1) % (1 << ab)) + 8, "Merkle path of FRI round %d does not lead to its cap" % r))
            plen_pos = row + (16 << ab)
            assert proof[plen_pos] == lay.rounds[r][1]
            cases.append((plen_pos, "Merkle path of FRI round %d does not lead to its cap" % r))        # one sibling more or fewer
            if lay.rounds[r][1]:
                cases.append((plen_pos + 1 + 32 * (lay.rounds[r][1] - 1) + 9, "Merkle path of FRI round %d does not lead to its cap" % r))
            shift += ab
        for pos, needle in cases:
            b = bytearray(proof); b[pos] ^= 1
            assert not v.verify(bytes(b)) and needle in v.reason, (pos, needle, v.reason)
            assert oc.verify(bytes(b)) != 0, needle
        for r, ab in enumerate(lay.arity_bits):
            b = bytearray(proof); b[base + lay.queries_pos + lay.rounds[r][0] + (16 << ab)] = 61
            assert not v.verify(bytes(b)) and "query 0: Merkle path length of FRI round %d out of range" % r in v.reason, v.reason
            assert oc.verify(bytes(b)) != 0
        for pos in (base + 8, base + lay.final_pos, base + lay.pow_pos):        # a FRI cap (or the first row), the final polynomial, the witness
            b = bytearray(proof); b[pos] ^= 1
            assert not v.verify(bytes(b)) and oc.verify(bytes(b)) != 0, pos
    finally:
        v.close()
