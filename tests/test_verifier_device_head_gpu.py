"""Batch verification wholly on the device (qpgpu_verifier_verify_many_device_ex with QPGPU_VERIFY_HEAD_ON_DEVICE,
include/qpgpu_verify.h): transcript, proof of work and quotient identity as kernels in front of the query-round kernels. The
host verifier is the specification everywhere: results, every reason row, return value and err equal qpgpu_verifier_verify /
verify_many, for every proof of every batch.

Which fixture has which gate type evaluated by the identity kernel (test_every_gate_type_is_evaluated_on_the_device asserts the
union from the packs themselves):
  bench shape (2^13, Poseidon)        Noop, Constant, PublicInput, Arithmetic, Poseidon, BaseSum
  zero knowledge / recursion=True     + ArithmeticExtension, MulExtension, Reducing, ReducingExtension, RandomAccess,
                                        Exponentiation, PoseidonMds
  restated leaf circuit               Poseidon2 (default wire layout), BaseSum
  private-batch proof                 ArithmeticExtension, MulExtension, Reducing, ReducingExtension, RandomAccess,
                                        CosetInterpolation, PoseidonMds
  p2_alt_layout=True                  Poseidon2 with the second wire layout of tests/test_poseidon2_gate_gpu.py"""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc
from test_verifier_device_gpu import (CAP, EINVAL, EVERIFY, SCHEDULE_LABELS, Layout, assert_oracle_agrees, close_schedule_fixture, host_call,
                                      schedule_fixture, set_word, tamper_corpus, word)

pytestmark = pytest.mark.gpu

HEAD_ON_DEVICE = 1
NONCANONICAL = "proof holds a non-canonical field element"
POW = "proof-of-work response has fewer than"
QUOTIENT = "quotient identity fails at zeta (challenge"
GATE_NAMES = ["Noop", "Constant", "PublicInput", "Arithmetic", "Poseidon", "BaseSum", "ArithmeticExtension", "MulExtension", "Reducing",
              "ReducingExtension", "RandomAccess", "Exponentiation", "PoseidonMds", "CosetInterpolation", "Poseidon2"]


def ex_call(v, gpu, proofs, flags=HEAD_ON_DEVICE, threads=0):
    """(return value, results, reasons, err) of qpgpu_verifier_verify_many_device_ex; None entries are passed as NULL."""
    n = len(proofs)
    bufs = [None if p is None else bytes(p) for p in proofs]
    ptrs = (ctypes.c_char_p * n)(*bufs)
    lens = (ctypes.c_size_t * n)(*[0 if b is None else len(b) for b in bufs])
    res = (ctypes.c_int * n)()
    rows = ctypes.create_string_buffer(CAP * n)
    err = ctypes.create_string_buffer(CAP)
    rc = v.lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, n, threads, flags, res, rows, err)
    raw = rows.raw
    return rc, list(res), [raw[CAP * i:CAP * (i + 1)].split(b"\0", 1)[0].decode() for i in range(n)], err.value.decode()


def assert_same_as_host(v, gpu, proofs, flags=HEAD_ON_DEVICE):
    got, want = ex_call(v, gpu, proofs, flags), host_call(v, proofs)
    assert got[1] == want[1], [(i, a, b, got[2][i], want[2][i]) for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:8]
    for i, (a, b) in enumerate(zip(got[2], want[2])):
        assert a == b, (i, a, b)
    assert got[0] == want[0] and got[3] == want[3], (got[0], got[3], want[0], want[3])
    return got


def gate_types(pkg, pack):
    """the gate types of a pack's gate table that carry constraints, plus Noop if listed"""
    h = pkg.pack_header(pack)
    at = 18 + h["num_arity_rounds"]
    return {int(pack[at + 8 * g]) for g in range(int(pack[16]))}


def head_regions(pkg, pack):
    """[(name, byte position)] of one word per region the head reads; the opening vectors with their first and last element"""
    lay = Layout(pkg, pack)
    h = lay.h
    nch = h["num_challenges"]
    counts = [h["num_selectors"] + h["num_constants"], h["num_routed_wires"], h["num_wires"], nch, nch, nch * h["num_partial_products"],
              nch * h["quotient_degree_factor"]]
    names = ["constants", "sigmas", "wires", "zs", "zs_next", "partial_products", "quotient"]
    out = [("wires cap", 8), ("zs cap", lay.cap_bytes + 16), ("quotient cap", 2 * lay.cap_bytes)]
    pos = lay.openings_pos
    openings = []
    for name, cnt in zip(names, counts):
        if cnt:
            openings += [(name + " first", pos), (name + " last", pos + 16 * cnt - 8)]
        pos += 16 * cnt
    assert pos == lay.fri_caps_pos
    out += openings
    if lay.arity_bits:
        out.append(("FRI cap", lay.fri_caps_pos + 8))
    out += [("final polynomial", lay.final_pos + 8), ("witness", lay.pow_pos)]
    if h["num_public_inputs"]:
        out.append(("public input", lay.pis_pos))
    return out, [n for n, _ in openings]


def head_corpus(pkg, pack, proof):
    """One tampered copy per region the head reads: a changed word, the value p, the value 2^64 - 1. Returns (names, proofs)."""
    regions, _ = head_regions(pkg, pack)
    names, out = [], []
    for name, pos in regions:
        for kind, value in (("flip", lambda b: (word(b, pos) + 1) % pkg.P), ("p", lambda b: pkg.P), ("max", lambda b: (1 << 64) - 1)):
            b = bytearray(proof)
            set_word(b, pos, value(b))
            names.append((name, kind)); out.append(bytes(b))
    return names, out


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bench(pkg, gpu):
    """A lockstep batch of bench-shape proofs (2^13 rows, 135 wires, 80 routed, Poseidon)."""
    agg = pkg.aggregation
    pack, wires, _ = pkg.synth_circuit(13, num_wires=135, num_routed=80, num_public_inputs=21, seed=1000, poseidon=True, base_sum=True)
    tp = agg.TemplateProver(gpu, pack, wires, max_batch=8)
    v = pkg.Verifier(pack, circuit=tp.circ)
    tp.commit_many([agg.leaf_public_inputs(i) for i in range(8)])
    proofs = tp.prove_many()
    yield pack, v, proofs
    v.close(); tp.close()


def synth_fixture(pkg, gpu, d, zk=False, no_pow=False, count=2, **kw):
    pack, wires, pis = pkg.synth_circuit(d, **kw)
    if zk:
        pack[14] = 1
    if no_pow:
        pack[12] = 0                    # proof_of_work_bits: every transcript passes, so the quotient identity is what a flip meets
    circ = pkg.Circuit(gpu, pack)
    v = pkg.Verifier(pack, circuit=circ)
    circ.set_blinding_seed(7)
    proofs = [circ.prove(wires, pis) for _ in range(count)]
    return pack, v, proofs, circ


@pytest.fixture(scope="module")
def zk(pkg, gpu):
    """Zero knowledge at 2^9 with every synthetic gate family: salted rows, Exponentiation among the recursion gates."""
    pack, v, proofs, circ = synth_fixture(pkg, gpu, 9, zk=True, num_wires=135, num_routed=60, num_public_inputs=21, seed=321, poseidon=True,
                                          base_sum=True, ext_arith=True, recursion=True)
    yield pack, v, proofs
    v.close(); circ.close()


@pytest.fixture(scope="module")
def no_pow(pkg, gpu):
    """The synthetic 15-family circuit without proof of work: the route to the quotient-identity message."""
    pack, v, proofs, circ = synth_fixture(pkg, gpu, 8, no_pow=True, seed=4, poseidon=True, base_sum=True, ext_arith=True, recursion=True,
                                          poseidon2=True)
    yield pack, v, proofs
    v.close(); circ.close()


@pytest.fixture(scope="module")
def batches(pkg, gpu):
    """Leaf proofs from CircuitInputs and a private-batch proof over them, the prover verifying wholly on the device."""
    L, R = pkg.leaf, pkg.recursion
    leaf = L.LeafCircuit()
    priv = R.PrivateBatchProver(pkg, gpu, leaf, 2, verify_on_device="full")
    leaves = [priv.leaf_prover.prove(x)[0] for x in lc.shared_tree_inputs(L, 2, exits=[(bytes([4] * 32), bytes([7] * 32))] * 2,
                                                                          outputs=[(200, 97), (150, 10)])]
    pb = priv.commit(leaves, seed=bytes(range(32))).prove()
    yield leaf, priv, leaves, pb
    priv.close()


def test_new_entry_point_with_the_device_head_flag(bench, gpu):
    pack, v, proofs = bench
    rc, res, reasons, err = assert_same_as_host(v, gpu, proofs)
    assert rc == 0 and res == [0] * len(proofs) and reasons == [""] * len(proofs) and err == ""


def test_python_verify_many_device_head(bench, pkg, gpu):
    pack, v, proofs = bench
    assert v.verify_many(proofs, gpu=gpu, device_head=True) == [True] * len(proofs) and v.reasons == [""] * len(proofs)
    bad = bytearray(proofs[3]); bad[Layout(pkg, pack).openings_pos + 3] ^= 1
    got = v.verify_many(proofs[:3] + [bytes(bad)], gpu=gpu, device_head=True)
    want = host_call(v, proofs[:3] + [bytes(bad)])
    assert got == [True, True, True, False] and v.reasons == want[2] and v.results == want[1] and v.reason == want[3]
    with pytest.raises(ValueError):
        v.verify_many(proofs, device_head=True)


def test_accepts_zero_knowledge_proofs(zk, gpu):
    pack, v, proofs = zk
    rc, res, _, _ = assert_same_as_host(v, gpu, proofs)
    assert rc == 0 and res == [0] * len(proofs)


def test_accepts_leaf_and_private_batch_proofs(batches, gpu):
    leaf, priv, leaves, pb = batches
    rc, res, _, _ = assert_same_as_host(priv.leaf_verifier, gpu, leaves)
    assert rc == 0 and res == [0, 0]
    rc, res, _, _ = assert_same_as_host(priv.verifier, gpu, [pb, pb])
    assert rc == 0 and res == [0, 0]


@pytest.mark.parametrize("alt", [False, True])
def test_accepts_both_poseidon2_gate_layouts(pkg, gpu, alt):
    from test_poseidon2_gate import KW
    pack, v, proofs, circ = synth_fixture(pkg, gpu, 8, zk=alt, seed=22, ext_arith=True, recursion=True, p2_alt_layout=alt, **KW)
    try:
        assert 14 in gate_types(pkg, pack)
        rc, res, _, _ = assert_same_as_host(v, gpu, proofs)
        assert rc == 0 and res == [0, 0]
        names, corpus = head_corpus(pkg, pack, proofs[0])
        assert_same_as_host(v, gpu, corpus)
    finally:
        v.close(); circ.close()


def test_every_gate_type_is_evaluated_on_the_device(pkg, bench, zk, no_pow, batches):
    leaf, priv, leaves, pb = batches
    seen = gate_types(pkg, bench[0]) | gate_types(pkg, zk[0]) | gate_types(pkg, no_pow[0]) | gate_types(pkg, leaf.pack) | gate_types(pkg, priv.circuit.pack)
    assert seen == set(range(15)), [GATE_NAMES[t] for t in set(range(15)) - seen]


@pytest.mark.parametrize("block", ["qp", "other"])
def test_accepts_proofs_under_poseidon2(pkg, block):
    """Poseidon2 as the proof-system hasher: the qp set (multiplication-free plug) and another block (general plug); with the
    Poseidon tests above all three permutation plugs run the transcript kernel."""
    from test_hasher_plug import placeholder_params
    prm = pkg.poseidon2_qp_params() if block == "qp" else placeholder_params()
    flat = pkg.binding._p2_block(*prm)
    g2 = pkg.QpGpu(0, hasher=prm)
    pkg.set_hasher_poseidon2(*prm)              # the synthetic witnesses hash their public inputs under the process default
    try:
        for d, kw, zk in ((8, dict(seed=81, num_wires=24, num_routed=16, num_public_inputs=3), False),
                          (9, dict(seed=82, poseidon=True, base_sum=True, ext_arith=True, recursion=True), True)):
            pack, wires, pis = pkg.synth_circuit(d, **kw)
            if zk:
                pack[14] = 1
            circ = pkg.Circuit(g2, pack)
            v = pkg.Verifier(pack, circuit=circ, hasher=1, params=flat)
            try:
                circ.set_blinding_seed(7)
                proofs = [circ.prove(wires, pis) for _ in range(2)]
                rc, res, _, _ = assert_same_as_host(v, g2, proofs)
                assert rc == 0 and res == [0, 0]
                names, corpus = head_corpus(pkg, pack, proofs[1])
                got = assert_same_as_host(v, g2, [proofs[0]] + corpus)
                assert got[1][0] == 0 and got[1].count(0) == 1
            finally:
                v.close(); circ.close()
    finally:
        pkg.set_hasher_poseidon()
        g2.close()


def test_head_tamper_corpus_bench_shape(bench, pkg, gpu):
    """Every region the head reads, then the query regions: the head's verdict comes before a query's."""
    pack, v, proofs = bench
    names, corpus = head_corpus(pkg, pack, proofs[0])
    got = assert_same_as_host(v, gpu, corpus + tamper_corpus(pkg, v, pack, proofs[1]) + [proofs[2]])
    assert got[0] == EVERIFY and got[1][-1] == 0
    for (name, kind), res, why in zip(names, got[1], got[2]):
        assert res == EVERIFY, (name, kind)
        if kind in ("p", "max"):
            assert why == NONCANONICAL, (name, kind, why)
    assert any(POW in r for r in got[2]) and any(r.startswith("query ") for r in got[2])


def test_head_tamper_corpus_zero_knowledge(zk, pkg, gpu):
    pack, v, proofs = zk
    names, corpus = head_corpus(pkg, pack, proofs[1])
    got = assert_same_as_host(v, gpu, corpus + tamper_corpus(pkg, v, pack, proofs[0], seed=12))
    assert got[0] == EVERIFY


def test_quotient_identity_message_without_proof_of_work(no_pow, pkg, gpu):
    """proof_of_work_bits = 0: a changed opening passes the proof of work and must fail the quotient identity, with the
    challenge index the host names. The corpus yields all three of the head's messages on the host verifier."""
    pack, v, proofs = no_pow
    names, corpus = head_corpus(pkg, pack, proofs[0])
    _, opening_names = head_regions(pkg, pack)
    want = host_call(v, corpus)
    for (name, kind), why in zip(names, want[2]):
        if kind == "flip" and name in opening_names:
            assert why.startswith(QUOTIENT), (name, why)       # checked on the host verifier first: the corpus does reach it
    assert any(w == NONCANONICAL for w in want[2]) and any(w.startswith(QUOTIENT) for w in want[2])
    got = assert_same_as_host(v, gpu, corpus + tamper_corpus(pkg, v, pack, proofs[1], seed=13) + proofs)
    assert got[1][-2:] == [0, 0]
    challenges = {w.split("(challenge ")[1][0] for w in got[2] if w.startswith(QUOTIENT)}
    print("quotient-identity challenges reported:", sorted(challenges))


def test_all_three_head_messages_are_reached(bench, no_pow, pkg, gpu):
    seen = []
    for pack, v, proofs in (bench, no_pow):
        names, corpus = head_corpus(pkg, pack, proofs[0])
        seen += ex_call(v, gpu, corpus)[2]
    for needle in (NONCANONICAL, POW, QUOTIENT):
        assert any(s.startswith(needle) for s in seen), (needle, sorted(set(seen)))


def test_mixed_batch_null_and_short(bench, pkg, gpu):
    pack, v, proofs = bench
    lay = Layout(pkg, pack)
    batch = [proofs[i % len(proofs)] for i in range(64)]
    for i, pos in ((0, lay.openings_pos + 40), (5, 3), (17, lay.queries_pos + 11), (40, lay.pow_pos), (63, lay.row(2, 1) + 3)):
        b = bytearray(batch[i]); b[pos] ^= 0x20
        batch[i] = bytes(b)
    batch[9] = None
    batch[33] = proofs[1][:-8]
    b = bytearray(proofs[2]); set_word(b, lay.pis_pos, pkg.P); batch[50] = bytes(b)
    rc, res, reasons, err = assert_same_as_host(v, gpu, batch)
    assert rc == EVERIFY and [i for i, r in enumerate(res) if r] == [0, 5, 9, 17, 33, 40, 50, 63] and res[9] == EINVAL
    assert reasons[50] == NONCANONICAL and reasons[17].startswith("query ") and "bytes" in reasons[33] and err.startswith("proof 0: ")


def test_chunk_boundary_empty_call_and_flags(pkg, gpu):
    """More proofs than one chunk holds (1 024), head and query rejections on each side of the boundary; count == 0 returns 0;
    an unknown flag is refused; flags = 0 is the old entry."""
    pack, wires, pis = pkg.synth_circuit(6, num_wires=24, num_routed=16, num_public_inputs=1, seed=55)
    circ = pkg.Circuit(gpu, pack)
    v = pkg.Verifier(pack, circuit=circ)
    try:
        lay = Layout(pkg, pack)
        proofs = [circ.prove(wires, pis)]
        batch = proofs * (1024 + 40)
        for i, pos in ((1022, lay.openings_pos + 1), (1023, lay.queries_pos + 3), (1024, lay.openings_pos + 17), (1025, lay.queries_pos + 5), (1063, 2)):
            b = bytearray(batch[i]); b[pos] ^= 1
            batch[i] = bytes(b)
        rc, res, reasons, err = assert_same_as_host(v, gpu, batch)
        assert [i for i, r in enumerate(res) if r] == [1022, 1023, 1024, 1025, 1063] and err.startswith("proof 1022: ")
        res = (ctypes.c_int * 1)(-99)
        err = ctypes.create_string_buffer(CAP)
        ptrs = (ctypes.c_char_p * 1)(proofs[0]); lens = (ctypes.c_size_t * 1)(len(proofs[0]))
        assert v.lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, 0, 0, HEAD_ON_DEVICE, res, None, err) == 0
        assert res[0] == -99
        assert v.lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, 1, 0, 2, res, None, err) == EINVAL and res[0] == -99
        assert v.lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, 1, 0, HEAD_ON_DEVICE, res, None, err) == 0 and res[0] == 0
        small = batch[1020:1030]
        from test_verifier_device_gpu import device_call
        assert ex_call(v, gpu, small, flags=0) == device_call(v, gpu, small) == ex_call(v, gpu, small)
    finally:
        v.close(); circ.close()


def test_hasher_rule(pkg, gpu):
    """A Poseidon2 verifier on a Poseidon context: QPGPU_EINVAL with a message, nothing verified."""
    pack, wires, pis = pkg.synth_circuit(6, num_wires=24, num_routed=16, num_public_inputs=1, seed=83)
    v = pkg.Verifier(pack, hasher=1)
    try:
        res = (ctypes.c_int * 1)(-99)
        err = ctypes.create_string_buffer(CAP)
        b = bytes(v.proof_size())
        ptrs = (ctypes.c_char_p * 1)(b); lens = (ctypes.c_size_t * 1)(len(b))
        assert v.lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, 1, 0, HEAD_ON_DEVICE, res, None, err) == EINVAL
        assert b"hasher" in err.value and res[0] == -99
        with pytest.raises(pkg.QpGpuError):
            v.verify_many([b], gpu=gpu, device_head=True)
    finally:
        v.close()


def test_private_batch_prover_with_the_full_device_route(batches, pkg, gpu):
    leaf, priv, leaves, pb = batches
    assert priv.verify_device_head
    forged = bytearray(leaves[1]); forged[Layout(pkg, leaf.pack).openings_pos + 9] ^= 1      # an opening: a head rejection
    msgs = []
    for route in (gpu, None):
        priv.verify_gpu = route
        try:
            with pytest.raises(ValueError) as e:
                priv.commit([leaves[0], bytes(forged)])
            msgs.append(str(e.value))
        finally:
            priv.verify_gpu = gpu
    assert msgs[0] == msgs[1] and "leaf proof 1 failed verification" in msgs[0]
    pub = pkg.recursion.PublicBatchProver(pkg, gpu, priv, 2, verify_on_device="full")
    try:
        pub.commit([pb])
        bad = bytearray(pb); bad[len(bad) // 2] ^= 1
        with pytest.raises(ValueError) as e:
            pub.commit([bytes(bad)])
        assert "private-batch proof 0 failed verification against the pinned private-batch verifier" in str(e.value)
    finally:
        pub.close()


# ---- FRI reduction schedules other than constant arity 16 (tests/fri_schedules.py) ----

@pytest.fixture(scope="module")
def schedules(pkg, gpu, orc):
    fx = schedule_fixture(pkg, gpu, orc)
    yield fx
    close_schedule_fixture(fx)


@pytest.mark.parametrize("label", SCHEDULE_LABELS)
def test_head_on_device_under_other_fri_schedules(schedules, pkg, gpu, label):
    """The device head under each schedule (its round count and its final-polynomial length are the transcript kernel's loop
    bounds: 7 rounds and 2 coefficients, 3 and 1, 3 and 8, 0 and 128): the proofs are accepted, and a changed final polynomial,
    FRI cap (the first opened row where there is no round) and proof-of-work witness get the host's verdict and reason; the
    oracle's verifier gives the same verdicts. Then the whole tamper corpus through the head."""
    pack, v, proofs, oc = schedules[label]
    lay = Layout(pkg, pack)
    assert v.verify_many(proofs, gpu=gpu, device_head=True) == [True] * 4 and v.reasons == [""] * 4
    tampers = []
    for pos in (lay.final_pos + 16 * (lay.final_n - 1) + 8, lay.fri_caps_pos + 8, lay.pow_pos):
        b = bytearray(proofs[2]); set_word(b, pos, (word(b, pos) + 1) % pkg.P)
        tampers.append(bytes(b))
    batch = [proofs[0]] + tampers + [proofs[3]]
    rc, res, reasons, _ = assert_same_as_host(v, gpu, batch)
    assert rc == EVERIFY and res == [0, EVERIFY, EVERIFY, EVERIFY, 0], (res, reasons)
    assert v.verify_many(batch, gpu=gpu, device_head=True) == [True, False, False, False, True] and v.reasons == reasons
    assert_oracle_agrees(oc, batch, res)
    corpus = tamper_corpus(pkg, v, pack, proofs[3], seed=14)
    got = assert_same_as_host(v, gpu, corpus)
    assert got[0] == EVERIFY
    assert_oracle_agrees(oc, corpus, got[1])
