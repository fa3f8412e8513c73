"""Batch verification with the query rounds on the device (qpgpu_verifier_verify_many_device, include/qpgpu_verify.h): every
proof gets the host verifier's verdict and reason (qpgpu_verifier_verify is the specification), the call's return value and err
are host verify_many's. Covers the bench shape, zero knowledge (salted rows), the leaf circuit, a private-batch proof, the three
permutation plugs, a tamper corpus over every region of a proof in one call, chunking, the hasher rule and the opt-in callers."""
import ctypes

import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu

EINVAL, EDEVICE, EVERIFY, CAP = -1, -3, -6, 200


def device_call(v, gpu, proofs, threads=0):
    """(return value, results, reasons, err) of the device entry; None entries are passed as NULL."""
    n = len(proofs)
    bufs = [None if p is None else bytes(p) for p in proofs]
    ptrs = (ctypes.c_char_p * n)(*bufs)
    lens = (ctypes.c_size_t * n)(*[0 if b is None else len(b) for b in bufs])
    res = (ctypes.c_int * n)()
    rows = ctypes.create_string_buffer(CAP * n)
    err = ctypes.create_string_buffer(CAP)
    rc = v.lib.qpgpu_verifier_verify_many_device(v.h, gpu.ctx, ptrs, lens, n, threads, res, rows, err)
    raw = rows.raw
    return rc, list(res), [raw[CAP * i:CAP * (i + 1)].split(b"\0", 1)[0].decode() for i in range(n)], err.value.decode()


def host_call(v, proofs, threads=16):
    """(return value, results, reasons, err): host verify_many, and qpgpu_verifier_verify per proof for the reasons."""
    n = len(proofs)
    bufs = [None if p is None else bytes(p) for p in proofs]
    ptrs = (ctypes.c_char_p * n)(*bufs)
    lens = (ctypes.c_size_t * n)(*[0 if b is None else len(b) for b in bufs])
    res = (ctypes.c_int * n)()
    err = ctypes.create_string_buffer(CAP)
    rc = v.lib.qpgpu_verifier_verify_many(v.h, ptrs, lens, n, threads, res, err)
    reasons = []
    for b in bufs:
        e = ctypes.create_string_buffer(CAP)
        if b is not None:
            v.lib.qpgpu_verifier_verify(v.h, b, len(b), e)
        reasons.append(e.value.decode())
    return rc, list(res), reasons, err.value.decode()


def assert_same_as_host(v, gpu, proofs):
    got, want = device_call(v, gpu, proofs), host_call(v, proofs)
    assert got[1] == want[1], [(i, a, b) for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:8]
    for i, (a, b) in enumerate(zip(got[2], want[2])):
        assert a == b, (i, a, b)
    assert got[0] == want[0] and got[3] == want[3], (got[0], got[3], want[0], want[3])
    return got


class Layout:
    """Byte offsets of a proof of a circuit pack (the layout of csrc/verifier.cpp: proof_size_of)."""

    def __init__(self, pkg, pack):
        h = pkg.pack_header(pack)
        self.h = h
        ab = [int(x) for x in pack[18:18 + h["num_arity_rounds"]]]
        nch, ncs = h["num_challenges"], h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
        nq, npp, nw = nch * h["quotient_degree_factor"], h["num_partial_products"], h["num_wires"]
        salt = 4 if h["zero_knowledge"] else 0
        L, cap_h = h["degree_bits"] + h["rate_bits"], h["cap_height"]
        self.cap_bytes = (1 << cap_h) * 32
        self.openings_pos = 3 * self.cap_bytes
        openings = (ncs + nw + 2 * nch + nch * npp + nq) * 16
        self.fri_caps_pos = self.openings_pos + openings
        self.queries_pos = self.fri_caps_pos + len(ab) * self.cap_bytes
        self.widths = [ncs, nw + salt, nch * (1 + npp) + salt, nq + salt]
        self.arity_bits = ab
        self.opens = []           # (row offset in a query, row words, path length)
        off = 0
        for w in self.widths:
            self.opens.append((off, w, L - cap_h))
            off += 8 * w + 1 + 32 * (L - cap_h)
        lvl = L
        for a in ab:
            lvl -= a
            self.opens.append((off, 2 << a, lvl - cap_h))
            off += 16 * (1 << a) + 1 + 32 * (lvl - cap_h)
        self.q_bytes = off
        self.nq = h["num_query_rounds"]
        self.final_pos = self.queries_pos + self.nq * off
        self.final_n = 1 << (h["degree_bits"] - sum(ab))
        self.pow_pos = self.final_pos + 16 * self.final_n
        self.pis_pos = self.pow_pos + 8

    def row(self, q, k):
        return self.queries_pos + q * self.q_bytes + self.opens[k][0]

    def plen_pos(self, q, k):
        return self.row(q, k) + 8 * self.opens[k][1]


def set_word(b, pos, value):
    b[pos:pos + 8] = int(value).to_bytes(8, "little")


def word(b, pos):
    return int.from_bytes(bytes(b[pos:pos + 8]), "little")


def tamper_corpus(pkg, v, pack, proof, seed=11):
    """One tampered copy of `proof` per region (the list of the issue: opened rows, siblings, path lengths, FRI evaluations and
    paths, final polynomial, proof of work, a cap, an opening, a public input, a non-canonical word, random byte flips)."""
    lay = Layout(pkg, pack)
    pkg.recursion._lib()                       # declares qpgpu_verifier_query_indices' argument types (pointers are 64-bit)
    idx = np.zeros(lay.nq, dtype=np.uint64)
    e = ctypes.create_string_buffer(CAP)
    assert v.lib.qpgpu_verifier_query_indices(v.h, proof, len(proof), idx.ctypes.data, lay.nq, e) == 0, e.value
    out = []

    def variant(fn):
        b = bytearray(proof)
        fn(b)
        out.append(bytes(b))

    P = pkg.P
    for k in range(4):
        for q in (0, lay.nq - 1):
            variant(lambda b, q=q, k=k: set_word(b, lay.row(q, k), (word(b, lay.row(q, k)) + 1) % P))
        variant(lambda b, k=k: b.__setitem__(lay.plen_pos(1, k) + 1 + 8, b[lay.plen_pos(1, k) + 1 + 8] ^ 4))      # a sibling word
    for k in range(len(lay.opens)):
        for val in (61, lay.opens[k][2] - 1 if lay.opens[k][2] else 1):     # a tree that is its own cap has no siblings: claim one
            variant(lambda b, k=k, val=val: b.__setitem__(lay.plen_pos(0, k), val))
    shift = 0
    for r, a in enumerate(lay.arity_bits):
        k = 4 + r
        within = (int(idx[0]) >> shift) & ((1 << a) - 1)
        for slot in (within, (within + 1) % (1 << a)):
            variant(lambda b, k=k, slot=slot: set_word(b, lay.row(0, k) + 16 * slot, (word(b, lay.row(0, k) + 16 * slot) + 5) % P))
        # FRI path (where the round has none, the byte belongs to what follows the empty path: the next query round)
        variant(lambda b, k=k: b.__setitem__(lay.plen_pos(2, k) + 1 + 16, b[lay.plen_pos(2, k) + 1 + 16] ^ 1))
        shift += a
    fin = lay.final_pos + (16 if lay.final_n > 1 else 0)                                                # final polynomial
    variant(lambda b: set_word(b, fin, (word(b, fin) + 1) % P))
    variant(lambda b: set_word(b, lay.pow_pos, (word(b, lay.pow_pos) + 1) % P))                         # proof-of-work witness
    variant(lambda b: b.__setitem__(8, b[8] ^ 1))                                                       # the wires cap
    variant(lambda b: b.__setitem__(lay.openings_pos + 24, b[lay.openings_pos + 24] ^ 1))               # an opening
    if lay.h["num_public_inputs"]:
        variant(lambda b: set_word(b, lay.pis_pos, (word(b, lay.pis_pos) + 1) % P))                     # a public input
    variant(lambda b: set_word(b, lay.row(3, 1) + 8, (1 << 64) - 1))                                    # non-canonical query word
    rng = np.random.default_rng(seed)
    for pos in rng.integers(0, len(proof), 128):
        variant(lambda b, pos=int(pos): b.__setitem__(pos, b[pos] ^ (1 << int(rng.integers(0, 8)))))
    return out


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


@pytest.fixture(scope="module")
def zk(pkg, gpu):
    """Zero knowledge at 2^9: salted rows in the opened oracles."""
    agg = pkg.aggregation
    pack, wires, _ = pkg.synth_circuit(9, num_wires=135, num_routed=60, num_public_inputs=21, seed=321, poseidon=True, base_sum=True, ext_arith=True, recursion=True)
    pack[14] = 1
    tp = agg.TemplateProver(gpu, pack, wires, max_batch=8)
    v = pkg.Verifier(pack, circuit=tp.circ)
    tp.commit_many([agg.leaf_public_inputs(i) for i in range(8)])
    proofs = tp.prove_many()
    yield pack, v, proofs
    v.close(); tp.close()


@pytest.fixture(scope="module")
def batches(pkg, gpu):
    """Leaf proofs from CircuitInputs and a private-batch proof over them, with a prover that verifies on the device."""
    L, R = pkg.leaf, pkg.recursion
    leaf = L.LeafCircuit()
    priv = R.PrivateBatchProver(pkg, gpu, leaf, 2, verify_on_device=True)
    leaves = [priv.leaf_prover.prove(x)[0] for x in lc.shared_tree_inputs(L, 2, exits=[(bytes([4] * 32), bytes([7] * 32))] * 2,
                                                                          outputs=[(200, 97), (150, 10)])]
    pb = priv.commit(leaves, seed=bytes(range(32))).prove()
    yield leaf, priv, leaves, pb
    priv.close()


SCHEDULE_LABELS = ["ones", "falling", "rising", "none_long_final"]
# different witnesses of one circuit come from its public-input cells, a trailer only packs with Poseidon rows carry (135 wires)
WITH_PI_CELLS = dict(poseidon=True, base_sum=True)


def schedule_fixture(pkg, gpu, orc, count=4):
    """label -> (pack, Verifier, proofs, OracleCircuit): `count` proofs of different witnesses of a Poseidon / BaseSum circuit under rows
    of fri_schedules.SCHEDULES."""
    from test_batch_gpu import _witnesses
    out = {}
    for i, label in enumerate(SCHEDULE_LABELS):
        pack, wires, _ = fs.synth_case(pkg, fs.BY_LABEL[label], seed=760 + i, **WITH_PI_CELLS)
        pis, ws = _witnesses(pkg, gpu, pack, wires, count)
        circ = pkg.Circuit(gpu, pack)
        v = pkg.Verifier(pack, circuit=circ)
        proofs = [circ.prove(w, p) for w, p in zip(ws, pis)]
        circ.close()
        out[label] = (pack, v, proofs, OracleCircuit(orc, pack))
    return out


def close_schedule_fixture(fx):
    for _, v, _, oc in fx.values():
        v.close(); oc.close()


@pytest.fixture(scope="module")
def schedules(pkg, gpu, orc):
    fx = schedule_fixture(pkg, gpu, orc)
    yield fx
    close_schedule_fixture(fx)


def assert_oracle_agrees(oc, proofs, results):
    """Three-way agreement: oracle/verify.c accepts exactly what the host verifier (and so the device) accepts."""
    for i, (p, r) in enumerate(zip(proofs, results)):
        assert (oc.verify(p) == 0) == (r == 0), (i, r)


@pytest.mark.parametrize("label", SCHEDULE_LABELS)
def test_accepts_proofs_under_other_fri_schedules(schedules, gpu, label):
    pack, v, proofs, oc = schedules[label]
    assert len(set(proofs)) == len(proofs) == 4
    rc, res, reasons, _ = assert_same_as_host(v, gpu, proofs)
    assert rc == 0 and res == [0] * 4 and reasons == [""] * 4
    assert_oracle_agrees(oc, proofs, res)


@pytest.mark.parametrize("label", SCHEDULE_LABELS)
def test_tamper_corpus_under_other_fri_schedules(schedules, pkg, gpu, label):
    """The tamper corpus per schedule: host and device give the same verdict and reason for every variant, and the oracle's
    verifier the same verdict. Under `ones` (arity 2, the last round's tree is its own cap) both kinds of FRI-round failure are
    reached, and a sibling count other than 0 at that round is refused in the same words on both sides."""
    pack, v, proofs, oc = schedules[label]
    lay = Layout(pkg, pack)
    corpus = tamper_corpus(pkg, v, pack, proofs[1], seed=13)
    got = assert_same_as_host(v, gpu, corpus)
    assert got[0] == EVERIFY and got[1].count(0) < len(corpus) // 4, got[1]
    assert_oracle_agrees(oc, corpus, got[1])
    kinds = {r.split(": ", 1)[-1] for r in got[2] if r}
    for needle in ("Merkle path length of oracle", "does not lead to its cap"):
        assert any(needle in k for k in kinds), (needle, sorted(kinds))
    if label == "ones":
        assert lay.opens[-1][2] == 0 and proofs[1][lay.plen_pos(0, len(lay.opens) - 1)] == 0
        for needle in ("does not continue the previous evaluation", "Merkle path of FRI round", "Merkle path length of FRI round 6 out of range"):
            assert any(needle in k for k in kinds), (needle, sorted(kinds))
        for q in (0, lay.nq - 1):
            for claimed in (1, 2):
                b = bytearray(proofs[1]); b[lay.plen_pos(q, len(lay.opens) - 1)] = claimed
                rc, res, reasons, _ = assert_same_as_host(v, gpu, [proofs[0], bytes(b)])
                assert res == [0, EVERIFY] and reasons[1] == "query %d: Merkle path of FRI round 6 does not lead to its cap" % q, reasons
                assert oc.verify(bytes(b)) != 0
    if label == "none_long_final":
        assert lay.arity_bits == [] and lay.final_n == 128
        assert any("final polynomial" in k for k in kinds) or any("proof-of-work" in k for k in kinds), sorted(kinds)


def test_accepts_what_the_host_accepts_bench_shape(bench, gpu):
    pack, v, proofs = bench
    rc, res, reasons, _ = assert_same_as_host(v, gpu, proofs)
    assert rc == 0 and res == [0] * len(proofs) and reasons == [""] * len(proofs)
    assert v.verify_many(proofs, gpu=gpu) == [True] * len(proofs) and v.reasons == [""] * len(proofs)


def test_accepts_zero_knowledge_proofs(zk, gpu):
    pack, v, proofs = zk
    rc, res, _, _ = assert_same_as_host(v, gpu, proofs)
    assert rc == 0 and res == [0] * len(proofs)


def test_accepts_leaf_and_private_batch_proofs(batches, pkg, gpu):
    leaf, priv, leaves, pb = batches
    rc, res, _, _ = assert_same_as_host(priv.leaf_verifier, gpu, leaves)
    assert rc == 0 and res == [0, 0]
    rc, res, _, _ = assert_same_as_host(priv.verifier, gpu, [pb, pb])
    assert rc == 0 and res == [0, 0]


@pytest.mark.parametrize("block", ["qp", "other"])
def test_accepts_proofs_under_poseidon2(pkg, block):
    """Poseidon2 as the proof-system hasher: the qp set (multiplication-free plug) and another block (general plug); with the
    Poseidon tests above all three permutation plugs run."""
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
                bad = bytearray(proofs[1]); bad[Layout(pkg, pack).final_pos + 1] ^= 2       # in the final polynomial
                rc, res, _, _ = assert_same_as_host(v, g2, [proofs[0], bytes(bad)])
                assert res == [0, EVERIFY]
            finally:
                v.close(); circ.close()
    finally:
        pkg.set_hasher_poseidon()
        g2.close()


def test_tamper_corpus_bench_shape(bench, pkg, gpu):
    pack, v, proofs = bench
    corpus = tamper_corpus(pkg, v, pack, proofs[0])
    got = assert_same_as_host(v, gpu, corpus)
    kinds = {r.split(": ", 1)[-1] for r in got[2] if r}
    assert got[0] == EVERIFY and got[1].count(0) < len(corpus) // 4, got[1]
    # every query-round check a tamper can reach is reached, not just the host's head (the final polynomial is absorbed by the
    # transcript: changing it fails the proof of work first; accepted proofs are what exercise that check)
    for needle in ("Merkle path length of oracle", "does not lead to its cap", "Merkle path length of FRI round",
                   "does not continue the previous evaluation"):
        assert any(needle in k for k in kinds), (needle, sorted(kinds))


def test_tamper_corpus_zero_knowledge(zk, pkg, gpu):
    pack, v, proofs = zk
    corpus = tamper_corpus(pkg, v, pack, proofs[3], seed=12)
    got = assert_same_as_host(v, gpu, corpus)
    assert got[0] == EVERIFY


def test_mixed_batch_null_and_short(bench, gpu):
    pack, v, proofs = bench
    batch = [proofs[i % len(proofs)] for i in range(64)]
    for i in (0, 17, 63):
        b = bytearray(batch[i]); b[len(b) // 2] ^= 0x20
        batch[i] = bytes(b)
    rc, res, reasons, err = assert_same_as_host(v, gpu, batch)
    assert rc == EVERIFY and [i for i, r in enumerate(res) if r] == [0, 17, 63] and err.startswith("proof 0: ")
    rc, res, reasons, err = assert_same_as_host(v, gpu, [proofs[0], None, proofs[1][:-8], proofs[2]])
    assert res[0] == 0 and res[1] == EINVAL and res[2] == EVERIFY and res[3] == 0 and err.startswith("proof 1: ")


def test_chunk_boundary_and_empty_call(pkg, gpu):
    """More proofs than one chunk holds (1 024), a rejection on each side of the boundary; count == 0 returns 0."""
    pack, wires, pis = pkg.synth_circuit(6, num_wires=24, num_routed=16, num_public_inputs=1, seed=55)
    circ = pkg.Circuit(gpu, pack)
    v = pkg.Verifier(pack, circuit=circ)
    try:
        proofs = [circ.prove(wires, pis)]
        batch = proofs * (1024 + 40)
        for i in (1023, 1024):
            b = bytearray(batch[i]); b[Layout(pkg, pack).queries_pos + 3] ^= 1
            batch[i] = bytes(b)
        rc, res, reasons, err = assert_same_as_host(v, gpu, batch)
        assert [i for i, r in enumerate(res) if r] == [1023, 1024] and err.startswith("proof 1023: ")
        res = (ctypes.c_int * 1)(-99)
        err = ctypes.create_string_buffer(CAP)
        ptrs = (ctypes.c_char_p * 1)(proofs[0]); lens = (ctypes.c_size_t * 1)(len(proofs[0]))
        assert v.lib.qpgpu_verifier_verify_many_device(v.h, gpu.ctx, ptrs, lens, 0, 0, res, None, err) == 0
        assert res[0] == -99
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
        assert v.lib.qpgpu_verifier_verify_many_device(v.h, gpu.ctx, ptrs, lens, 1, 0, res, None, err) == EINVAL
        assert b"hasher" in err.value and res[0] == -99
        assert "hasher" in gpu.last_error()
        with pytest.raises(pkg.QpGpuError):
            v.verify_many([b], gpu=gpu)
    finally:
        v.close()


def test_callers_verify_on_device(batches, pkg, gpu):
    leaf, priv, leaves, pb = batches
    seed = bytes([9] * 32)
    priv.commit(leaves, seed=seed)
    priv.circ.set_blinding_seed(5)                             # the salts of the next proof, for reproducible bytes
    on_dev = priv.prove()
    arr_dev = [a.copy() for a in priv.arrangement]
    priv.verify_gpu = None                                     # the default route: the host verifier
    try:
        priv.commit(leaves, seed=seed)
        priv.circ.set_blinding_seed(5)
        on_host = priv.prove()
        arr_host = [a.copy() for a in priv.arrangement]
    finally:
        priv.verify_gpu = gpu
    assert on_dev == on_host and all(np.array_equal(a, b) for a, b in zip(arr_dev, arr_host))
    forged = bytearray(leaves[1]); forged[len(forged) // 2] ^= 1
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
    pub = pkg.recursion.PublicBatchProver(pkg, gpu, priv, 2, verify_on_device=True)
    try:
        pub.commit([pb])
        bad = bytearray(pb); bad[len(bad) // 2] ^= 1
        with pytest.raises(ValueError) as e:
            pub.commit([bytes(bad)])
        assert "private-batch proof 0 failed verification against the pinned private-batch verifier" in str(e.value)
    finally:
        pub.close()
