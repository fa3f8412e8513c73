"""Stage-level C ABI (qpgpu_oracle_*, qpgpu_challenger_*, qpgpu_fri_prove): the flow a patched plonky2 prove() would
run — commitments, opening evaluations and the FRI proof on the GPU, gate-dependent stages elsewhere — must reproduce
the CPU restatement's proof byte for byte. The gate-dependent intermediate columns (Z / partial products, quotient
chunks) come from the oracle's stage trace, standing in for the Rust code that would compute them."""
import numpy as np
import pytest

import fri_schedules as fs
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


def parse_pack(pack):
    names = ["degree_bits", "num_wires", "num_routed_wires", "num_constants", "num_selectors", "num_challenges",
             "quotient_degree_factor", "num_partial_products", "num_public_inputs", "rate_bits", "cap_height",
             "proof_of_work_bits", "num_query_rounds", "zero_knowledge", "num_gate_constraints", "num_gates", "num_arity_rounds"]
    h = {k: int(pack[1 + i]) for i, k in enumerate(names)}
    off = 18
    h["arity_bits"] = [int(x) for x in pack[off:off + h["num_arity_rounds"]]]; off += h["num_arity_rounds"]
    off += 8 * h["num_gates"] + h["num_routed_wires"]
    h["circuit_digest"] = pack[off:off + 4].copy(); off += 4
    n = 1 << h["degree_bits"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    h["constants_sigmas"] = pack[off:off + ncs * n].reshape(ncs, n)
    return h


def staged_proof(pkg, gpu, orc, oc, pack, wires, pis, seed=0, fri_out=None):
    """fri_out: a dict that receives the FriProof bytes, a copy of the challenger as it stood when FRI began, and the leaf
    widths of the four oracles (what fri_schedules.python_fri_check replays)."""
    h = parse_pack(pack)
    d, nch, zk = h["degree_bits"], h["num_challenges"], bool(h["zero_knowledge"])
    n = 1 << d
    want = oc.prove(wires, pis, seed=seed)               # fills the stage trace
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    zkw = dict(blinding=zk, blinding_seed=seed)
    ch = pkg.Challenger()
    o_cs = pkg.PolyOracle(gpu, h["constants_sigmas"], **kw)
    o_w = pkg.PolyOracle(gpu, wires, blinding_stream=1, **kw, **zkw)
    ch.observe(h["circuit_digest"]); ch.observe(oc.trace("pi_hash")); ch.observe(o_w.cap())
    betas, gammas = ch.get_n(nch), ch.get_n(nch)
    assert betas == list(oc.trace("betas")) and gammas == list(oc.trace("gammas"))
    zs_vals = oc.trace("zs_pp_values").reshape(-1, n)
    o_zs = pkg.PolyOracle(gpu, zs_vals, blinding_stream=2, **kw, **zkw)
    ch.observe(o_zs.cap())
    assert ch.get_n(nch) == list(oc.trace("alphas"))
    o_q = pkg.PolyOracle(gpu, oc.trace("quotient_chunk_coeffs").reshape(-1, n), coeffs=True, blinding_stream=3, **kw, **zkw)
    ch.observe(o_q.cap())
    zeta = ch.get_n(2)
    assert zeta == list(oc.trace("zeta"))
    g = orc.root(d)
    g_zeta = [orc.mul(zeta[0], g), orc.mul(zeta[1], g)]
    oracles = [o_cs, o_w, o_zs, o_q]
    opens = [o.eval(zeta) for o in oracles]
    zs_next = o_zs.eval(g_zeta, 0, nch)
    ch.observe(np.concatenate(opens)); ch.observe(zs_next)
    if fri_out is not None:
        fri_out["challenger"] = fs.copy_challenger(pkg, ch)
        fri_out["leaf_widths"] = [o.num_polys + (4 if zk and i else 0) for i, o in enumerate(oracles)]
    fri = pkg.fri_prove(gpu, oracles, [(zeta, [(0, 0, o_cs.num_polys), (1, 0, o_w.num_polys), (2, 0, o_zs.num_polys), (3, 0, o_q.num_polys)]),
                                       (g_zeta, [(2, 0, nch)])],
                        ch, h["arity_bits"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"], **kw)
    # ProofWithPublicInputs::to_bytes: caps, openings (zs, zs_next, partial products split out of the Z/PP oracle), FRI, PIs
    zs_open = opens[2]
    parts = [o_w.cap(), o_zs.cap(), o_q.cap(), opens[0], opens[1], zs_open[:nch], zs_next, zs_open[nch:], opens[3]]
    got = b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in parts) + fri + \
        (np.asarray(pis, dtype=np.uint64) % np.uint64(P)).tobytes()
    for o in oracles:
        o.close()
    if fri_out is not None:
        fri_out["fri"] = fri
    return got, want


def test_staged_flow_reproduces_the_proof(pkg, gpu, orc):
    for d, kwargs in ((8, dict(seed=61)), (10, dict(seed=62, poseidon=True, base_sum=True)), (6, dict(seed=63, num_wires=24, num_routed=16, num_public_inputs=3))):
        pack, wires, pis = pkg.synth_circuit(d, **kwargs)
        oc = OracleCircuit(orc, pack)
        got, want = staged_proof(pkg, gpu, orc, oc, pack, wires, pis)
        assert len(got) == len(want)
        assert got == want, f"staged proof differs at byte {next(i for i in range(len(got)) if got[i] != want[i])}"
        assert oc.verify(got) == 0
        oc.close()


# (label, degree_bits, rate_bits, cap_height, arity_bits, replay in Python integers?): reductions of 5..8 bits are the stage ABI's
# alone (the pack loader stops at 4), so the pack is rewritten for the oracle only and the device never loads it as a circuit
STAGE_SCHEDULES = [("five", 9, 3, 4, [5], True),
                   ("eight", 9, 3, 4, [8], False),            # FRI leaves of 512 elements, 16 of them: the cap itself, path length 0
                   ("six_one", 10, 3, 4, [6, 1], False)] + \
                  [(s["label"], s["degree_bits"], s["rate_bits"], s["cap_height"], s["arity_bits"], True) for s in (fs.BY_LABEL["falling"], fs.BY_LABEL["ones"])]


@pytest.mark.parametrize("label,d,rate_bits,cap_height,arity_bits,replay", STAGE_SCHEDULES, ids=[c[0] for c in STAGE_SCHEDULES])
def test_staged_flow_under_other_schedules(pkg, gpu, orc, label, d, rate_bits, cap_height, arity_bits, replay):
    """qpgpu_fri_prove under reduction schedules away from arity 16, byte for byte against the oracle; for three of them the FRI
    commit phase is replayed in Python integers as well (fri_schedules.python_fri_check): every query of the device's FriProof
    folds, round by round, into the final polynomial under plain Lagrange interpolation."""
    pack, wires, pis = pkg.synth_circuit(d, seed=65, num_wires=24, num_routed=16, num_public_inputs=3)
    pack = fs.with_schedule(pack, arity_bits, cap_height=cap_height, rate_bits=rate_bits)
    oc = OracleCircuit(orc, pack)
    out = {}
    try:
        got, want = staged_proof(pkg, gpu, orc, oc, pack, wires, pis, fri_out=out)
        assert len(got) == len(want)
        assert got == want, f"staged proof differs at byte {next(i for i in range(len(got)) if got[i] != want[i])}"
        assert oc.verify(got) == 0
    finally:
        oc.close()
    if replay:
        h = parse_pack(pack)
        lay = fs.FriLayout(d, rate_bits, cap_height, arity_bits, h["num_query_rounds"], out["leaf_widths"])
        betas, indices = fs.replay_transcript(out["challenger"], out["fri"], lay)
        assert len(indices) == h["num_query_rounds"] and len(betas) == len(arity_bits)
        assert fs.python_fri_check(out["fri"], lay, betas, indices) == []


def _fri_prove_raw(pkg, gpu, oracle, challenger, arity_bits, cap_height):
    """qpgpu_fri_prove itself on one oracle's first two polynomials at the point (3, 4), without the size query pkg.fri_prove
    makes first: (return code, bytes written)."""
    import ctypes
    B = pkg.binding
    hs = (ctypes.c_void_p * 1)(oracle.h)
    bs = (B._FriBatch * 1)()
    bs[0].point[0], bs[0].point[1], bs[0].num_ranges = 3, 4, 1
    bs[0].ranges[0].oracle, bs[0].ranges[0].first, bs[0].ranges[0].count = 0, 0, 2
    prm = B._FriParams(oracle.rate_bits, cap_height, 4, 5, len(arity_bits))
    for i, a in enumerate(arity_bits):
        prm.reduction_arity_bits[i] = a
    out = np.zeros(1 << 16, dtype=np.uint8)
    ln = ctypes.c_size_t(0)
    rc = gpu.lib.qpgpu_fri_prove(gpu.ctx, hs, 1, ctypes.byref(bs), 1, ctypes.byref(prm), ctypes.byref(challenger.state), out.ctypes.data,
                                 out.size, ctypes.byref(ln))
    return rc, out[:ln.value].tobytes()


def test_stage_api_refuses_bad_schedules(pkg, gpu):
    """Schedules qpgpu_fri_prove must refuse, through the binding (which asks qpgpu_fri_proof_size first) and at the entry
    itself: deeper than the degree, a tree below the cap, a round of 0 or 9 bits. Each is QPGPU_EINVAL; the context and the
    oracle keep working (a good call follows, and its FriProof replays in Python integers)."""
    rng = np.random.default_rng(66)
    vals = rng.integers(0, P, size=(2, 64), dtype=np.uint64)                   # degree_bits 6, rate 3: the LDE has 2^9 points
    o = pkg.PolyOracle(gpu, vals, rate_bits=3, cap_height=4)
    try:
        # sum 7 > 6 twice; sum 6 leaves a tree of 2^3 leaves under a cap of 2^4; rounds of 0 and 9 bits
        for bad in ([4, 3], [3, 3, 1], [3, 3], [0], [2, 0], [9], [1, 9]):
            with pytest.raises(pkg.QpGpuError):
                pkg.fri_prove(gpu, [o], [([3, 4], [(0, 0, 2)])], pkg.Challenger(), bad, cap_height=4)
            rc, out = _fri_prove_raw(pkg, gpu, o, pkg.Challenger(), bad, 4)
            assert rc == -1 and out == b"", (bad, rc)
        lay = fs.FriLayout(6, 3, 4, [3, 2], 5, [2])
        ch = pkg.Challenger()
        rc, fri = _fri_prove_raw(pkg, gpu, o, ch, [3, 2], 4)
        assert rc == 0 and len(fri) == lay.total
        ch2 = pkg.Challenger()
        assert fri == pkg.fri_prove(gpu, [o], [([3, 4], [(0, 0, 2)])], fs.copy_challenger(pkg, ch2), [3, 2], cap_height=4, proof_of_work_bits=4,
                                    num_query_rounds=5)
        betas, indices = fs.replay_transcript(ch2, fri, lay)
        assert fs.python_fri_check(fri, lay, betas, indices) == []
    finally:
        o.close()


def test_staged_flow_zero_knowledge(pkg, gpu, orc):
    pack, wires, pis = pkg.synth_circuit(7, seed=64, poseidon=True)
    pack = pack.copy(); pack[14] = 1
    oc = OracleCircuit(orc, pack)
    got, want = staged_proof(pkg, gpu, orc, oc, pack, wires, pis, seed=4242)
    assert got == want
    oc.close()


def test_oracle_read_and_eval(pkg, gpu, orc):
    rng = np.random.default_rng(5)
    vals = rng.integers(0, P, size=(5, 256), dtype=np.uint64)
    o = pkg.PolyOracle(gpu, vals, rate_bits=2, cap_height=3)
    coeffs = o.read()
    ref_coeffs, ref_lde = orc.lde_batch(vals, 8, 2, pkg.MULT_GEN)      # natural-order values on the coset g<w>
    assert (coeffs == ref_coeffs).all()
    lde = o.read(lde=True)
    assert lde.shape == (5, 1024)
    brev = np.array([int(format(i, "010b")[::-1], 2) for i in range(1024)])
    assert (lde == ref_lde[:, brev]).all()                               # slot s holds the value at g*w^bitrev(s)
    leaves = np.ascontiguousarray(lde.T)
    _, cap = orc.merkle(leaves, 3)
    assert (o.cap() == cap).all()
    # Horner in the extension field F[x]/(x^2 - 7) against the device evaluation
    z = [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]
    got = o.eval(z, 1, 3)

    def ext_mul(x, y):
        a = orc.add(orc.mul(x[0], y[0]), orc.mul(7, orc.mul(x[1], y[1])))
        return [a, orc.add(orc.mul(x[0], y[1]), orc.mul(x[1], y[0]))]
    for j in range(3):
        acc = [0, 0]
        for c in coeffs[1 + j][::-1]:
            acc = ext_mul(acc, z)
            acc[0] = orc.add(acc[0], int(c))
        assert list(map(int, got[j])) == acc
    # a second oracle from the coefficients commits to the same tree
    o2 = pkg.PolyOracle(gpu, coeffs, rate_bits=2, cap_height=3, coeffs=True)
    assert (o.cap() == o2.cap()).all()
    o.close(); o2.close()


def test_stage_api_argument_errors(pkg, gpu):
    vals = np.zeros((2, 64), dtype=np.uint64)
    with pytest.raises(pkg.QpGpuError):
        pkg.PolyOracle(gpu, vals, rate_bits=3, cap_height=12)      # cap above the tree
    o = pkg.PolyOracle(gpu, vals, rate_bits=3, cap_height=2)
    with pytest.raises(pkg.QpGpuError):
        o.eval([1, 2], 1, 5)
    ch = pkg.Challenger()
    with pytest.raises(pkg.QpGpuError):
        pkg.fri_prove(gpu, [o], [([3, 4], [(0, 0, 3)])], ch, [4], cap_height=2)    # range outside the oracle
    with pytest.raises(pkg.QpGpuError):
        pkg.fri_prove(gpu, [o], [([3, 4], [(0, 0, 2)])], ch, [4, 4], cap_height=2)  # reduction deeper than the degree
    o.close()


def test_openings_at_edge_points(pkg, gpu):
    """qpgpu_oracle_eval on structured rows at edge points of the extension field, against Horner in Python integers over
    F[x]/(x^2 - 7). Rows (coefficients, degree 2^8): random, all p - 1, multiples of 2^32, a delta, the field probe's edge set
    reduced mod p in a cycle, random again. Points: (p-1, p-1), (0, 1), (1, 0), (2^32, 2^32 - 1), (p - 2^32, 7) and three random
    ones. Only (1, 0) lies in the base field (an element of the subgroup, off the coset g<w>); evaluation alone is asked for, no
    FRI at these points, so nothing divides by zero."""
    from field_vectors import E
    n = 256
    rng = np.random.default_rng(808)
    rows = np.stack([rng.integers(0, P, n, dtype=np.uint64),
                     np.full(n, P - 1, dtype=np.uint64),
                     (rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)),
                     np.zeros(n, dtype=np.uint64),
                     np.resize(np.array([e % P for e in E], dtype=np.uint64), n),
                     rng.integers(0, P, n, dtype=np.uint64)])
    rows[3, 5] = 1
    assert int(rows.max()) < P
    points = [(P - 1, P - 1), (0, 1), (1, 0), (2**32, 2**32 - 1), (P - 2**32, 7)]
    points += [tuple(int(v) for v in rng.integers(0, P, 2, dtype=np.uint64)) for _ in range(3)]
    o = pkg.PolyOracle(gpu, rows, rate_bits=3, cap_height=4, coeffs=True)
    try:
        assert np.array_equal(o.read(), rows)
        for z in points:
            got = o.eval(list(z))
            for j in range(rows.shape[0]):
                a, b = 0, 0
                for c in rows[j][::-1]:
                    a, b = (a * z[0] + 7 * b * z[1] + int(c)) % P, (a * z[1] + b * z[0]) % P
                assert [int(v) for v in got[j]] == [a, b], (z, j)
    finally:
        o.close()
