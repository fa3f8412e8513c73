"""qpgpu_fri_verify and qpgpu_fri_verify_many_device against the proofs qpgpu_fri_prove / FriSession make, on the smallest
instances that reach every branch (ROWS), held to two independent statements: the Python-integer model (tests/fri_verify_model.py)
and, on plonk-shaped instances, the whole-proof verifiers. Host function, device call and model must agree on every verdict as the
triple (kind, query, oracle or round); device and host on code and text. Exact arithmetic: every comparison is equality. Four
query rounds per proof; the largest instance has 2^12 leaves."""
import numpy as np
import pytest

import fri_schedules as fs
import fri_verify_model as fm
import leaf_cases as lc

pytestmark = pytest.mark.gpu
P = fs.P
EINVAL, EVERIFY = -1, -6
NQ = 4

# degree, rate, cap, schedule, oracles (polys, blinded), batches (oracle, first, count), proof_of_work_bits
ROWS = {
    "no_rounds": (5, 1, 0, [], [(3, False)], [[(0, 0, 3)]], 0),                               # the final polynomial is the whole polynomial
    "copied_leaf": (5, 3, 2, [1], [(1, False), (4, False)], [[(0, 0, 1), (1, 0, 4)], [(1, 0, 4)]], 4),   # 4-word round leaf, copied
    "split_ranges": (8, 3, 2, [3, 2], [(5, False), (8, True), (9, False)],
                     [[(0, 0, 2), (0, 2, 3), (1, 0, 8), (2, 0, 9)],
                      [(0, 0, 1), (0, 1, 1), (1, 0, 2), (1, 2, 2), (1, 4, 4), (2, 0, 3), (2, 3, 3), (2, 6, 3)],
                      [(2, 4, 2)]], 4),
    "cap_is_the_tree": (9, 3, 4, [8], [(3, False)], [[(0, 0, 3)]], 0),                          # last tree is the cap: path length 0
    "one_final_coeff": (8, 3, 0, [4, 4], [(17, True)], [[(0, 0, 17)], [(0, 3, 5)]], 10),
    "plonk_shape": None,        # filled by plonk_row(): the four oracles of a 2^9 synthetic circuit, opened at zeta and g zeta
}


def plonk_row(pkg):
    """The FRI instance of a proof of the 24-wire synthetic circuit at 2^9 rows under the `rising` schedule: oracles constants /
    sigmas, wires, Zs / partial products, quotient; batch 0 opens all of them, batch 1 the Zs."""
    row = fs.BY_LABEL["rising"]
    h = pkg.pack_header(fs.synth_case(pkg, row, seed=760)[0])
    nch = h["num_challenges"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    nzp, nq = nch * (1 + h["num_partial_products"]), nch * h["quotient_degree_factor"]
    assert (h["degree_bits"], h["rate_bits"], h["cap_height"], row["arity_bits"]) == (9, 3, 4, [1, 2, 3]) and not h["zero_knowledge"]
    shapes = [(ncs, False), (h["num_wires"], False), (nzp, False), (nq, False)]
    return (9, 3, 4, [1, 2, 3], shapes, [[(0, 0, ncs), (1, 0, h["num_wires"]), (2, 0, nzp), (3, 0, nq)], [(2, 0, nch)]], 4)


class Case:
    """A proof of qpgpu_fri_prove over fresh random oracles of a row's shapes, with everything its verifier is given."""

    def __init__(self, pkg, gpu, row, seed, hasher=0):
        d, rate, cap, arity, shapes, batches, pow_bits = ROWS[row] or plonk_row(pkg)
        rng = np.random.default_rng(seed)
        self.oracles = [pkg.PolyOracle(gpu, rng.integers(0, P, size=(n, 1 << d), dtype=np.uint64), rate_bits=rate, cap_height=cap,
                                       **(dict(blinding=True, blinding_seed=seed + 1, blinding_stream=i) if b else {}))
                        for i, (n, b) in enumerate(shapes)]
        try:
            self.points = [tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in batches]
            if row == "plonk_shape":        # zeta and g zeta
                g = fs.root_of_unity(d)
                self.points[1] = (self.points[0][0] * g % P, self.points[0][1] * g % P)
            self.caps = [o.cap() for o in self.oracles]
            self.openings = np.concatenate([self.oracles[o].eval(pt, f, c) for pt, rg in zip(self.points, batches) for o, f, c in rg])
            ch = pkg.Challenger(gpu)
            ch.observe(np.arange(seed, seed + 11, dtype=np.uint64)); ch.get(); ch.observe([seed, 7])
            self.before = fs.copy_challenger(pkg, ch)
            kw = dict(rate_bits=rate, cap_height=cap, proof_of_work_bits=pow_bits, num_query_rounds=NQ)
            self.proof = pkg.fri_prove(gpu, self.oracles, list(zip(self.points, batches)), ch, arity, **kw)
            self.after = ch
        finally:
            for o in self.oracles:
                o.close()
        self.fv = pkg.FriVerifier(d, shapes, batches, arity, hasher=hasher, **kw)
        self.inst = fm.Instance(d, rate, cap, arity, NQ, shapes, batches, pow_bits=pow_bits)
        self.pkg = pkg
        self.challenges = self.fv.challenges(fs.copy_challenger(pkg, self.before), self.proof)

    def args(self, **change):
        alpha, betas, powr, idx = self.challenges
        a = dict(caps=self.caps, points=self.points, openings=self.openings, alpha=alpha, betas=betas, pow_response=powr, indices=idx, proof=self.proof)
        a.update(change)
        return a

    def close(self):
        self.fv.close()


def host(fv, a):
    fv.verify(**a)
    return fv.code, fv.reason


def many_args(fv, cases):
    """The arrays qpgpu_fri_verify_many_device takes for `cases` (dicts of qpgpu_fri_verify's arguments), every cap per proof."""
    n, nb, nr = len(cases), fv.num_batches, fv.num_rounds
    return ([np.array([np.asarray(c["caps"][o]).reshape(-1) for c in cases]) for o in range(fv.num_oracles)],
            np.array([[c["points"][b] for c in cases] for b in range(nb)], dtype=np.uint64),
            np.array([c["openings"] for c in cases], dtype=np.uint64), np.array([c["alpha"] for c in cases], dtype=np.uint64),
            np.array([c["betas"] for c in cases], dtype=np.uint64).reshape(n, nr, 2) if nr else None,
            [c["pow_response"] for c in cases], np.array([c["indices"] for c in cases], dtype=np.uint64), [c["proof"] for c in cases])


def device(fv, gpu, cases):
    """(code, reason) per case from ONE qpgpu_fri_verify_many_device call."""
    fv.verify_many(*many_args(fv, cases), gpu=gpu, cap_counts=[len(cases)] * fv.num_oracles)
    assert fv.code in (0, EINVAL, EVERIFY), (fv.code, fv.reason)
    return list(zip(fv.results, fv.reasons))


def model(orc, inst, a):
    return fm.verify(orc, inst, a["caps"], a["points"], a["openings"], a["alpha"], a["betas"], a["pow_response"], a["indices"], a["proof"])


@pytest.mark.parametrize("row", list(ROWS))
def test_accepted_by_host_device_and_model(pkg, gpu, orc, row):
    c = Case(pkg, gpu, row, seed=300 + len(row))
    try:
        assert c.fv.proof_size() == len(c.proof) == c.inst.lay.total
        alpha, betas, powr, idx = c.challenges
        replay = fs.copy_challenger(pkg, c.before); c.fv.challenges(replay, c.proof)
        assert bytes(replay.state) == bytes(c.after.state)          # qpgpu_fri_prove's transcript, to its end
        assert host(c.fv, c.args()) == (0, "")
        assert device(c.fv, gpu, [c.args()]) == [(0, "")]
        assert model(orc, c.inst, c.args()) is None
    finally:
        c.close()


def test_accepted_under_the_poseidon2_hasher(pkg, gpu, orc):
    prm = pkg.poseidon2_qp_params()
    g2 = pkg.QpGpu(0, hasher=prm)
    orc.select_poseidon2(*prm)
    try:
        c = Case(pkg, g2, "split_ranges", seed=411, hasher=1)
        try:
            assert host(c.fv, c.args()) == (0, "")
            assert device(c.fv, g2, [c.args()]) == [(0, "")]
            assert model(orc, c.inst, c.args()) is None
            broken = bytearray(c.proof); broken[c.inst.lay.queries_pos + 8] ^= 1
            got = device(c.fv, g2, [c.args(proof=bytes(broken))])
            assert got == [host(c.fv, c.args(proof=bytes(broken)))] and got[0][0] == EVERIFY
            # the verifier's hasher must be the context's
            c.fv.verify_many(*many_args(c.fv, [c.args()]), gpu=gpu, cap_counts=[1] * c.fv.num_oracles)
            assert c.fv.code == EINVAL and "hasher" in c.fv.reason
        finally:
            c.close()
    finally:
        orc.select_poseidon()
        g2.close()


@pytest.mark.parametrize("arity", [[4], [3, 2], [1, 2, 3]], ids=lambda a: "-".join(map(str, a)))
def test_caller_chosen_transcript(pkg, gpu, orc, arity):
    """The alpha, betas and indices of test_fri_steps_gpu.py::test_session_assumes_nothing_about_the_transcript, which no
    challenger produced: index 0, the last index and a repeated one."""
    d, rate, cap = 6, 3, 2
    rng = np.random.default_rng(31)
    o = pkg.PolyOracle(gpu, rng.integers(0, P, size=(3, 1 << d), dtype=np.uint64), rate_bits=rate, cap_height=cap)
    point = [int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)]
    betas = [(3, 5), (P - 1, 1), (0x123456789, 0)][:len(arity)]
    indices = [0, (1 << (d + rate)) - 1, 77, 77]
    try:
        with pkg.FriSession(gpu, [o], [(point, [(0, 0, 3)])], (11, 13), arity, rate_bits=rate, cap_height=cap) as s:
            caps = []
            for b in betas:
                caps.append(s.round_commit())
                s.round_fold(b)
            queries = s.open(indices)
            final = s.final_poly()
        fri = b"".join(c.tobytes() for c in caps) + queries + final.tobytes() + bytes(8)
        a = dict(caps=[o.cap()], points=[point], openings=o.eval(point), alpha=(11, 13), betas=betas, pow_response=0, indices=indices, proof=fri)
    finally:
        o.close()
    inst = fm.Instance(d, rate, cap, arity, 4, [(3, False)], [[(0, 0, 3)]])
    with pkg.FriVerifier(d, [(3, False)], [[(0, 0, 3)]], arity, rate_bits=rate, cap_height=cap, proof_of_work_bits=0, num_query_rounds=4) as fv:
        assert host(fv, a) == (0, "") and device(fv, gpu, [a]) == [(0, "")] and model(orc, inst, a) is None
        off = inst.lay.queries_pos + 3 * inst.lay.q_bytes + inst.lay.rounds[-1][0]
        broken = bytearray(fri); broken[off] ^= 1
        b = dict(a, proof=bytes(broken))
        assert host(fv, b)[0] == EVERIFY and device(fv, gpu, [b]) == [host(fv, b)] and fm.reason_of(model(orc, inst, b)) == host(fv, b)[1]


def sweep(c, rng):
    """[(name, changed arguments)]: one bit flipped at a seeded offset of every region of the proof at the first, middle and last
    query (rows, salts, path-length bytes, first and last path node), of every round cap and final coefficient; and one bit in each
    oracle's cap, each opening, each point, alpha, each beta and each index."""
    inst, out = c.inst, []
    alpha, betas, powr, idx = c.challenges
    keep = {0, NQ // 2, NQ - 1}
    for name, pos, n in inst.regions():
        if name == "nonce":
            continue
        if name.startswith("q"):
            q, what = int(name[1:name.index(".")]), name.split(".")[2]
            plen = inst.rows[int(name.split(".")[1][1:])][2] if name.split(".")[1][0] == "o" else inst.lay.rounds[int(name.split(".")[1][1:])][1]
            if q not in keep or (what.startswith("node") and int(what[4:]) not in (0, plen - 1)):
                continue
        at, bit = pos + int(rng.integers(0, n)), int(rng.integers(0, 8))
        if name.startswith("cap"):          # a cap entry no query leads to is bound by the transcript alone: one that a query uses
            r = int(name[3:])
            at = pos + 32 * (idx[int(rng.integers(0, NQ))] >> (sum(inst.arity_bits[:r + 1]) + inst.lay.rounds[r][1])) + int(rng.integers(0, 32))
        broken = bytearray(c.proof); broken[at] ^= 1 << bit
        out.append(("%s+%d.%d" % (name, at - pos, bit), dict(proof=bytes(broken))))

    def flipped(words, i):
        w = np.array(words, dtype=np.uint64).copy()
        w.reshape(-1)[i] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 63)))
        return w

    for o in range(len(c.caps)):
        used = idx[int(rng.integers(0, NQ))] >> inst.rows[o][2]          # the cap entry a query's path leads to
        caps = list(c.caps); caps[o] = flipped(caps[o], 4 * used + int(rng.integers(0, 4)))
        out.append(("cap of oracle %d" % o, dict(caps=caps)))
    for i in range(len(c.openings)):
        out.append(("opening %d" % i, dict(openings=flipped(c.openings, 2 * i + int(rng.integers(0, 2))))))
    for b in range(len(c.points)):
        out.append(("point %d" % b, dict(points=[tuple(int(x) for x in p) for p in flipped(c.points, 2 * b + int(rng.integers(0, 2)))])))
    out.append(("alpha", dict(alpha=tuple(int(x) for x in flipped(alpha, int(rng.integers(0, 2)))))))
    for r in range(len(betas)):
        out.append(("beta %d" % r, dict(betas=[tuple(int(x) for x in p) for p in flipped(betas, 2 * r + int(rng.integers(0, 2)))])))
    L = inst.degree_bits + inst.rate_bits
    for q in range(NQ):
        i2 = list(idx); i2[q] ^= 1 << int(rng.integers(0, L))
        out.append(("index %d" % q, dict(indices=i2)))
    return out


@pytest.mark.parametrize("row", ["copied_leaf", "split_ranges", "one_final_coeff", "plonk_shape"])
def test_tamper_sweep(pkg, gpu, orc, row):
    c = Case(pkg, gpu, row, seed=500 + len(row))
    try:
        cases = sweep(c, np.random.default_rng(77))
        args = [c.args(**change) for _, change in cases]
        dev = device(c.fv, gpu, args)
        kinds = set()
        for (name, _), a, got in zip(cases, args, dev):
            want = host(c.fv, a)
            assert want[0] != 0, name                                 # every one is rejected
            assert got == want, (name, got, want)
            if want[0] == EINVAL:                                     # the flip left a word of the caller's outside the field
                words = [np.asarray(x, dtype=np.uint64).reshape(-1) for x in a["caps"]] + [np.array(a[k], dtype=np.uint64).reshape(-1) for k in ("points", "openings", "alpha", "betas")]
                assert any(int(w.max()) >= P for w in words if w.size), name
                continue
            verdict = model(orc, c.inst, a)
            assert fm.reason_of(verdict) == want[1], (name, verdict, want)
            kinds.add(verdict[0])
        print("%s: %d tampers, verdict kinds %s" % (row, len(cases), sorted(kinds)))
        assert kinds >= {"oracle_path", "round_cont", "round_path", "final"}, kinds
        # the nonce: bound through the challenges only
        lay = c.inst.lay
        broken = bytearray(c.proof); broken[lay.pow_pos] ^= 1
        a = c.args(proof=bytes(broken))
        assert host(c.fv, a) == (0, "") and device(c.fv, gpu, [a]) == [(0, "")]
        alpha, betas, powr, idx = c.fv.challenges(fs.copy_challenger(pkg, c.before), bytes(broken))
        b = c.args(proof=bytes(broken), alpha=alpha, betas=betas, pow_response=powr, indices=idx)
        assert host(c.fv, b)[0] == EVERIFY and device(c.fv, gpu, [b]) == [host(c.fv, b)]
    finally:
        c.close()


def whole_proof_cases(pkg, gpu, orc):
    """(name, pack, Circuit.prove's proof, public inputs): the `rising` schedule on the 2^9 synthetic circuit, the leaf circuit at 2^8."""
    pack, wires, pis = fs.synth_case(pkg, fs.BY_LABEL["rising"], seed=760)
    circ = pkg.Circuit(gpu, pack)
    try:
        yield "synthetic_2^9", pack, circ, circ.prove(wires, pis), pis
    finally:
        circ.close()
    leaf = pkg.leaf.LeafCircuit(min_degree_bits=8)
    cells, values, lpis = leaf.commit(lc.real_inputs(pkg.leaf, depth=3))
    circ = pkg.Circuit(gpu, leaf.pack)
    d_w = gpu.alloc(pkg.pack_header(leaf.pack)["num_wires"] * 256 * 8)
    try:
        circ.generate_witness_partial_dev(cells, values, lpis, d_w)
        yield "leaf_2^8", leaf.pack, circ, circ.prove_dev(d_w, lpis), lpis
    finally:
        d_w.free(scrub=True); circ.close()


def test_whole_proof_agreement(pkg, gpu, orc):
    """The FRI part of whole proofs, untouched and with a tamper of each kind: verdict and reason of the FRI-level device check
    (challenges re-derived from the tampered bytes, as a verifier head would) equal qpgpu_verifier_verify_many_device's, and so do
    the host function's and the model's."""
    for name, pack, circ, proof, pis in whole_proof_cases(pkg, gpu, orc):
        ver = pkg.Verifier(pack, circuit=circ)
        cap = circ.constants_sigmas_cap(int(pack[11]))
        pi_hash = orc.hash_n_to_m(np.array(pis, dtype=np.uint64), 4)
        v = fm.plonk_view(pkg, pack, proof, pi_hash, cap)
        h, lay = v["header"], v["lay"]
        nq = h["num_query_rounds"]
        kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=nq)
        inst = fm.Instance(h["degree_bits"], h["rate_bits"], h["cap_height"], lay.arity_bits, nq, v["oracles"], v["batches"],
                           pow_bits=h["proof_of_work_bits"])
        fv = pkg.FriVerifier(h["degree_bits"], v["oracles"], v["batches"], lay.arity_bits, **kw)
        try:
            idx = fv.challenges(fs.copy_challenger(pkg, v["challenger"]), v["fri"])[3]
            q = nq - 2
            r = len(lay.arity_bits) - 1                                # the last round
            rnd = lay.queries_pos + q * lay.q_bytes + lay.rounds[r][0]
            ab = lay.arity_bits[r]
            within = (idx[q] >> sum(lay.arity_bits[:r])) & ((1 << ab) - 1)
            row2 = lay.queries_pos + q * lay.q_bytes + inst.rows[2][0]
            flips = [None, (row2 + 8, 0), (row2 + 8 * inst.rows[2][1], 7), (row2 + 8 * inst.rows[2][1], 0), (rnd + 16 * within, 0),
                     (rnd + 16 * ((within + 1) % (1 << ab)), 0), (rnd + (16 << ab), 7), (rnd + (16 << ab) + 1, 2), (lay.final_pos, 0), (8, 0)]
            wholes, args = [], []
            for f in flips:
                fri, whole = bytearray(v["fri"]), bytearray(proof)
                if f:
                    fri[f[0]] ^= 1 << f[1]; whole[v["base"] + f[0]] ^= 1 << f[1]
                alpha, betas, powr, ix = fv.challenges(fs.copy_challenger(pkg, v["challenger"]), bytes(fri))
                wholes.append(bytes(whole))
                args.append(dict(caps=v["caps"], points=v["points"], openings=v["openings"], alpha=alpha, betas=betas, pow_response=powr, indices=ix, proof=bytes(fri)))
            ver.verify_many(wholes, gpu=gpu)
            want = list(zip(ver.results, ver.reasons))
            got = device(fv, gpu, args)
            assert got == want, (name, got, want)
            assert want[0] == (0, "") and all(w[0] == EVERIFY for w in want[1:])
            for a, w in zip(args, want):                               # the host function and the model: the same triple
                assert host(fv, a) == w, (name, host(fv, a), w)
                assert fm.reason_of(model(orc, inst, a)) == w[1], (name, model(orc, inst, a), w)
            kinds = {fm.verdict_of(w[1])[0] for w in want[1:]}
            assert kinds >= {"oracle_path", "oracle_plen", "round_cont", "round_path", "round_plen", "pow"}, (name, kinds)
        finally:
            fv.close(); ver.close()


def test_more_proofs_than_one_chunk(pkg, gpu):
    """1 027 proofs (a chunk holds 1 024), the cap shared: the tampered ones on both sides of the boundary are the ones rejected."""
    c = Case(pkg, gpu, "no_rounds", seed=640)
    try:
        n, bad = 1027, {3: "final", 1023: "oracle_path", 1025: "oracle_path"}
        lay = c.inst.lay
        proofs = [c.proof] * n
        for i, kind in bad.items():
            b = bytearray(c.proof); b[lay.final_pos + 16 if kind == "final" else lay.queries_pos + (i % NQ) * lay.q_bytes] ^= 1
            proofs[i] = bytes(b)
        alpha, betas, powr, idx = c.challenges
        c.fv.verify_many([c.caps[0].reshape(-1)], np.tile(np.array(c.points, dtype=np.uint64), (1, n, 1)), np.tile(c.openings, (n, 1, 1)),
                         [alpha] * n, None, [powr] * n, [idx] * n, proofs, gpu=gpu)
        assert [i for i, r in enumerate(c.fv.results) if r] == sorted(bad) and c.fv.code == EVERIFY
        for i, kind in bad.items():
            assert c.fv.results[i] == EVERIFY and fm.verdict_of(c.fv.reasons[i])[:2] == (kind, 0 if kind == "final" else i % NQ), c.fv.reasons[i]
        assert c.fv.reason == "proof 3: " + c.fv.reasons[3]
    finally:
        c.close()


def test_batch_semantics(pkg, gpu, orc):
    """Five proofs over one shared constants-like oracle (cap_counts 1) and two oracles per proof; proofs 1 and 3 tampered."""
    d, rate, cap, arity, shapes, batches, pow_bits = ROWS["split_ranges"]
    nb = 5
    rng = np.random.default_rng(91)
    shared = pkg.PolyOracle(gpu, rng.integers(0, P, size=(5, 1 << d), dtype=np.uint64), rate_bits=rate, cap_height=cap)
    own = [pkg.PolyOracle.commit_batch(gpu, rng.integers(0, P, size=(nb, n, 1 << d), dtype=np.uint64), rate_bits=rate, cap_height=cap,
                                       **(dict(blinding=True, blinding_seed=1234, blinding_stream=i + 1) if b else {}))
           for i, (n, b) in enumerate(shapes[1:])]
    oracles = [shared] + own
    kw = dict(rate_bits=rate, cap_height=cap, proof_of_work_bits=pow_bits, num_query_rounds=NQ)
    fv = pkg.FriVerifier(d, shapes, batches, arity, **kw)
    try:
        points = [rng.integers(0, P, size=(nb, 2), dtype=np.uint64) for _ in batches]
        caps = [shared.cap().reshape(-1)] + [o.cap() for o in own]
        ops = []
        for pts, rg in zip(points, batches):
            for o, f, c in rg:
                ops.append(np.array([shared.eval(pts[b], f, c) for b in range(nb)]) if o == 0 else oracles[o].eval(pts, f, c))
        openings = np.concatenate(ops, axis=1)
        chs = []
        for b in range(nb):
            ch = pkg.Challenger(gpu); ch.observe(np.arange(b, b + 9, dtype=np.uint64)); ch.get()
            chs.append(ch)
        before = [fs.copy_challenger(pkg, ch) for ch in chs]
        proofs = pkg.fri_prove_batch(gpu, oracles, list(zip(points, batches)), chs, arity, **kw)
        chal = [fv.challenges(before[b], proofs[b]) for b in range(nb)]
        lay = fm.Instance(d, rate, cap, arity, NQ, shapes, batches).lay
        p1 = bytearray(proofs[1]); p1[lay.queries_pos + 2 * lay.q_bytes + lay.rounds[1][0] + 3] ^= 4
        p3 = bytearray(proofs[3]); p3[lay.final_pos + 9] ^= 1
        proofs = [proofs[0], bytes(p1), proofs[2], bytes(p3), proofs[4]]
        many = dict(caps=caps, points=np.array(points), openings=openings, alphas=[c[0] for c in chal], betas=[c[1] for c in chal],
                    pow_responses=[c[2] for c in chal], indices=[c[3] for c in chal], proofs=proofs)
        assert fv.verify_many(gpu=gpu, **many) == [True, False, True, False, True]
        assert fv.results == [0, EVERIFY, 0, EVERIFY, 0] and fv.code == EVERIFY
        single = []
        for b in range(nb):
            single.append(host(fv, dict(caps=[caps[0]] + [c[b] for c in caps[1:]], points=[p[b] for p in points], openings=openings[b], alpha=chal[b][0], betas=chal[b][1],
                                        pow_response=chal[b][2], indices=chal[b][3], proof=proofs[b])))
        fv.verify_many(gpu=gpu, **many)
        assert list(zip(fv.results, fv.reasons)) == single
        assert single[1][1] != single[3][1] and fv.reason == "proof 1: " + single[1][1]
        assert fv.verify_many(gpu=None, **many) == [True, False, True, False, True]      # the binding's host loop: the same answers
        # count == 0 is an empty answer; a cap count that is neither 1 nor count names its oracle
        assert fv.verify_many(caps, [], [], [], [], [], [], [], gpu=gpu, cap_counts=[1, 1, 1]) == [] and fv.code == 0
        fv.verify_many(gpu=gpu, cap_counts=[1, 2, nb], **many)
        assert fv.code == EINVAL and "oracle 1" in fv.reason and "batch of 5" in fv.reason
    finally:
        fv.close()
        for o in oracles:
            o.close()
