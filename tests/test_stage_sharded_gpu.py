"""Stage s6 on the shards of coset-sharded oracles (qpgpu_stage_plan_create_sharded; qpgpu_stage_quotient on such a plan): the stage
flow of tests/test_stage_plan_gpu.py with every commitment made by qpgpu_oracle_commit_sharded over G contexts (all of them on
device 0) and the plan made by the new entry, held to the same flow on one context, which is unchanged code that the rest of the
suite pins to the CPU restatement. The quotient chunks and the Z / partial-product columns must be equal word for word, the proof
byte for byte (to the plain flow's and to qpgpu_prove_dev's), and the oracle's verifier must accept it. Exact arithmetic: every
comparison is equality.

The shapes are the smallest that reach each branch: two cosets per shard and one (radix-2 and radix-8 merge), the hash-gate kernels
and the fold sweep on every shard context, the tail chunk with the smallest transforms (M = 2^7), the Poseidon2 gate's constants on
a context that is not the home context, salted sharded oracles, rate_bits above log2 of the quotient degree factor (one working
shard with and without a cut of its own, idle shards behind two and four working ones), and the restated leaf circuit with its
witness made on the device."""
import ctypes

import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_stage_plan_gpu import CIRCUITS, Flow, public_inputs_hash
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
EINVAL, EUNSAT = -1, -4


@pytest.fixture(scope="module")
def ctxs(pkg, gpu):
    """Eight contexts on device 0, the session's first: the home context of every sharded oracle here."""
    more = [pkg.QpGpu(0) for _ in range(7)]
    yield [gpu] + more
    for c in more:
        c.close()


class ShardedPkg:
    """The package as Flow sees it, with every commitment sharded over `gpus` and the plan made by qpgpu_stage_plan_create_sharded:
    Flow's own code then runs the sharded route, statement for statement the plain one."""

    def __init__(self, pkg, gpus):
        self._pkg, self._gpus = pkg, list(gpus)

    def __getattr__(self, name):
        return getattr(self._pkg, name)

    def PolyOracle(self, gpu, polys, **kw):
        assert gpu is self._gpus[0]
        return self._pkg.PolyOracle.commit_sharded(self._gpus, polys, **kw)

    def StagePlan(self, gpu, words, cs_oracle):
        return self._pkg.StagePlan.create_sharded(gpu, words, cs_oracle)


def sharded_flow(pkg, ctxs, orc, pack, G):
    return Flow(ShardedPkg(pkg, ctxs[:G]), ctxs[0], orc, pack)


def synth(pkg, name, rate_bits=None):
    d, kw = CIRCUITS[name]
    pack, wires, pis = pkg.synth_circuit(d, **kw)
    if rate_bits is not None:
        pack = fs.with_schedule(pack, parse_pack(pack)["arity_bits"], rate_bits=rate_bits)
    return pack, wires, pis


def zk_pack(pkg):
    pack, wires, pis = pkg.synth_circuit(8, seed=64, poseidon=True)
    pack = pack.copy(); pack[14] = 1
    return pack, wires, pis


# name -> (how the circuit is made, blinding seed, the shard counts it runs at)
SYNTH = {
    "plain_2p8": (lambda pkg: synth(pkg, "plain_2p8"), 0, (2, 8)),
    "hash_base_sum_2p10": (lambda pkg: synth(pkg, "hash_base_sum_2p10"), 0, (4,)),
    "narrow_2p6": (lambda pkg: synth(pkg, "narrow_2p6"), 0, (4,)),
    "poseidon2_rows_2p8": (lambda pkg: synth(pkg, "poseidon2_rows_2p8"), 0, (2,)),
    "zero_knowledge_2p8": (zk_pack, 4242, (4,)),
    "narrow_2p6_rate4": (lambda pkg: synth(pkg, "narrow_2p6", rate_bits=4), 0, (2, 4, 8)),
    "narrow_2p6_rate5": (lambda pkg: synth(pkg, "narrow_2p6", rate_bits=5), 0, (2,)),
}
CASES = [(name, G) for name, (_, _, gs) in SYNTH.items() for G in gs]


def working_shards(rate_bits, factor, G):
    qbits = (factor - 1).bit_length()
    return max(1, G >> (rate_bits - qbits))


@pytest.fixture(scope="module")
def plain(pkg, gpu, orc):
    """Each circuit once through the plain stage flow and the all-in-one prover; the tests below only compare."""
    cache = {}

    def get(name):
        if name not in cache:
            make, seed, _ = SYNTH[name]
            pack, wires, pis = make(pkg)
            fl = Flow(pkg, gpu, orc, pack)
            circ = pkg.Circuit(gpu, pack)
            d_w = gpu.to_device(wires)
            try:
                got = fl.prove(wires, pis, seed=seed)
                factor = fl.plan.quotient_degree_factor
                assert fl.plan.shards == 1
                if seed:
                    circ.set_blinding_seed(seed)
                all_in_one = circ.prove_dev(d_w, pis)
            finally:
                d_w.free(scrub=True); circ.close(); fl.close()
            cache[name] = dict(pack=pack, wires=wires, pis=pis, seed=seed, got=got, all_in_one=all_in_one, factor=factor)
        return cache[name]
    return get


def test_the_cases_reach_every_number_of_working_shards(pkg, plain):
    seen = set()
    for name, G in CASES:
        r = plain(name)
        seen.add(working_shards(parse_pack(r["pack"])["rate_bits"], r["factor"], G))
    assert seen == {1, 2, 4, 8}, seen


@pytest.mark.parametrize("name,G", CASES, ids=["%s-G%d" % c for c in CASES])
def test_sharded_flow_equals_the_plain_flow(pkg, ctxs, orc, plain, name, G):
    r = plain(name)
    fl = sharded_flow(pkg, ctxs, orc, r["pack"], G)
    try:
        assert fl.plan.shards == G and fl.plan.max_batch == 1 and fl.o_cs.shards == G
        assert fl.plan.quotient_degree_factor == r["factor"]
        proof, zs, q = fl.prove(r["wires"], r["pis"], seed=r["seed"])
    finally:
        fl.close()
    want_proof, want_zs, want_q = r["got"]
    assert np.array_equal(zs, want_zs), "the Z / partial-product columns differ from the plain flow's"
    assert q.shape == want_q.shape
    assert np.array_equal(q, want_q), "the quotient chunks differ from the plain flow's at %s" % (np.argwhere(q != want_q)[:4].tolist(),)
    assert proof == want_proof, "the sharded flow's proof differs from the plain flow's"
    assert proof == r["all_in_one"], "the sharded flow's proof differs from qpgpu_prove_dev's"
    oc = OracleCircuit(orc, r["pack"])
    try:
        assert oc.verify(proof) == 0
    finally:
        oc.close()


@pytest.mark.parametrize("case", ["dummy"])
def test_leaf_circuit_with_a_device_witness(pkg, ctxs, orc, case):
    """The restated leaf circuit at its own 2^8 rows over two contexts, the witness made on the device: a real gate list end to end."""
    gpu = ctxs[0]
    leaf = pkg.leaf.LeafCircuit(min_degree_bits=8)
    hdr = pkg.pack_header(leaf.pack)
    assert hdr["degree_bits"] == 8
    cells, values, pis = leaf.commit(lc.dummy_inputs(pkg.leaf))
    circ = pkg.Circuit(gpu, leaf.pack)
    ver = pkg.Verifier(leaf.pack, circuit=circ)
    d_w = gpu.alloc(hdr["num_wires"] * 256 * 8)
    plain_fl = Flow(pkg, gpu, orc, leaf.pack)
    fl = None
    try:
        fl = sharded_flow(pkg, ctxs, orc, leaf.pack, 2)
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        want = circ.prove_dev(d_w, pis)
        assert fl.plan.fused_selected == plain_fl.plan.fused_selected == circ.quotient_info()[1]
        want_proof, want_zs, want_q = plain_fl.prove(None, pis, d_wires=d_w)
        got, zs, q = fl.prove(None, pis, d_wires=d_w)
        assert np.array_equal(zs, want_zs) and np.array_equal(q, want_q)
        assert got == want_proof == want
        assert ver.verify(got)
        oc = OracleCircuit(orc, leaf.pack)
        try:
            assert oc.verify(got) == 0
        finally:
            oc.close()
    finally:
        if fl is not None:
            fl.close()
        plain_fl.close(); d_w.free(scrub=True); ver.close(); circ.close()


def test_unsatisfied_witness_is_refused_and_the_plan_survives(pkg, ctxs, orc):
    gpu = ctxs[0]
    pack, wires, pis = pkg.synth_circuit(8, seed=61, poseidon=True, base_sum=True)
    bad = wires.copy(); bad[3, 20] = (int(bad[3, 20]) + 1) % P          # arithmetic output of op 0 on row 20
    plain_fl = Flow(pkg, gpu, orc, pack)
    fl = None
    try:
        fl = sharded_flow(pkg, ctxs, orc, pack, 4)
        with pytest.raises(pkg.QpGpuError) as e_plain:
            plain_fl.prove(bad, pis)
        with pytest.raises(pkg.QpGpuError) as e_sharded:
            fl.prove(bad, pis)
        assert e_plain.value.code == e_sharded.value.code == EUNSAT
        assert str(e_sharded.value) == str(e_plain.value) and "row 20" in str(e_sharded.value)
        # the same plan, the good witness: the right chunks and the plain flow's proof
        want = plain_fl.prove(wires, pis)
        got = fl.prove(wires, pis)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and got[0] == want[0]
    finally:
        if fl is not None:
            fl.close()
        plain_fl.close()


def test_refusals(pkg, ctxs, orc):
    gpu, lib = ctxs[0], ctxs[0].lib
    G = 4
    pack, wires, pis = pkg.synth_circuit(6, seed=63, num_wires=24, num_routed=16, num_public_inputs=3)
    h = parse_pack(pack)
    cs, n = h["constants_sigmas"], 64
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])

    def refused(make, *words):
        with pytest.raises(pkg.QpGpuError) as e:
            make()
        assert e.value.code == EINVAL and all(w in str(e.value) for w in words), str(e.value)

    # the plan: a plain cs_oracle, a context that is not the home context, NULL arguments; a sharded oracle to a plain plan
    o_plain = pkg.PolyOracle(gpu, cs, **kw)
    o_cs = gpu.commit_sharded(ctxs[:G], cs, **kw)
    opened = [o_plain, o_cs]
    plan = plain_plan = None
    try:
        refused(lambda: pkg.StagePlan.create_sharded(gpu, pack, o_plain), "stage_plan_create_sharded: cs_oracle is not sharded", "qpgpu_stage_plan_create")
        refused(lambda: pkg.StagePlan.create_sharded(ctxs[1], pack, o_cs), "stage_plan_create_sharded: cs_oracle", "home context")
        refused(lambda: pkg.StagePlan(gpu, pack, o_cs), "stage_plan_create: cs_oracle is sharded over 4 contexts: sharded oracles are not taken here yet")
        hp = ctypes.c_void_p(0x1234)
        err = ctypes.create_string_buffer(pkg.binding.STAGE_ERR_CAP)
        pw = np.ascontiguousarray(pack, dtype=np.uint64)
        assert lib.qpgpu_stage_plan_create_sharded(gpu.ctx, pw.ctypes.data, pw.size, o_cs.h, None, err) == EINVAL
        assert lib.qpgpu_stage_plan_create_sharded(gpu.ctx, None, 0, o_cs.h, ctypes.byref(hp), err) == EINVAL and hp.value is None
        assert lib.qpgpu_stage_plan_create_sharded(None, pw.ctypes.data, pw.size, o_cs.h, ctypes.byref(hp), err) == EINVAL and b"null context" in err.value
        assert lib.qpgpu_stage_plan_create_sharded(gpu.ctx, pw.ctypes.data, pw.size, None, ctypes.byref(hp), err) == EINVAL and b"null cs_oracle" in err.value
        # the header goes first: a length that is neither form is refused before the oracle is looked at
        assert lib.qpgpu_stage_plan_create_sharded(gpu.ctx, pw.ctypes.data, pw.size - 5, o_plain.h, ctypes.byref(hp), err) == EINVAL
        assert b"length fits neither" in err.value

        plan = pkg.StagePlan.create_sharded(gpu, pack, o_cs)
        plain_plan = pkg.StagePlan(gpu, pack, o_plain)
        assert plan.shards == G and plain_plan.shards == 1 and lib.qpgpu_stage_plan_shards(None) == 0
        ones = [1] * plan.num_challenges
        d_zs = plan.partial_products(wires, ones, ones)
        want_zs = plain_plan.partial_products(wires, ones, ones)
        assert np.array_equal(d_zs.download(), want_zs.download())
        o_w = gpu.commit_sharded(ctxs[:G], wires, **kw); opened.append(o_w)
        o_zs = gpu.commit_sharded(ctxs[:G], (d_zs, plan.num_zs_pp, n), **kw); opened.append(o_zs)
        o_w_plain = pkg.PolyOracle(gpu, wires, **kw); opened.append(o_w_plain)
        o_zs_plain = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), **kw); opened.append(o_zs_plain)
        o_w_half = gpu.commit_sharded(ctxs[:G // 2], wires, **kw); opened.append(o_w_half)
        o_w_swapped = gpu.commit_sharded([ctxs[0], ctxs[2], ctxs[1], ctxs[3]], wires, **kw); opened.append(o_w_swapped)
        o_w_other_home = ctxs[1].commit_sharded([ctxs[1], ctxs[0], ctxs[2], ctxs[3]], wires, **kw); opened.append(o_w_other_home)
        o_w_short = gpu.commit_sharded(ctxs[:G], wires[:-1], **kw); opened.append(o_w_short)

        marker = np.full(plan.num_quotient * n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        d_out = gpu.to_device(marker)
        args = [np.array(ones, dtype=np.uint64) for _ in range(3)] + [np.zeros(4, dtype=np.uint64)]

        def raw(pl, w, z):
            rc = lib.qpgpu_stage_quotient(pl.h, w.h, z.h, *[a.ctypes.data for a in args], d_out.ptr)
            return rc, gpu.last_error()

        for w, z, words in ((o_w_plain, o_zs, ("stage_quotient: wires_oracle is not sharded",)),
                            (o_w, o_zs_plain, ("stage_quotient: zs_pp_oracle is not sharded",)),
                            (o_w_half, o_zs, ("wires_oracle is sharded over 2 contexts", "cs_oracle over 4")),
                            (o_w_swapped, o_zs, ("wires_oracle runs shard 1 on another context",)),
                            (o_w_other_home, o_zs, ("wires_oracle has another home context",)),
                            (o_w_short, o_zs, ("wires_oracle has 23 polynomials, the circuit needs 24",)),
                            (o_w, o_w, ("zs_pp_oracle has 24 polynomials",))):
            rc, msg = raw(plan, w, z)
            assert rc == EINVAL and all(s in msg for s in words), msg
            assert np.array_equal(d_out.download(), marker), "a refused call wrote d_out"
        # a sharded oracle to a plain plan: today's words
        rc, msg = raw(plain_plan, o_w, o_zs_plain)
        assert rc == EINVAL and "stage_quotient: wires_oracle is sharded over 4 contexts: sharded oracles are not taken here yet" in msg
        rc, msg = raw(plain_plan, o_w_plain, o_zs)
        assert rc == EINVAL and "stage_quotient: zs_pp_oracle is sharded over 4 contexts: sharded oracles are not taken here yet" in msg
        assert np.array_equal(d_out.download(), marker)
        # the lockstep entries on a sharded plan
        refused(lambda: plan.partial_products_batch([wires], [ones], [ones]), "stage_partial_products_batch", "sharded over 4 contexts", "one proof")
        rc = lib.qpgpu_stage_quotient_batch(plan.h, o_w.h, o_zs.h, 1, *[a.ctypes.data for a in args], d_out.ptr)
        assert rc == EINVAL and "stage_quotient_batch" in gpu.last_error() and "a sharded plan takes one proof" in gpu.last_error()
        assert np.array_equal(d_out.download(), marker)
        # NULL arguments
        assert lib.qpgpu_stage_quotient(plan.h, o_w.h, o_zs.h, None, None, None, None, None) == EINVAL
        assert lib.qpgpu_stage_quotient(plan.h, None, o_zs.h, *[a.ctypes.data for a in args], d_out.ptr) == EINVAL
        assert lib.qpgpu_stage_quotient(None, o_w.h, o_zs.h, *[a.ctypes.data for a in args], d_out.ptr) == EINVAL
        assert lib.qpgpu_stage_partial_products(plan.h, None, 0, None, None, None) == EINVAL
        assert np.array_equal(d_out.download(), marker)
        # and the plan still works: with the public-input hash in place the good call answers as the plain plan answers, and writes
        # the same words
        args[3] = public_inputs_hash(pkg, gpu, pis)
        rc_s, msg_s = raw(plan, o_w, o_zs)
        got = d_out.download().copy()
        d_out.upload(marker)
        rc_p, msg_p = raw(plain_plan, o_w_plain, o_zs_plain)
        assert rc_s == rc_p and (rc_s == 0 or msg_s == msg_p)
        if rc_s == 0:
            assert np.array_equal(got, d_out.download())
        d_out.free(scrub=True); d_zs.free(scrub=True); want_zs.free(scrub=True)
    finally:
        if plan is not None:
            plan.close()
        if plain_plan is not None:
            plain_plan.close()
        for o in opened[::-1]:
            o.close()


def test_free_leaves_no_residue_on_any_shard(pkg, ctxs, orc):
    """After a sharded quotient, qpgpu_stage_plan_free and the oracles' close: no word of the witness, of the wire LDE or of the
    quotient chunks is left in what the plan and the oracles owned, on any shard context. Before that the same scan finds the witness in
    the plan's workspace on the home context (the witness check's wire values) and the wire LDE in every shard's oracle block. The needles
    are words above 2^32, as the scan requires; the wire LDE is read on a context that is no shard's (a read passes the reader's
    bounce buffer)."""
    G = 4
    gpu, outside = ctxs[0], ctxs[7]
    pack, wires, pis = pkg.synth_circuit(8, seed=64, poseidon=True)
    h = parse_pack(pack)
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    consts = set(int(v) for v in np.asarray(h["constants_sigmas"]).ravel())

    def words_of(vals, count):
        out = list(dict.fromkeys(int(v) for v in vals if int(v) >= 1 << 32 and int(v) not in consts))[:count]
        assert len(out) == count
        return np.array(out, dtype=np.uint64)

    o = pkg.PolyOracle(outside, wires, **kw)
    lde = o.read(lde=True)
    o.close()
    N = lde.shape[1]
    witness = words_of(wires[:, 3:].ravel(), 8)
    lde_words = [words_of(lde[5:, g * (N // G) + 1: (g + 1) * (N // G)].ravel(), 4) for g in range(G)]     # four of each shard's leaves
    regions = ["stage-plan", "oracle"]

    class Probe(ShardedPkg):
        """Scans while the plan and the oracles are alive: right after the quotient."""
        found = None

        def PolyOracle(self, gpu_, polys, **kw_):
            if kw_.get("coeffs") and Probe.found is None:                # the quotient commitment: the quotient stage has just run
                Probe.found = ([c.residue_scan(witness, regions=["stage-plan"])[0] for c in ctxs[:G]],
                               [ctxs[g].residue_scan(lde_words[g], regions=["oracle"])[0] for g in range(G)])
            return ShardedPkg.PolyOracle(self, gpu_, polys, **kw_)

    fl = Flow(Probe(pkg, ctxs[:G]), gpu, orc, pack)
    try:
        _, _, q = fl.prove(wires, pis)
    finally:
        fl.close()
    in_plan, in_oracle = Probe.found
    assert in_plan[0] >= witness.size, "the home context's plan workspace held the witness check's wire values"
    assert all(x >= 4 for x in in_oracle), in_oracle
    for needles in (np.concatenate([witness, words_of(q.ravel(), 8)]), np.concatenate(lde_words)):      # a scan takes 16 needles
        for g in range(G):
            hits, first, nbytes = ctxs[g].residue_scan(needles, regions=regions)
            assert hits == 0 and nbytes >= 0, (g, first)
