"""Stage-level C ABI, the two gate-dependent stages (qpgpu_stage_plan_*, qpgpu_stage_partial_products, qpgpu_stage_quotient): the
stage flow of tests/test_staged_gpu.py with NOTHING taken from the CPU oracle's stage trace. The Z / partial-product columns and
the quotient chunks come from the new entries, stay on the device, and are committed from there; the proof must equal the
oracle's (or qpgpu_prove_dev's) byte for byte, and each stage's output must equal the oracle's trace word for word, so that a
byte mismatch names its stage. Exact arithmetic: no tolerance anywhere. Shapes: the ones the existing staged test uses (the
smallest at which each kernel family is reached: plain gates at 2^8 rows, hash and base-sum gates at 2^10, the narrow circuit with
a tail chunk at 2^6), Poseidon2-gate rows at 2^8, a zero-knowledge pack at 2^8 (salted oracles), and the restated leaf circuit at
its own 2^8 rows with the witness made on the device."""
import numpy as np
import pytest

import leaf_cases as lc
from oracle_binding import OracleCircuit
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001

CIRCUITS = {
    "plain_2p8": (8, dict(seed=61)),
    "hash_base_sum_2p10": (10, dict(seed=62, poseidon=True, base_sum=True)),
    "narrow_2p6": (6, dict(seed=63, num_wires=24, num_routed=16, num_public_inputs=3)),
    "poseidon2_rows_2p8": (8, dict(seed=67, poseidon=True, base_sum=True, poseidon2=True)),
}


def public_inputs_hash(pkg, gpu, pis):
    """hash_no_pad of the public inputs under the context's hasher, through the library's duplex challenger: observing them and
    squeezing once leaves the sponge as the overwrite-mode hash leaves it; the digest is its first four words."""
    pis = np.asarray(pis, dtype=np.uint64)
    if pis.size == 0:
        return np.zeros(4, dtype=np.uint64)
    ch = pkg.Challenger(gpu)
    ch.observe(pis % np.uint64(P))
    ch.get()
    return np.array(list(ch.state.sponge_state)[:4], dtype=np.uint64)


class Flow:
    """The constants/sigmas oracle and the stage plan of one circuit, and the prove() flow over them."""

    def __init__(self, pkg, gpu, orc, pack, words=None):
        self.pkg, self.gpu, self.orc, self.pack = pkg, gpu, orc, pack
        self.h = parse_pack(pack)
        self.kw = dict(rate_bits=self.h["rate_bits"], cap_height=self.h["cap_height"])
        self.o_cs = pkg.PolyOracle(gpu, self.h["constants_sigmas"], **self.kw)
        try:
            self.plan = pkg.StagePlan(gpu, pack if words is None else words, self.o_cs)
        except Exception:
            self.o_cs.close()
            raise

    def close(self):
        self.plan.close()
        self.o_cs.close()

    def prove(self, wires, pis, seed=0, d_wires=None):
        """wires: host matrix; d_wires: the same matrix on the device (then s5 and the wire commitment read it there).
        Returns (proof bytes, zs_pp values [cols, n], quotient chunk coefficients [cols, n])."""
        pkg, gpu, h, plan = self.pkg, self.gpu, self.h, self.plan
        d, nch, zk = h["degree_bits"], h["num_challenges"], bool(h["zero_knowledge"])
        n = 1 << d
        assert (plan.degree_bits, plan.num_challenges, plan.num_partial_products, plan.quotient_degree_factor) == \
            (d, nch, h["num_partial_products"], h["quotient_degree_factor"])
        zkw = dict(blinding=zk, blinding_seed=seed)
        oracles, bufs = [self.o_cs], []
        try:
            ch = pkg.Challenger(gpu)
            pih = public_inputs_hash(pkg, gpu, pis)
            src = wires if d_wires is None else (d_wires, h["num_wires"], n)
            o_w = pkg.PolyOracle(gpu, src, blinding_stream=1, **self.kw, **zkw); oracles.append(o_w)
            ch.observe(h["circuit_digest"]); ch.observe(pih); ch.observe(o_w.cap())
            betas, gammas = ch.get_n(nch), ch.get_n(nch)
            d_zs = plan.partial_products(wires if d_wires is None else d_wires, betas, gammas); bufs.append(d_zs)
            zs_vals = d_zs.download().reshape(-1, n)
            o_zs = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), blinding_stream=2, **self.kw, **zkw); oracles.append(o_zs)
            ch.observe(o_zs.cap())
            alphas = ch.get_n(nch)
            d_q = plan.quotient(o_w, o_zs, betas, gammas, alphas, pih); bufs.append(d_q)
            q_coeffs = d_q.download().reshape(-1, n)
            o_q = pkg.PolyOracle(gpu, (d_q, plan.num_quotient, n), coeffs=True, blinding_stream=3, **self.kw, **zkw); oracles.append(o_q)
            ch.observe(o_q.cap())
            zeta = ch.get_n(2)
            g = self.orc.root(d)
            g_zeta = [self.orc.mul(zeta[0], g), self.orc.mul(zeta[1], g)]
            opens = [o.eval(zeta) for o in oracles]
            zs_next = o_zs.eval(g_zeta, 0, nch)
            ch.observe(np.concatenate(opens)); ch.observe(zs_next)
            fri = pkg.fri_prove(gpu, oracles, [(zeta, [(i, 0, o.num_polys) for i, o in enumerate(oracles)]), (g_zeta, [(2, 0, nch)])],
                                ch, h["arity_bits"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"], **self.kw)
            zs_open = opens[2]
            parts = [o_w.cap(), o_zs.cap(), o_q.cap(), opens[0], opens[1], zs_open[:nch], zs_next, zs_open[nch:], opens[3]]
            proof = b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in parts) + fri + \
                (np.asarray(pis, dtype=np.uint64) % np.uint64(P)).tobytes()
            return proof, zs_vals, q_coeffs
        finally:
            for o in oracles[1:]:
                o.close()
            for b in bufs:
                b.free(scrub=True)


@pytest.fixture(scope="module")
def runs(pkg, gpu, orc):
    """Each circuit through the oracle (proof and stage trace) and through the stage flow, once; the tests below only compare."""
    cache = {}

    def get(name):
        if name not in cache:
            d, kw = CIRCUITS[name]
            pack, wires, pis = pkg.synth_circuit(d, **kw)
            oc = OracleCircuit(orc, pack)
            want = oc.prove(wires, pis)                       # fills the stage trace (one trace for the whole oracle: read it now)
            trace = {k: oc.trace(k).copy() for k in ("zs_pp_values", "quotient_chunk_coeffs", "pi_hash")}
            fl = Flow(pkg, gpu, orc, pack)
            try:
                got = fl.prove(wires, pis)
            finally:
                fl.close()
            cache[name] = dict(pack=pack, wires=wires, pis=pis, want=want, trace=trace, got=got, verdict=oc.verify(got[0]))
            oc.close()
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_each_stage_equals_the_oracle_trace(pkg, gpu, runs, name):
    r = runs(name)
    n = 1 << CIRCUITS[name][0]
    assert np.array_equal(public_inputs_hash(pkg, gpu, r["pis"]), r["trace"]["pi_hash"])
    _, zs, q = r["got"]
    assert np.array_equal(zs, r["trace"]["zs_pp_values"].reshape(-1, n)), "qpgpu_stage_partial_products differs from the oracle's zs_pp_values"
    assert np.array_equal(q, r["trace"]["quotient_chunk_coeffs"].reshape(-1, n)), "qpgpu_stage_quotient differs from the oracle's quotient_chunk_coeffs"


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_whole_flow_reproduces_the_proof(runs, name):
    r = runs(name)
    got, want = r["got"][0], r["want"]
    assert len(got) == len(want)
    assert got == want, f"staged proof differs at byte {next(i for i in range(len(got)) if got[i] != want[i])}"
    assert r["verdict"] == 0


def test_zero_knowledge_flow_reaches_the_salted_oracles(pkg, gpu, orc):
    pack, wires, pis = pkg.synth_circuit(8, seed=64, poseidon=True)
    pack = pack.copy(); pack[14] = 1
    oc = OracleCircuit(orc, pack)
    want = oc.prove(wires, pis, seed=4242)
    trace = {k: oc.trace(k).copy() for k in ("zs_pp_values", "quotient_chunk_coeffs")}
    fl = Flow(pkg, gpu, orc, pack)
    try:
        got, zs, q = fl.prove(wires, pis, seed=4242)
        assert np.array_equal(zs, trace["zs_pp_values"].reshape(-1, 256))
        assert np.array_equal(q, trace["quotient_chunk_coeffs"].reshape(-1, 256))
        assert got == want and oc.verify(got) == 0
    finally:
        fl.close(); oc.close()


@pytest.fixture(scope="module")
def leaf(pkg):
    return pkg.leaf.LeafCircuit(min_degree_bits=8)


@pytest.mark.parametrize("case", ["dummy", "spend"])
def test_leaf_circuit_with_a_device_witness(pkg, gpu, orc, leaf, case):
    """The restated leaf circuit at its own 2^8 rows: the witness is made on the device (qpgpu_generate_witness_partial_dev) and
    never leaves it; the stage flow's proof equals qpgpu_prove_dev's for that witness and the host verifier accepts it."""
    L = pkg.leaf
    hdr = pkg.pack_header(leaf.pack)
    assert hdr["degree_bits"] == 8
    x = lc.dummy_inputs(L) if case == "dummy" else lc.real_inputs(L, depth=3)
    cells, values, pis = leaf.commit(x)
    circ = pkg.Circuit(gpu, leaf.pack)
    ver = pkg.Verifier(leaf.pack, circuit=circ)
    d_w = gpu.alloc(hdr["num_wires"] * 256 * 8)
    fl = Flow(pkg, gpu, orc, leaf.pack)
    try:
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        want = circ.prove_dev(d_w, pis)
        assert fl.plan.fused_selected == circ.quotient_info()[1]
        got, _, _ = fl.prove(None, pis, d_wires=d_w)
        assert got == want
        assert ver.verify(got)
    finally:
        fl.close(); d_w.free(scrub=True); ver.close(); circ.close()


@pytest.mark.parametrize("name", ["plain_2p8", "poseidon2_rows_2p8"])
def test_header_only_words_give_the_same_plan(pkg, gpu, orc, runs, name):
    """The pack with its constants/sigmas value block cut out (the P2GL1 trailer kept, where there is one)."""
    r = runs(name)
    short = pkg.stage_header_words(r["pack"])
    h = parse_pack(r["pack"])
    assert short.size == r["pack"].size - h["constants_sigmas"].size
    fl = Flow(pkg, gpu, orc, r["pack"], words=short)
    try:
        got, zs, q = fl.prove(r["wires"], r["pis"])
    finally:
        fl.close()
    assert np.array_equal(zs, r["got"][1]) and np.array_equal(q, r["got"][2]) and got == r["got"][0]


def test_unsatisfied_witness_is_refused_and_the_plan_survives(pkg, gpu, orc):
    pack, wires, pis = pkg.synth_circuit(8, seed=61, poseidon=True, base_sum=True)
    bad = wires.copy(); bad[3, 20] = (int(bad[3, 20]) + 1) % P          # arithmetic output of op 0 on row 20
    circ = pkg.Circuit(gpu, pack)
    fl = Flow(pkg, gpu, orc, pack)
    try:
        circ.set_witness_check(True)
        d_bad = gpu.to_device(bad)
        with pytest.raises(pkg.QpGpuError) as e_all:
            circ.prove_dev(d_bad, pis)
        d_bad.free(scrub=True)
        with pytest.raises(pkg.QpGpuError) as e_stage:
            fl.prove(bad, pis)
        assert e_all.value.code == e_stage.value.code == -4
        assert str(e_stage.value) == str(e_all.value) and "row 20" in str(e_stage.value)
        # the same plan, the good witness: the flow succeeds and its proof is the all-in-one prover's
        assert fl.prove(wires, pis)[0] == circ.prove(wires, pis)
    finally:
        fl.close(); circ.close()


def test_argument_errors_name_the_argument(pkg, gpu):
    pack, wires, pis = pkg.synth_circuit(6, seed=63, num_wires=24, num_routed=16, num_public_inputs=3)
    h = parse_pack(pack)
    cs, n = h["constants_sigmas"], 64
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])

    def refused(make, *names):
        with pytest.raises(pkg.QpGpuError) as e:
            make()
        assert e.value.code == -1 and all(s in str(e.value) for s in names), str(e.value)

    def plan_with(o, words=pack):
        try:
            pkg.StagePlan(gpu, words, o).close()
        finally:
            if o is not None:
                o.close()
    # the constants/sigmas oracle: a column short, another degree, another rate, blinded
    refused(lambda: plan_with(pkg.PolyOracle(gpu, cs[:-1], **kw)), "cs_oracle", "polynomials")
    refused(lambda: plan_with(pkg.PolyOracle(gpu, np.concatenate([cs, cs], axis=1), **kw)), "cs_oracle", "degree_bits")
    refused(lambda: plan_with(pkg.PolyOracle(gpu, cs, rate_bits=h["rate_bits"] - 1, cap_height=h["cap_height"])), "cs_oracle", "rate_bits")
    refused(lambda: plan_with(pkg.PolyOracle(gpu, cs, blinding=True, blinding_seed=7, **kw)), "cs_oracle", "blinded")
    # words: a length that is neither form; a type-14 gate list without its layout trailer (the loader's message)
    refused(lambda: plan_with(pkg.PolyOracle(gpu, cs, **kw), pack[:-5]), "length fits neither")
    p2pack = pkg.synth_circuit(8, seed=67, poseidon=True, base_sum=True, poseidon2=True)[0]
    cut = p2pack[:p2pack.size - 12]                                                   # "P2GL1", 10, ten layout words: the last trailer
    assert int(p2pack[-12]) == 0x000000314C473250
    with pytest.raises(pkg.QpGpuError) as e_load:
        pkg.Circuit(gpu, cut)
    reason = str(e_load.value).split("circuit_load: ")[1]
    assert "without a wire-layout trailer" in reason
    refused(lambda: plan_with(None, cut), reason)
    refused(lambda: plan_with(None, pkg.stage_header_words(p2pack)[:-12]), reason)
    # the stage entries: wrong oracles in the wires and Z / partial-products places; a good call follows on the same plan
    o_cs = pkg.PolyOracle(gpu, cs, **kw)
    plan = pkg.StagePlan(gpu, pack, o_cs)
    o_w = pkg.PolyOracle(gpu, wires, **kw)
    ones = [1] * plan.num_challenges
    d_zs = plan.partial_products(wires, ones, ones)
    o_zs = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), **kw)
    try:
        short_w = pkg.PolyOracle(gpu, wires[:-1], **kw)
        refused(lambda: plan.quotient(short_w, o_zs, ones, ones, ones, [0] * 4), "wires_oracle", "polynomials")
        short_w.close()
        refused(lambda: plan.quotient(o_w, o_w, ones, ones, ones, [0] * 4), "zs_pp_oracle", "polynomials")
        low_rate = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), rate_bits=h["rate_bits"] - 1, cap_height=h["cap_height"])
        refused(lambda: plan.quotient(o_w, low_rate, ones, ones, ones, [0] * 4), "zs_pp_oracle", "rate_bits")
        low_rate.close()
        assert gpu.lib.qpgpu_stage_quotient(plan.h, o_w.h, o_zs.h, None, None, None, None, None) == -1
        assert gpu.lib.qpgpu_stage_partial_products(plan.h, None, 0, None, None, None) == -1
    finally:
        o_zs.close(); d_zs.free(scrub=True); o_w.close(); plan.close(); o_cs.close()


def test_stage_example_in_c(tmp_path):
    """examples/stage_prove_example.c: the whole stage flow from plain C at 2^8 rows; it compares its bytes with qpgpu_prove's itself and
    shows the refusal of a broken witness."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "qpgpu_stage_prove_example_gpu")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "stage_prove_example.c"),
                           "-L", os.path.join(root, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(root, "qp-zk-circuits_amd"), "-o", out])
    res = subprocess.run([out, "8"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "gate constraints fail at row 20" in res.stdout and "staged flow == qpgpu_prove" in res.stdout
