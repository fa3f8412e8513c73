"""Stage-level C ABI for lockstep batches (qpgpu_oracle_commit_batch, _eval_batch, _open_batch, qpgpu_stage_plan_create_batch,
qpgpu_stage_partial_products_batch, qpgpu_stage_quotient_batch, qpgpu_fri_prove_batch, qpgpu_fri_begin_batch, qpgpu_fri_grind_batch):
one call per stage for `batch` proofs of a circuit, the transcripts kept by the caller. Proof b of a batch must equal the CPU
restatement's proof of witness b and qpgpu_prove_batch_dev's, byte for byte; every batched call must equal `batch` calls of the
single-proof entry word for word. Exact arithmetic: every comparison is equality. Shapes are the smallest at which a proof
stride can be wrong: 2^6 .. 2^10 rows, batches of 2 and 3 (an odd batch with more than two proofs catches a stride applied once
too few or computed from the wrong width), three or four query indices in the step tests."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fri_schedules as fs
import test_fri_steps_gpu as steps
import test_stage_plan_gpu as sp
from oracle_binding import OracleCircuit
from test_batch_gpu import _witnesses
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


class BatchFlow(sp.Flow):
    """sp.Flow with a plan for max_batch proofs, and the prove() flow for a lockstep batch over it."""

    def __init__(self, pkg, gpu, orc, pack, max_batch):
        self.pkg, self.gpu, self.orc, self.pack = pkg, gpu, orc, pack
        self.h = parse_pack(pack)
        self.kw = dict(rate_bits=self.h["rate_bits"], cap_height=self.h["cap_height"])
        self.o_cs = pkg.PolyOracle(gpu, self.h["constants_sigmas"], **self.kw)
        try:
            self.plan = pkg.StagePlan(gpu, pack, self.o_cs, max_batch=max_batch)
        except Exception:
            self.o_cs.close()
            raise

    def prove_batch(self, ws, pis, seed=0, keep=None):
        """ws: host witness matrices, one per proof. Returns (list of proof bytes, zs_pp values [B, cols, n], quotient chunk
        coefficients [B, cols, n]). keep: a dict that receives the three committed oracles' caps."""
        pkg, gpu, h, plan = self.pkg, self.gpu, self.h, self.plan
        d, nch, zk = h["degree_bits"], h["num_challenges"], bool(h["zero_knowledge"])
        n, B = 1 << d, len(ws)
        zkw = dict(blinding=zk, blinding_seed=seed)
        oracles, bufs = [self.o_cs], []
        try:
            chs = [pkg.Challenger(gpu) for _ in range(B)]
            pihs = [sp.public_inputs_hash(pkg, gpu, p) for p in pis]
            o_w = pkg.PolyOracle.commit_batch(gpu, ws, blinding_stream=1, **self.kw, **zkw); oracles.append(o_w)
            betas, gammas = [], []
            for b, ch in enumerate(chs):
                ch.observe(h["circuit_digest"]); ch.observe(pihs[b]); ch.observe(o_w.cap()[b])
                betas.append(ch.get_n(nch)); gammas.append(ch.get_n(nch))
            d_zs = plan.partial_products_batch(ws, betas, gammas); bufs.append(d_zs)
            zs_vals = d_zs.download().reshape(B, -1, n)
            o_zs = pkg.PolyOracle.commit_batch(gpu, [(d_zs.ptr + b * plan.num_zs_pp * n * 8, plan.num_zs_pp, n) for b in range(B)],
                                               blinding_stream=2, **self.kw, **zkw); oracles.append(o_zs)
            alphas = []
            for b, ch in enumerate(chs):
                ch.observe(o_zs.cap()[b]); alphas.append(ch.get_n(nch))
            d_q = plan.quotient_batch(o_w, o_zs, B, betas, gammas, alphas, pihs); bufs.append(d_q)
            q_coeffs = d_q.download().reshape(B, -1, n)
            o_q = pkg.PolyOracle.commit_batch(gpu, [(d_q.ptr + b * plan.num_quotient * n * 8, plan.num_quotient, n) for b in range(B)],
                                              coeffs=True, blinding_stream=3, **self.kw, **zkw); oracles.append(o_q)
            g = self.orc.root(d)
            zetas, g_zetas = [], []
            for b, ch in enumerate(chs):
                ch.observe(o_q.cap()[b])
                z = ch.get_n(2)
                zetas.append(z); g_zetas.append([self.orc.mul(z[0], g), self.orc.mul(z[1], g)])
            opens = [np.stack([self.o_cs.eval(z) for z in zetas])] + [o.eval(zetas) for o in oracles[1:]]      # [B, cols, 2] each
            zs_next = o_zs.eval(g_zetas, 0, nch)
            for b, ch in enumerate(chs):
                ch.observe(np.concatenate([x[b] for x in opens])); ch.observe(zs_next[b])
            fri = pkg.fri_prove_batch(gpu, oracles, [(zetas, [(i, 0, o.num_polys) for i, o in enumerate(oracles)]), (g_zetas, [(2, 0, nch)])],
                                      chs, h["arity_bits"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"],
                                      **self.kw)
            caps = [o_w.cap(), o_zs.cap(), o_q.cap()]
            if keep is not None:
                keep["caps"] = caps
            proofs = []
            for b in range(B):
                zs_open = opens[2][b]
                parts = [caps[0][b], caps[1][b], caps[2][b], opens[0][b], opens[1][b], zs_open[:nch], zs_next[b], zs_open[nch:], opens[3][b]]
                proofs.append(b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in parts) + fri[b] +
                              (np.asarray(pis[b], dtype=np.uint64) % np.uint64(P)).tobytes())
            return proofs, zs_vals, q_coeffs
        finally:
            for o in oracles[1:]:
                o.close()
            for b in bufs:
                b.free(scrub=True)


def witnesses(pkg, gpu, pack, wires, count):
    """_witnesses of tests/test_batch_gpu.py; for a pack without the public-input cell trailer (a circuit with no Poseidon rows: its
    PublicInputGate row holds the hash as a plain source, and the template prover refuses it) the same thing by hand: the template's
    free cells under `count` different public inputs, completed by stage s1."""
    if pkg.binding.pack_public_input_cells(pack) is not None:
        return _witnesses(pkg, gpu, pack, wires, count)
    npis = pkg.pack_header(pack)["num_public_inputs"]
    circ = pkg.Circuit(gpu, pack)
    try:
        free = np.where(circ.witness_free_mask(*wires.shape) == 1, wires, 0).astype(np.uint64)
        out_p = [pkg.aggregation.leaf_public_inputs(i, npis) for i in range(count)]
        return out_p, [circ.generate_witness(free.copy(), p).copy() for p in out_p]
    finally:
        circ.close()


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


# ---- 1. the whole flow, per proof, against the oracle and against the all-in-one batch ----

@pytest.mark.parametrize("name, batch", [("narrow_2p6", 3), ("hash_base_sum_2p10", 2)])
def test_whole_flow_per_proof(pkg, gpu, orc, name, batch):
    d, kw = sp.CIRCUITS[name]
    pack, wires, _ = pkg.synth_circuit(d, **kw)
    pis, ws = witnesses(pkg, gpu, pack, wires, batch)
    assert len({w.tobytes() for w in ws}) == batch
    oc = OracleCircuit(orc, pack)
    circ = pkg.Circuit(gpu, pack, max_batch=batch)
    fl = BatchFlow(pkg, gpu, orc, pack, batch)
    try:
        got, _, _ = fl.prove_batch(ws, pis)
        bufs = [gpu.to_device(w) for w in ws]
        all_in_one = circ.prove_batch_dev(bufs, pis)
        for x in bufs:
            x.free()
        for b in range(batch):
            want = oc.prove(ws[b], pis[b])
            assert len(got[b]) == len(want)
            assert got[b] == want, "proof %d of the batched stage flow differs from the oracle's at byte %d" % (b, first_diff(got[b], want))
            assert got[b] == all_in_one[b], "proof %d differs from qpgpu_prove_batch_dev's at byte %d" % (b, first_diff(got[b], all_in_one[b]))
    finally:
        fl.close(); circ.close(); oc.close()


# ---- 2, 3, 6: each stage word for word; wire input forms; the batch of one ----

@pytest.fixture(scope="module")
def p2(pkg, gpu, orc):
    """The Poseidon2-rows circuit at 2^8 with three witnesses: the single-proof entries' outputs per witness (computed once) and
    the oracle's stage trace for proof 0."""
    d, kw = sp.CIRCUITS["poseidon2_rows_2p8"]
    pack, wires, _ = pkg.synth_circuit(d, **kw)
    pis, ws = _witnesses(pkg, gpu, pack, wires, 3)
    h = parse_pack(pack)
    n, nch = 1 << d, h["num_challenges"]
    okw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    oc = OracleCircuit(orc, pack)
    oc.prove(ws[0], pis[0])
    trace = {k: oc.trace(k).copy() for k in ("zs_pp_values", "quotient_chunk_coeffs", "betas", "gammas", "alphas")}
    oc.close()
    rng = np.random.default_rng(5)
    # proof 0 gets the oracle's challenges (so that its columns are the trace's), the others arbitrary ones
    ch = dict(betas=[list(trace["betas"])], gammas=[list(trace["gammas"])], alphas=[list(trace["alphas"])])
    for k in ch:
        ch[k] += [[int(x) for x in rng.integers(0, P, size=nch, dtype=np.uint64)] for _ in range(2)]
    pihs = [sp.public_inputs_hash(pkg, gpu, p) for p in pis]
    L = d + h["rate_bits"]
    points = [[int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(3)]
    indices = np.array([[0, (1 << L) - 1, 5, 5], [(1 << L) - 1, 17, 0, 300], [1, 2, (1 << L) - 2, 0]], dtype=np.uint64)
    single = dict(zs=[], q=[], w_cap=[], zs_cap=[], q_cap=[], w_eval=[], rows=[], paths=[])
    fl = sp.Flow(pkg, gpu, orc, pack)
    try:
        for b in range(3):
            o_w = pkg.PolyOracle(gpu, ws[b], **okw)
            d_zs = fl.plan.partial_products(ws[b], ch["betas"][b], ch["gammas"][b])
            o_zs = pkg.PolyOracle(gpu, (d_zs, fl.plan.num_zs_pp, n), **okw)
            d_q = fl.plan.quotient(o_w, o_zs, ch["betas"][b], ch["gammas"][b], ch["alphas"][b], pihs[b])
            o_q = pkg.PolyOracle(gpu, (d_q, fl.plan.num_quotient, n), coeffs=True, **okw)
            single["zs"].append(d_zs.download().reshape(-1, n)); single["q"].append(d_q.download().reshape(-1, n))
            single["w_cap"].append(o_w.cap().ravel()); single["zs_cap"].append(o_zs.cap().ravel()); single["q_cap"].append(o_q.cap().ravel())
            single["w_eval"].append(o_w.eval(points[b], 2, 7))
            r, p = o_w.open(indices[b])
            single["rows"].append(r); single["paths"].append(p)
            for x in (o_q, o_zs, o_w):
                x.close()
            d_q.free(scrub=True); d_zs.free(scrub=True)
    finally:
        fl.close()
    return dict(pack=pack, ws=ws, pis=pis, h=h, n=n, okw=okw, trace=trace, ch=ch, pihs=pihs, points=points, indices=indices, single=single)


def run_batched(pkg, gpu, orc, p2, batch, wires_form="host"):
    """The stages of `p2` through the batch entries for its first `batch` witnesses. wires_form: "host", "dense" (device, back to
    back) or "reversed" (separate device allocations passed in reverse order; the results are put back in order)."""
    ws, n, okw, c = p2["ws"][:batch], p2["n"], p2["okw"], p2["ch"]
    order = list(range(batch))
    dev = []
    fl = BatchFlow(pkg, gpu, orc, p2["pack"], batch)
    out = {}
    try:
        if wires_form == "host":
            src_commit = src_s5 = ws
        elif wires_form == "dense":
            dev = [gpu.to_device(np.stack(ws))]
            src_s5 = [dev[0].ptr + b * ws[0].nbytes for b in range(batch)]
            src_commit = [(q, ws[0].shape[0], n) for q in src_s5]
        else:
            order = order[::-1]
            dev = [gpu.to_device(w) for w in ws]
            src_s5 = [dev[b] for b in order]
            src_commit = [(dev[b], ws[0].shape[0], n) for b in order]
        pick = lambda k: [c[k][b] for b in order]
        o_w = pkg.PolyOracle.commit_batch(gpu, src_commit, **okw)
        d_zs = fl.plan.partial_products_batch(src_s5, pick("betas"), pick("gammas"))
        cols = fl.plan.num_zs_pp
        o_zs = pkg.PolyOracle.commit_batch(gpu, [(d_zs.ptr + b * cols * n * 8, cols, n) for b in range(batch)], **okw)
        d_q = fl.plan.quotient_batch(o_w, o_zs, batch, pick("betas"), pick("gammas"), pick("alphas"), [p2["pihs"][b] for b in order])
        qc = fl.plan.num_quotient
        o_q = pkg.PolyOracle.commit_batch(gpu, [(d_q.ptr + b * qc * n * 8, qc, n) for b in range(batch)], coeffs=True, **okw)
        inv = np.argsort(order)
        out = dict(zs=d_zs.download().reshape(batch, -1, n)[inv], q=d_q.download().reshape(batch, -1, n)[inv],
                   w_cap=o_w.cap()[inv], zs_cap=o_zs.cap()[inv], q_cap=o_q.cap()[inv],
                   w_eval=o_w.eval([p2["points"][b] for b in order], 2, 7)[inv], strides=o_w.strides(), batch=(o_w.batch, fl.plan.max_batch))
        r, p = o_w.open(p2["indices"][order])
        out["rows"], out["paths"] = r[inv], p[inv]
        for x in (o_q, o_zs, o_w):
            x.close()
        d_q.free(scrub=True); d_zs.free(scrub=True)
    finally:
        fl.close()
        for x in dev:
            x.free(scrub=True)
    return out


@pytest.fixture(scope="module")
def batched3(pkg, gpu, orc, p2):
    return run_batched(pkg, gpu, orc, p2, 3)


def test_each_stage_word_for_word(p2, batched3):
    got, one, n = batched3, p2["single"], p2["n"]
    assert got["batch"] == (3, 3)
    ncols = p2["ws"][0].shape[0]
    L = p2["h"]["degree_bits"] + p2["h"]["rate_bits"]
    assert got["strides"] == (ncols * n, ncols << L, ((2 << L) - (1 << p2["h"]["cap_height"])) * 4)
    for b in range(3):
        assert np.array_equal(got["zs"][b], one["zs"][b]), "qpgpu_stage_partial_products_batch, proof %d" % b
        assert np.array_equal(got["q"][b], one["q"][b]), "qpgpu_stage_quotient_batch, proof %d" % b
        assert np.array_equal(got["w_eval"][b], one["w_eval"][b]), "qpgpu_oracle_eval_batch, proof %d" % b
        assert np.array_equal(got["rows"][b], one["rows"][b]), "qpgpu_oracle_open_batch rows, proof %d" % b
        assert np.array_equal(got["paths"][b], one["paths"][b]), "qpgpu_oracle_open_batch paths, proof %d" % b
        for k in ("w_cap", "zs_cap", "q_cap"):
            assert np.array_equal(got[k][b], one[k][b]), "qpgpu_oracle_cap of %s, proof %d" % (k, b)
    assert np.array_equal(got["zs"][0], p2["trace"]["zs_pp_values"].reshape(-1, n))
    assert np.array_equal(got["q"][0], p2["trace"]["quotient_chunk_coeffs"].reshape(-1, n))
    assert not np.array_equal(got["zs"][0], got["zs"][1]) and not np.array_equal(got["w_cap"][1], got["w_cap"][2])


@pytest.mark.parametrize("form", ["dense", "reversed"])
def test_wire_input_forms(pkg, gpu, orc, p2, batched3, form):
    got = run_batched(pkg, gpu, orc, p2, 3, wires_form=form)
    assert np.array_equal(got["w_cap"], batched3["w_cap"]), "wire commitment from %s device matrices" % form
    assert np.array_equal(got["zs"], batched3["zs"]), "s5 from %s device matrices" % form
    assert np.array_equal(got["q"], batched3["q"]) and np.array_equal(got["q_cap"], batched3["q_cap"])


def test_batch_of_one(pkg, gpu, orc, p2):
    """Every new entry at batch = 1, on a plan of max_batch = 1: the single-proof entries' words; the whole flow and the FRI
    entries: their bytes."""
    got, one = run_batched(pkg, gpu, orc, p2, 1), p2["single"]
    assert got["batch"] == (1, 1) and got["strides"] == (0, 0, 0)
    for k in ("zs", "q", "w_cap", "zs_cap", "q_cap", "w_eval", "rows", "paths"):
        assert np.array_equal(got[k][0], one[k][0]), k
    fl1, flb = sp.Flow(pkg, gpu, orc, p2["pack"]), BatchFlow(pkg, gpu, orc, p2["pack"], 1)
    try:
        want = fl1.prove(p2["ws"][1], p2["pis"][1])[0]
        assert flb.prove_batch([p2["ws"][1]], [p2["pis"][1]])[0] == [want]
        # a plan made by the batch entry serves the single-proof entries too
        assert flb.prove(p2["ws"][1], p2["pis"][1])[0] == want
    finally:
        fl1.close(); flb.close()
    ch = steps.started_challenger(pkg, gpu, 5)
    assert pkg.fri_grind_batch(gpu, [ch], 8) == [pkg.fri_grind(gpu, ch, 8)]


# ---- 4. zero knowledge ----

def test_zero_knowledge_batch(pkg, gpu, orc):
    pack, wires, _ = pkg.synth_circuit(8, seed=64, poseidon=True)
    pack = pack.copy(); pack[14] = 1
    pis, ws = _witnesses(pkg, gpu, pack, wires, 2)
    oc = OracleCircuit(orc, pack)
    fl = BatchFlow(pkg, gpu, orc, pack, 2)
    try:
        got, _, _ = fl.prove_batch(ws, pis, seed=4242)
        for b in range(2):
            want = oc.prove(ws[b], pis[b], seed=4242 + b)
            assert got[b] == want, "seeded zero-knowledge proof %d differs at byte %d" % (b, first_diff(got[b], want))
        # unseeded: the same witness twice in one batch opens to different salt words
        o = pkg.PolyOracle.commit_batch(gpu, [ws[0], ws[0]], blinding=True, blinding_seed=0, blinding_stream=1, **fl.kw)
        try:
            rows, _ = o.open([[0, 1, 2, 3], [0, 1, 2, 3]], paths=False)
            nw = ws[0].shape[0]
            assert rows.shape == (2, 4, nw + 4)
            assert np.array_equal(rows[0, :, :nw], rows[1, :, :nw])
            for q in range(4):
                assert not np.array_equal(rows[0, q, nw:], rows[1, q, nw:]), q
            assert not np.array_equal(o.cap()[0], o.cap()[1])
        finally:
            o.close()
    finally:
        fl.close(); oc.close()


# ---- 5. FRI steps on a batch ----

def three_oracles(pkg, gpu, d, rate, cap, seed):
    rng = np.random.default_rng(seed)
    polys = rng.integers(0, P, size=(3, 3, 1 << d), dtype=np.uint64)
    points = [[int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(3)]
    kw = dict(rate_bits=rate, cap_height=cap)
    return pkg.PolyOracle.commit_batch(gpu, polys, **kw), [pkg.PolyOracle(gpu, polys[b], **kw) for b in range(3)], points


@pytest.mark.parametrize("d, arity", [(6, [4]), (9, [1, 2, 3]), (6, [])], ids=["4", "1-2-3", "none_2p6"])
def test_fri_steps_on_a_batch(pkg, gpu, d, arity):
    rate, cap = 3, 2
    L = d + rate
    ob, os1, points = three_oracles(pkg, gpu, d, rate, cap, seed=70 + d)
    alphas = [(11, 13), (P - 2, 5), (0x123456789, 0)]
    betas = [[(3, 5), (P - 1, 1), (7, 0)], [(2, 2), (9, 1 << 40), (P - 3, 4)], [(0x55, 0), (1, 1), (6, P - 6)]]      # [proof][round]
    indices = np.array([[0, (1 << L) - 1, 77, 77], [5, 0, 300, (1 << L) - 1], [(1 << L) - 2, 1, 2, 3]], dtype=np.uint64)
    kw = dict(rate_bits=rate, cap_height=cap)
    fill = np.full(1 << 16, 0xA5A5A5A5, dtype=np.uint64)      # large enough for any of the refused calls, were it not refused
    lib = gpu.lib

    def refused(rc, *parts):
        msg = gpu.last_error()
        assert rc == -1 and all(p in msg for p in parts), (rc, msg)
        assert (fill == 0xA5A5A5A5).all()

    try:
        want = []
        for b in range(3):
            with pkg.FriSession(gpu, [os1[b]], [(points[b], [(0, 0, 3)])], alphas[b], arity, **kw) as s:
                caps = []
                for r in range(len(arity)):
                    caps.append(s.round_commit().ravel()); s.round_fold(betas[b][r])
                want.append(dict(caps=caps, final=s.final_poly(), open=s.open(indices[b]), qs=s.query_size))
        with pkg.FriSession(gpu, [ob], [(points, [(0, 0, 3)])], alphas, arity, batch=3, **kw) as s:
            assert s.query_size == want[0]["qs"]
            capw = 4 << cap
            n = ctypes.c_size_t(55)
            for r in range(len(arity)):
                # a batch-1 sized cap buffer: refused naming the expected size, nothing written, the session goes on
                refused(lib.qpgpu_fri_round_commit(s.h, fill.ctypes.data, capw), "fri_round_commit", "cap_words", str(3 * capw))
                got = s.round_commit()
                for b in range(3):
                    assert np.array_equal(got[b], want[b]["caps"][r]), (r, b)
                s.round_fold([betas[b][r] for b in range(3)])
            refused(lib.qpgpu_fri_final_poly(s.h, fill.ctypes.data, 2 * s.final_len, ctypes.byref(n)), "fri_final_poly", "out_words", str(6 * s.final_len))
            final = s.final_poly()
            refused(lib.qpgpu_fri_open(s.h, indices.ctypes.data, 4, fill.ctypes.data, 4 * s.query_size, ctypes.byref(n)), "fri_open", "out_cap", "3 x 4 x")
            assert n.value == 55
            opened = s.open(indices)
            for b in range(3):
                assert np.array_equal(final[b], want[b]["final"]), b
                assert opened[b] == want[b]["open"], "qpgpu_fri_open, proof %d, byte %d" % (b, first_diff(opened[b], want[b]["open"]))
        # the one-call form: bytes and final challenger state of three single calls
        pkw = dict(proof_of_work_bits=4, num_query_rounds=3, **kw)
        ch_b = [steps.started_challenger(pkg, gpu, 5 + b) for b in range(3)]
        ch_1 = [steps.started_challenger(pkg, gpu, 5 + b) for b in range(3)]
        got = pkg.fri_prove_batch(gpu, [ob], [(points, [(0, 0, 3)])], ch_b, arity, **pkw)
        for b in range(3):
            one = pkg.fri_prove(gpu, [os1[b]], [(points[b], [(0, 0, 3)])], ch_1[b], arity, **pkw)
            assert got[b] == one, "qpgpu_fri_prove_batch, proof %d, byte %d" % (b, first_diff(got[b], one))
            assert bytes(ch_b[b].state) == bytes(ch_1[b].state), b
    finally:
        ob.close()
        for o in os1:
            o.close()


def test_grind_batch(pkg, gpu):
    chs = [steps.started_challenger(pkg, gpu, 20 + b) for b in range(3)]
    before = [bytes(c.state) for c in chs]
    want = [pkg.fri_grind(gpu, c, 8) for c in chs]
    assert pkg.fri_grind_batch(gpu, chs, 8) == want and len(set(want)) > 1
    assert pkg.fri_grind_batch(gpu, chs, 0) == [0, 0, 0]
    assert [bytes(c.state) for c in chs] == before
    chs[1].observe([3])                                  # one transcript ahead of the others
    with pytest.raises(pkg.QpGpuError) as e:
        pkg.fri_grind_batch(gpu, chs, 8)
    assert e.value.code == -1 and "challengers[1]" in str(e.value)


# ---- 7. unsatisfied witness ----

def test_unsatisfied_witness_names_the_proof(pkg, gpu, orc):
    pack, wires, _ = pkg.synth_circuit(8, seed=61, poseidon=True, base_sum=True)
    pis, ws = _witnesses(pkg, gpu, pack, wires, 3)
    bad = [w.copy() for w in ws]
    bad[1][3, 20] = (int(bad[1][3, 20]) + 1) % P         # arithmetic output of op 0 on row 20, proof 1
    circ = pkg.Circuit(gpu, pack, max_batch=3)
    fl = BatchFlow(pkg, gpu, orc, pack, 3)
    try:
        with pytest.raises(pkg.QpGpuError) as e:
            fl.prove_batch(bad, pis)
        assert e.value.code == -4 and "row 20" in str(e.value) and "(proof 1 of the batch)" in str(e.value), str(e.value)
        bufs = [gpu.to_device(w) for w in ws]
        want = circ.prove_batch_dev(bufs, pis)
        for x in bufs:
            x.free()
        assert fl.prove_batch(ws, pis)[0] == want
    finally:
        fl.close(); circ.close()


# ---- 8. argument errors name the argument ----

def test_argument_errors_name_the_argument(pkg, gpu, orc):
    d, kw = sp.CIRCUITS["narrow_2p6"]
    pack, wires, _ = pkg.synth_circuit(d, **kw)
    h = parse_pack(pack)
    n, L = 1 << d, d + h["rate_bits"]
    okw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])

    def refused(make, *names):
        with pytest.raises(pkg.QpGpuError) as e:
            make()
        assert e.value.code == -1 and all(s in str(e.value) for s in names), str(e.value)

    fl = BatchFlow(pkg, gpu, orc, pack, 3)
    o_w3 = pkg.PolyOracle.commit_batch(gpu, [wires] * 3, **okw)
    o_w2 = pkg.PolyOracle.commit_batch(gpu, [wires] * 2, **okw)
    cs2 = pkg.PolyOracle.commit_batch(gpu, [h["constants_sigmas"]] * 2, **okw)
    plan = fl.plan
    ones = lambda b: [[1] * plan.num_challenges] * b
    d_zs = plan.partial_products_batch([wires] * 3, ones(3), ones(3))
    o_zs3 = pkg.PolyOracle.commit_batch(gpu, [(d_zs.ptr + b * plan.num_zs_pp * n * 8, plan.num_zs_pp, n) for b in range(3)], **okw)
    try:
        assert plan.max_batch == 3
        refused(lambda: plan.partial_products_batch([wires] * 4, ones(4), ones(4)), "stage_partial_products_batch", "batch is 4", "max_batch is 3")
        refused(lambda: plan.quotient_batch(o_w3, o_zs3, 4, ones(4), ones(4), ones(4), [[0] * 4] * 4), "stage_quotient_batch", "batch is 4", "max_batch")
        refused(lambda: plan.quotient_batch(o_w2, o_zs3, 3, ones(3), ones(3), ones(3), [[0] * 4] * 3), "wires_oracle", "holds 2 proofs")
        refused(lambda: plan.quotient_batch(o_w3, o_w2, 3, ones(3), ones(3), ones(3), [[0] * 4] * 3), "zs_pp_oracle")
        refused(lambda: plan.quotient(o_w3, o_zs3, ones(1), ones(1), ones(1), [0] * 4), "wires_oracle", "qpgpu_stage_quotient_batch")
        refused(lambda: pkg.StagePlan(gpu, pack, cs2, max_batch=3), "cs_oracle", "batch of 2")
        refused(lambda: pkg.StagePlan(gpu, pack, cs2), "cs_oracle", "batch of 2")
        zeta = [[5, 6]] * 3
        refused(lambda: pkg.FriSession(gpu, [fl.o_cs, o_w3, o_w2], [(zeta, [(0, 0, 1), (1, 0, 1), (2, 0, 1)])], [[1, 2]] * 3, h["arity_bits"], batch=3, **okw),
                "oracle 2", "holds 2 proofs", "batch of 3")
        refused(lambda: pkg.fri_prove_batch(gpu, [o_w2, o_w3], [(zeta, [(0, 0, 1)])], [pkg.Challenger(gpu) for _ in range(3)], h["arity_bits"],
                                            proof_of_work_bits=0, num_query_rounds=2, **okw), "oracle 0", "holds 2 proofs")
        refused(lambda: pkg.fri_prove(gpu, [o_w3], [((5, 6), [(0, 0, 1)])], pkg.Challenger(gpu), h["arity_bits"], proof_of_work_bits=0,
                                      num_query_rounds=2, **okw), "oracle 0", "holds 3 proofs")
        # the single-proof read entries on a batched oracle: refused naming what to use; they do not serve proof 0
        two, out = np.array([1, 2], dtype=np.uint64), np.full(1 << 14, 0xA5A5, dtype=np.uint64)
        for call, parts in ((lambda: gpu.lib.qpgpu_oracle_eval(o_w3.h, two.ctypes.data, 0, 1, out.ctypes.data), ("oracle_eval", "batch of 3", "qpgpu_oracle_eval_batch")),
                            (lambda: gpu.lib.qpgpu_oracle_read(o_w3.h, 0, 0, 1, out.ctypes.data), ("oracle_read", "batch of 3", "qpgpu_oracle_strides")),
                            (lambda: gpu.lib.qpgpu_oracle_open(o_w3.h, two.ctypes.data, 2, out.ctypes.data, None), ("oracle_open", "batch of 3", "qpgpu_oracle_open_batch"))):
            assert call() == -1 and all(s in gpu.last_error() for s in parts), gpu.last_error()
            assert (out == 0xA5A5).all()
        # a cap buffer for one proof only
        assert gpu.lib.qpgpu_oracle_cap(o_w3.h, out.ctypes.data, 4 << h["cap_height"]) == -1 and (out == 0xA5A5).all()
        # an index out of range at proof 1, entry 2: named, outputs untouched
        idx = np.array([[0, 1, 2], [3, 4, 1 << L], [5, 6, 7]], dtype=np.uint64)
        rows = np.full((3, 3, o_w3.leaf_width), 0xA5A5, dtype=np.uint64)
        paths = np.full((3, 3, L - h["cap_height"], 4), 0xA5A5, dtype=np.uint64)
        rc = gpu.lib.qpgpu_oracle_open_batch(o_w3.h, idx.ctypes.data, 3, rows.ctypes.data, paths.ctypes.data)
        assert rc == -1 and "indices[1][2]" in gpu.last_error() and str(1 << L) in gpu.last_error(), gpu.last_error()
        assert (rows == 0xA5A5).all() and (paths == 0xA5A5).all()
        # batch 0 and 1025
        arr = (ctypes.c_void_p * 1)(wires.ctypes.data)
        hh = ctypes.c_void_p()
        for bad in (0, 1025):
            assert gpu.lib.qpgpu_oracle_commit_batch(gpu.ctx, arr, bad, wires.shape[0], d, 3, 4, 0, 0, 0, ctypes.byref(hh)) == -1
            assert "1..1024" in gpu.last_error() and not hh.value
    finally:
        o_zs3.close(); d_zs.free(scrub=True); cs2.close(); o_w2.close(); o_w3.close(); fl.close()


# ---- 9. the C example ----

def test_stage_example_in_c_with_a_batch(tmp_path):
    """examples/stage_prove_example.c, `<degree_bits> batch <N>`: the whole flow for N witnesses in lockstep from plain C; the example
    compares each proof's bytes with qpgpu_prove_batch_dev's itself."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "qpgpu_stage_prove_example_batch")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "stage_prove_example.c"),
                           "-L", os.path.join(root, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(root, "qp-zk-circuits_amd"), "-o", out])
    res = subprocess.run([out, "8", "batch", "3"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "staged flow in lockstep, 3 proofs, == qpgpu_prove_batch_dev" in res.stdout
