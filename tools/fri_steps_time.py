"""Stages s8..s11 (PolynomialBatch::prove_openings) through the step entries against the single call qpgpu_fri_prove.

  fri_steps_time.py [--degree-bits 13] [--reps 20] [--out profiles/fri_steps.txt]

The leaf circuit padded to 2^degree_bits rows, one witness made on the device, the stage flow run up to the openings (four committed
oracles, two opening points, the challenger as it stands after the openings were observed). From that state, on copies of the
challenger: (a) qpgpu_fri_prove; (b) qpgpu_fri_begin, per round qpgpu_fri_round_commit / _fold, qpgpu_fri_final_poly, qpgpu_fri_grind,
qpgpu_fri_open, with the host challenger calls between them, through the Python binding. A host timer around each, median of --reps
calls after two warm-up calls, the two alternated call by call. The bytes of (b) are compared with (a)'s every time. Prints one JSON
line and appends it, with the command, to --out. Not a pass/fail figure. No GPU: it fails, it does not fall back."""
import argparse, ctypes, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge

P = 0xFFFFFFFF00000001
POWER_OF_TWO_GENERATOR = 7277203076849721926


def copy_challenger(pkg, ch):
    other = pkg.Challenger(ch.gpu)
    ctypes.memmove(ctypes.byref(other.state), ctypes.byref(ch.state), ctypes.sizeof(ch.state))
    return other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, default=13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    import leaf_cases
    L = pkg.leaf
    leaf = L.LeafCircuit(min_degree_bits=a.degree_bits)
    pack = leaf.pack
    h = pkg.pack_header(pack)
    d, n, nw, nch = h["degree_bits"], 1 << h["degree_bits"], h["num_wires"], h["num_challenges"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    off = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    cs = np.ascontiguousarray(pack[off:off + ncs * n]).reshape(ncs, n)
    arity = [int(x) for x in pack[18:18 + h["num_arity_rounds"]]]
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    pow_bits, nq = h["proof_of_work_bits"], h["num_query_rounds"]
    zkw = dict(blinding=True, blinding_seed=1) if h["zero_knowledge"] else {}
    cells, values, pis = leaf.commit(leaf_cases.dummy_inputs(L))
    with pkg.QpGpu(0) as gpu:
        circ = pkg.Circuit(gpu, pack)
        d_w = gpu.alloc(nw * n * 8)
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        circ.close()
        # the stage flow up to the openings
        o_cs = pkg.PolyOracle(gpu, cs, **kw)
        plan = pkg.StagePlan(gpu, pkg.stage_header_words(pack), o_cs)
        hc = pkg.Challenger(gpu)
        hc.observe(np.asarray(pis, dtype=np.uint64) % np.uint64(P)); hc.get()
        pih = np.array(list(hc.state.sponge_state)[:4], dtype=np.uint64)
        ch = pkg.Challenger(gpu)
        o_w = pkg.PolyOracle(gpu, (d_w, nw, n), blinding_stream=1, **kw, **zkw)
        ch.observe(pack[off - 4:off]); ch.observe(pih); ch.observe(o_w.cap())
        betas, gammas = ch.get_n(nch), ch.get_n(nch)
        d_zs = plan.partial_products(d_w, betas, gammas)
        o_zs = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), blinding_stream=2, **kw, **zkw)
        ch.observe(o_zs.cap())
        alphas = ch.get_n(nch)
        d_q = plan.quotient(o_w, o_zs, betas, gammas, alphas, pih)
        o_q = pkg.PolyOracle(gpu, (d_q, plan.num_quotient, n), coeffs=True, blinding_stream=3, **kw, **zkw)
        ch.observe(o_q.cap())
        zeta = ch.get_n(2)
        g = pow(POWER_OF_TWO_GENERATOR, 1 << (32 - d), P)
        g_zeta = [zeta[0] * g % P, zeta[1] * g % P]
        oracles = [o_cs, o_w, o_zs, o_q]
        ch.observe(np.concatenate([o.eval(zeta) for o in oracles])); ch.observe(o_zs.eval(g_zeta, 0, nch))
        batches = [(zeta, [(i, 0, o.num_polys) for i, o in enumerate(oracles)]), (g_zeta, [(2, 0, nch)])]

        def single():
            c = copy_challenger(pkg, ch)
            t0 = time.perf_counter()
            out = pkg.fri_prove(gpu, oracles, batches, c, arity, proof_of_work_bits=pow_bits, num_query_rounds=nq, **kw)
            return 1e3 * (time.perf_counter() - t0), out

        def steps():
            c = copy_challenger(pkg, ch)
            t0 = time.perf_counter()
            caps = []
            with pkg.FriSession(gpu, oracles, batches, c.get_n(2), arity, **kw) as s:
                for _ in arity:
                    caps.append(s.round_commit())
                    c.observe(caps[-1])
                    s.round_fold(c.get_n(2))
                final = s.final_poly()
                c.observe(final)
                nonce = pkg.fri_grind(gpu, c, pow_bits)
                c.observe([nonce]); c.get()
                queries = s.open([c.get() % s.lde_size for _ in range(nq)])
            out = b"".join(x.tobytes() for x in caps) + queries + final.tobytes() + np.uint64(nonce).tobytes()
            return 1e3 * (time.perf_counter() - t0), out

        for _ in range(2):
            want = single()[1]
            assert steps()[1] == want, "the steps' bytes differ from qpgpu_fri_prove's"
        ta, tb = [], []
        for _ in range(a.reps):
            t, x = single(); ta.append(t)
            t, y = steps(); tb.append(t)
            assert x == want and y == want
        for o in (o_q, o_zs, o_w):
            o.close()
        d_q.free(scrub=True); d_zs.free(scrub=True); plan.close(); o_cs.close(); d_w.free(scrub=True)
    med = lambda v: round(float(np.median(v)), 4)
    res = {"degree_bits": d, "reps": a.reps, "rounds": arity, "proof_of_work_bits": pow_bits, "num_query_rounds": nq,
           "fri_prove_ms": med(ta), "fri_prove_min_max_ms": [round(min(ta), 4), round(max(ta), 4)],
           "fri_steps_ms": med(tb), "fri_steps_min_max_ms": [round(min(tb), 4), round(max(tb), 4)],
           "steps_over_single": round(med(tb) / med(ta), 3), "fri_proof_bytes": len(want)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("$ python tools/fri_steps_time.py " + " ".join(sys.argv[1:]) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
