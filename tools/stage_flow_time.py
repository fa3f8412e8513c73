"""Stages s5 + s6 through the stage-level entries against the same two stages inside the all-in-one prover's lockstep batch.

  stage_flow_time.py [--degree-bits 13] [--batch 32] [--reps 20] [--out profiles/stage_flow.txt]

The leaf circuit padded to 2^degree_bits rows, one witness made on the device. All-in-one: qpgpu_prove_batch_dev on `batch` copies of
the witness, the library's profile regions prove_partial_products and prove_quotient (HIP events around each stage of the whole
batch), mean of three batches after a warm-up batch, divided by the batch: what bench.py reports as lockstep_batch_stage_ms. Stage
flow: qpgpu_stage_partial_products and qpgpu_stage_quotient on the committed oracles of ONE proof, a host timer around each
synchronous call (witness check, its two transforms and the stream synchronisation included), median of --reps calls after two
warm-up calls; the same profile regions are read there too (the kernels alone, at a batch of one). The engine clock over the stage-flow
window is read as bench.py reads it. Also printed: the device-to-host bytes of the three LDEs a caller without the two entries
downloads per proof, 8 * 2^(degree_bits + rate_bits) * columns. Prints one JSON line and appends it, with the command, to --out.
No GPU: it fails, it does not fall back."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, default=13)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    from bench import EngineClock
    import leaf_cases
    L = pkg.leaf
    leaf = L.LeafCircuit(min_degree_bits=a.degree_bits)
    pack = leaf.pack
    h = pkg.pack_header(pack)
    d, n, nw, nch = h["degree_bits"], 1 << h["degree_bits"], h["num_wires"], h["num_challenges"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    off = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    cs = np.ascontiguousarray(pack[off:off + ncs * n]).reshape(ncs, n)
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
    cells, values, pis = leaf.commit(leaf_cases.dummy_inputs(L))
    med = lambda v: round(float(np.median(v)), 4)
    B = a.batch
    with pkg.QpGpu(0) as gpu:
        circ = pkg.Circuit(gpu, pack, max_batch=B)
        d_w = gpu.alloc(nw * n * 8)
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        # ---- all-in-one, lockstep batch (the scattered-witness path gathers B copies of the one witness) ----
        ptrs, pil = [d_w.ptr] * B, [pis] * B
        want = circ.prove_batch_dev(ptrs, pil)[0]
        gpu.profile(True)
        for _ in range(3):
            circ.prove_batch_dev(ptrs, pil)
        lock = {}
        for s in ("prove_partial_products", "prove_quotient"):
            ms, cnt = gpu.profile_read(s)
            lock[s] = ms / max(cnt, 1)
        gpu.profile(False)
        circ.close()
        # ---- the stage flow, one proof ----
        o_cs = pkg.PolyOracle(gpu, cs, **kw)
        plan = pkg.StagePlan(gpu, pkg.stage_header_words(pack), o_cs)
        o_w = pkg.PolyOracle(gpu, (d_w, nw, n), blinding_stream=1, **kw)
        ch = pkg.Challenger(gpu)
        ch.observe(o_w.cap())
        betas, gammas, alphas = ch.get_n(nch), ch.get_n(nch), ch.get_n(nch)
        pih = np.arange(1, 5, dtype=np.uint64)

        def once():
            t0 = time.perf_counter()
            d_zs = plan.partial_products(d_w, betas, gammas)
            t1 = time.perf_counter()
            o_zs = pkg.PolyOracle(gpu, (d_zs, plan.num_zs_pp, n), blinding_stream=2, **kw)
            t2 = time.perf_counter()
            d_q = plan.quotient(o_w, o_zs, betas, gammas, alphas, pih)
            t3 = time.perf_counter()
            o_zs.close(); d_zs.free(); d_q.free()
            return 1e3 * (t1 - t0), 1e3 * (t3 - t2)
        once(); once()
        with EngineClock(gpu) as clk:
            t = [once() for _ in range(a.reps)]
        clock = clk.summary(skip_s=0.0)
        gpu.profile(True)
        for _ in range(3):
            once()
        kern = {}
        for s in ("prove_partial_products", "prove_quotient"):
            ms, cnt = gpu.profile_read(s)
            kern[s] = ms / max(cnt, 1)
        gpu.profile(False)
        fused = plan.fused_selected
        o_w.close(); plan.close(); o_cs.close(); d_w.free(scrub=True)
    s5, s6 = med([x[0] for x in t]), med([x[1] for x in t])
    lock_pp = (lock["prove_partial_products"] + lock["prove_quotient"]) / B
    lde = 8 << (d + h["rate_bits"])
    res = {"degree_bits": d, "batch": B, "reps": a.reps, "fused_quotient": fused,
           "lockstep_s5_ms_per_batch": round(lock["prove_partial_products"], 4), "lockstep_s6_ms_per_batch": round(lock["prove_quotient"], 4),
           "lockstep_s5_s6_ms_per_proof": round(lock_pp, 4),
           "stage_s5_ms": s5, "stage_s6_ms": s6, "stage_s5_s6_ms": round(s5 + s6, 4),
           "stage_s5_min_max_ms": [round(min(x[0] for x in t), 4), round(max(x[0] for x in t), 4)],
           "stage_s6_min_max_ms": [round(min(x[1] for x in t), 4), round(max(x[1] for x in t), 4)],
           "stage_kernels_only_ms": {k: round(v, 4) for k, v in kern.items()},
           "stage_over_lockstep_per_proof": round((s5 + s6) / lock_pp, 2) if lock_pp else None,
           "engine_clock_mhz": clock,
           "lde_download_bytes_avoided": {"constants_sigmas": lde * ncs, "wires": lde * nw, "zs_partial_products": lde * plan.num_zs_pp,
                                          "total": lde * (ncs + nw + plan.num_zs_pp)},
           "proof_bytes": len(want)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("$ python tools/stage_flow_time.py " + " ".join(sys.argv[1:]) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
