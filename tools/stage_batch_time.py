"""The stage flow for a lockstep batch (the *_batch entries of include/qpgpu.h) against the all-in-one prover at the same batch and
against the single-proof stage flow.

  stage_batch_time.py [--degree-bits 13] [--batches 1,8,32] [--reps 20] [--out profiles/stage_batch.txt]

The leaf circuit padded to 2^degree_bits rows, one witness made on the device and copied `batch` times back to back. Per batch size
three figures, in ms per proof, each the median of --reps runs after two warm-up runs, a host timer around the synchronous calls:
  stage_batch_ms_per_proof   commit -> s5 -> commit -> s6 -> commit -> openings -> qpgpu_fri_prove_batch through the batch entries,
                             the `batch` transcripts in the binding's Challenger (a ctypes call per observe / squeeze)
  all_in_one_ms_per_proof    qpgpu_prove_batch_dev at the same batch (transcripts inside the library)
  stage_single_ms_per_proof  the same flow through the single-proof entries, one proof
The engine clock over each batch size's window is read as bench.py reads it. The library's profile regions (qpgpu_profile_*) over
three further batched runs give the device time of the stages the two routes bracket alike (s5, s6, the FRI steps); the commitments and
the opening evaluations are not bracketed on the stage route (their regions read 0), so "outside_regions" is their kernels plus the
caller's side: transcripts, calls, allocations. Each batch size runs in a child process of its own under `timeout`; the first one
that fails ends the run. Prints one JSON line per batch size and appends them, with the command, to --out. No GPU: it fails, it does
not fall back."""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = 0xFFFFFFFF00000001
POWER_OF_TWO_GENERATOR = 7277203076849721926
REGIONS = ("prove_commit_wires", "prove_partial_products", "prove_commit_zs", "prove_quotient", "prove_commit_quotient", "prove_openings",
           "prove_fri_batch", "prove_fri_commit", "prove_pow", "prove_queries")


def pi_hash(pkg, gpu, pis):
    ch = pkg.Challenger(gpu)
    ch.observe(np.asarray(pis, dtype=np.uint64) % np.uint64(P))
    ch.get()
    return np.array(list(ch.state.sponge_state)[:4], dtype=np.uint64)


class Flow:
    """prove() after witness generation over the stage entries; batch None: the single-proof entries."""

    def __init__(self, pkg, gpu, pack, batch):
        self.pkg, self.gpu, self.batch = pkg, gpu, batch
        h = self.h = pkg.pack_header(pack)
        self.n = 1 << h["degree_bits"]
        ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
        off = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"]
        self.digest = pack[off:off + 4].copy()
        cs = np.ascontiguousarray(pack[off + 4:off + 4 + ncs * self.n]).reshape(ncs, self.n)
        self.arity = [int(x) for x in pack[18:18 + h["num_arity_rounds"]]]
        self.kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"])
        self.o_cs = pkg.PolyOracle(gpu, cs, **self.kw)
        self.plan = pkg.StagePlan(gpu, pkg.stage_header_words(pack), self.o_cs, max_batch=batch)
        self.g = pow(POWER_OF_TWO_GENERATOR, 1 << (32 - h["degree_bits"]), P)

    def close(self):
        self.plan.close(); self.o_cs.close()

    def prove(self, d_wires, pis, pih):
        """d_wires: device pointer of `batch` wire matrices back to back. Returns the proofs' bytes."""
        pkg, gpu, h, plan, n, kw = self.pkg, self.gpu, self.h, self.plan, self.n, self.kw
        nch, nw, B = h["num_challenges"], h["num_wires"], self.batch or 1
        one = self.batch is None
        commit = (lambda ptr, cols, **k: pkg.PolyOracle(gpu, (ptr, cols, n), **kw, **k)) if one else \
            (lambda ptr, cols, **k: pkg.PolyOracle.commit_batch(gpu, [(ptr + b * cols * n * 8, cols, n) for b in range(B)], **kw, **k))
        rows = (lambda x: np.asarray(x).reshape(1, -1)) if one else (lambda x: x)          # per-proof rows of a cap
        per = (lambda x: np.asarray(x)[None]) if one else (lambda x: x)                    # per-proof blocks of an evaluation
        chs = [pkg.Challenger(gpu) for _ in range(B)]
        oracles, bufs = [self.o_cs], []
        try:
            o_w = commit(d_wires, nw, blinding_stream=1); oracles.append(o_w)
            cap = rows(o_w.cap())
            betas, gammas, alphas, zetas, g_zetas = [], [], [], [], []
            for b, ch in enumerate(chs):
                ch.observe(self.digest); ch.observe(pih); ch.observe(cap[b])
                betas.append(ch.get_n(nch)); gammas.append(ch.get_n(nch))
            d_zs = plan.partial_products(d_wires, betas[0], gammas[0]) if one else \
                plan.partial_products_batch([d_wires + b * nw * n * 8 for b in range(B)], betas, gammas)
            bufs.append(d_zs)
            o_zs = commit(d_zs.ptr, plan.num_zs_pp, blinding_stream=2); oracles.append(o_zs)
            cap_zs = rows(o_zs.cap())
            for b, ch in enumerate(chs):
                ch.observe(cap_zs[b]); alphas.append(ch.get_n(nch))
            d_q = plan.quotient(o_w, o_zs, betas[0], gammas[0], alphas[0], pih) if one else \
                plan.quotient_batch(o_w, o_zs, B, betas, gammas, alphas, [pih] * B)
            bufs.append(d_q)
            o_q = commit(d_q.ptr, plan.num_quotient, coeffs=True, blinding_stream=3); oracles.append(o_q)
            cap_q = rows(o_q.cap())
            for b, ch in enumerate(chs):
                ch.observe(cap_q[b])
                z = ch.get_n(2)
                zetas.append(z); g_zetas.append([z[0] * self.g % P, z[1] * self.g % P])
            opens = [np.stack([self.o_cs.eval(z) for z in zetas])]
            opens += [per(o.eval(zetas[0] if one else zetas)) for o in oracles[1:]]
            zs_next = per(o_zs.eval(g_zetas[0] if one else g_zetas, 0, nch))
            for b, ch in enumerate(chs):
                ch.observe(np.concatenate([x[b] for x in opens])); ch.observe(zs_next[b])
            ranges = [(i, 0, o.num_polys) for i, o in enumerate(oracles)]
            fkw = dict(proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"], **kw)
            if one:
                fri = [pkg.fri_prove(gpu, oracles, [(zetas[0], ranges), (g_zetas[0], [(2, 0, nch)])], chs[0], self.arity, **fkw)]
            else:
                fri = pkg.fri_prove_batch(gpu, oracles, [(zetas, ranges), (g_zetas, [(2, 0, nch)])], chs, self.arity, **fkw)
            tail = (np.asarray(pis, dtype=np.uint64) % np.uint64(P)).tobytes()
            out = []
            for b in range(B):
                zo = opens[2][b]
                parts = [cap[b], cap_zs[b], cap_q[b], opens[0][b], opens[1][b], zo[:nch], zs_next[b], zo[nch:], opens[3][b]]
                out.append(b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in parts) + fri[b] + tail)
            return out
        finally:
            for o in oracles[1:]:
                o.close()
            for x in bufs:
                x.free()


def one_batch(a, B):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from bench import EngineClock
    import leaf_cases
    L = pkg.leaf
    leaf = L.LeafCircuit(min_degree_bits=a.degree_bits)
    pack = leaf.pack
    h = pkg.pack_header(pack)
    n, nw = 1 << h["degree_bits"], h["num_wires"]
    cells, values, pis = leaf.commit(leaf_cases.dummy_inputs(L))
    med = lambda v: round(float(np.median(v)), 4)

    def timed(fn, reps):
        fn(); fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
        return t

    with pkg.QpGpu(0) as gpu:
        circ = pkg.Circuit(gpu, pack, max_batch=B)
        mat = nw * n * 8
        d_w = gpu.alloc(mat * B)
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        one = d_w.download(nw * n)
        for b in range(1, B):
            gpu._check(gpu.lib.qpgpu_memcpy_h2d(gpu.ctx, d_w.ptr + b * mat, one.ctypes.data, mat))
        ptrs, pil = [d_w.ptr + b * mat for b in range(B)], [pis] * B
        pih = pi_hash(pkg, gpu, pis)
        want = circ.prove_batch_dev(ptrs, pil)
        fb, f1 = Flow(pkg, gpu, pack, B), Flow(pkg, gpu, pack, None)
        same = fb.prove(d_w.ptr, pis, pih) == want and f1.prove(d_w.ptr, pis, pih) == want[:1]
        with EngineClock(gpu) as clk:
            t_batch = timed(lambda: fb.prove(d_w.ptr, pis, pih), a.reps)
            t_all = timed(lambda: circ.prove_batch_dev(ptrs, pil), a.reps)
            t_one = timed(lambda: f1.prove(d_w.ptr, pis, pih), a.reps)
        clock = clk.summary(skip_s=0.0)
        gpu.profile(True)
        for _ in range(3):
            fb.prove(d_w.ptr, pis, pih)
        regions = {}
        for s in REGIONS:
            ms, cnt = gpu.profile_read(s)
            regions[s] = round(ms / 3 / B, 4)
        gpu.profile(False)
        fb.close(); f1.close(); circ.close(); d_w.free(scrub=True)
    dev = round(sum(regions.values()), 4)
    res = {"degree_bits": h["degree_bits"], "batch": B, "reps": a.reps, "bytes_equal_all_in_one": bool(same),
           "stage_batch_ms_per_proof": round(med(t_batch) / B, 4), "all_in_one_ms_per_proof": round(med(t_all) / B, 4),
           "stage_single_ms_per_proof": med(t_one),
           "stage_batch_min_max_ms_per_proof": [round(min(t_batch) / B, 4), round(max(t_batch) / B, 4)],
           "all_in_one_min_max_ms_per_proof": [round(min(t_all) / B, 4), round(max(t_all) / B, 4)],
           "stage_single_min_max_ms": [round(min(t_one), 4), round(max(t_one), 4)],
           "stage_batch_profile_regions_ms_per_proof": regions, "stage_batch_device_regions_ms_per_proof": dev,
           "stage_batch_outside_regions_ms_per_proof": round(med(t_batch) / B - dev, 4),
           "engine_clock_mhz": clock, "proof_bytes": len(want[0])}
    print(json.dumps(res), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, default=13)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one batch size may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help="(internal) measure this batch size in this process")
    a = ap.parse_args()
    if a.one is not None:
        sys.exit(one_batch(a, a.one))
    lines = []
    for B in [int(x) for x in a.batches.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--degree-bits", str(a.degree_bits),
               "--reps", str(a.reps), "--one", str(B)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print("batch %d: exit status %d; nothing more is started on the GPU" % (B, r.returncode))
            sys.stdout.write(r.stdout[-2000:])
            sys.exit(r.returncode or 1)
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("$ python tools/stage_batch_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
