#!/usr/bin/env python3
"""Time of FRI-level verification at the bench shape: the FRI parts of leaf-shaped proofs (2^13 rows, 135 wires, 80 routed,
Poseidon, made by TemplateProver.prove_many), sliced out and described as a 4-oracle, 2-batch instance, in batches of 64 and 1024.
Three ways, alternated in one session, three rounds, min and max of each:
  device   qpgpu_fri_verify_many_device, the whole call (host checks, upload, kernels, read-back) and its query-round kernels alone
  host     qpgpu_fri_verify, the proofs spread over 16 host threads
  special  the query-round kernels of qpgpu_verifier_verify_many_device (verify_kernels.hip, welded to the Plonk layout) on the
           whole proofs the FRI parts were cut from
Writes profiles/fri_verify.txt (or the file named as the second argument). No threshold: a record, not a check.
Usage: fri_verify_time.py [B,B,...] [out]"""
import concurrent.futures
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import fri_verify_model as fm  # noqa: E402  (the slicing of a whole proof; nothing of the model's arithmetic is used here)

THREADS, ROUNDS = 16, 3


def fri_view(pkg, pack, proof, cs_cap):
    """The FRI part of a whole proof as qpgpu_fri_verify takes it (tests/fri_verify_model.py: plonk_view, the transcript of
    plonky2's prove() replayed up to the point FRI begins). The public-input hash it needs is hash_no_pad of the proof's last
    words: the sponge's first four words after absorbing them."""
    n_pis = pkg.pack_header(pack)["num_public_inputs"]
    hc = pkg.Challenger(); hc.observe(np.frombuffer(proof, dtype="<u8", count=n_pis, offset=len(proof) - 8 * n_pis))
    return fm.plonk_view(pkg, pack, proof, np.array(hc.get_n(8)[::-1][:4], dtype=np.uint64), cs_cap)


def main():
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "64,1024").split(",")]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fri_verify.txt")
    pkg = ge.load_package()
    agg = pkg.aggregation
    gpu = pkg.QpGpu(0)
    pack, wires, _ = pkg.synth_circuit(13, num_wires=135, num_routed=80, num_public_inputs=21, seed=1000, poseidon=True, base_sum=True)
    tp = agg.TemplateProver(gpu, pack, wires, max_batch=8)
    tp.commit_many([agg.leaf_public_inputs(i) for i in range(8)])
    base = tp.prove_many()
    ver = pkg.Verifier(pack, circuit=tp.circ)
    assert all(ver.verify_many(base))
    cs_cap = tp.circ.constants_sigmas_cap(int(pack[11]))
    views = [fri_view(pkg, pack, p, cs_cap) for p in base]
    h = views[0]["header"]
    fv = pkg.FriVerifier(h["degree_bits"], views[0]["oracles"], views[0]["batches"], views[0]["lay"].arity_bits, rate_bits=h["rate_bits"],
                         cap_height=h["cap_height"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"])
    for v in views:
        v["chal"] = fv.challenges(v["challenger"], v["fri"])
        assert fv.verify(v["caps"], v["points"], v["openings"], *v["chal"], v["fri"]), fv.reason
    lib, lines = fv.lib, []
    for B in sizes:
        vs = [views[i % len(views)] for i in range(B)]
        # both calls' arguments are marshalled once, outside the timers: the figures are the library's, not the binding's
        u64 = lambda x: np.ascontiguousarray(np.array(x, dtype=np.uint64))      # noqa: E731
        d_caps = [u64(vs[0]["caps"][0]).reshape(-1)] + [u64([np.asarray(v["caps"][o]).reshape(-1) for v in vs]) for o in (1, 2, 3)]
        d_arr = [u64([[v["points"][b] for v in vs] for b in range(2)]), u64([v["openings"] for v in vs]), u64([v["chal"][0] for v in vs]),
                 u64([v["chal"][1] for v in vs]), u64([v["chal"][2] for v in vs]), u64([v["chal"][3] for v in vs])]
        d_cptr = (ctypes.c_void_p * 4)(*[k.ctypes.data for k in d_caps])
        d_counts = (ctypes.c_uint32 * 4)(1, B, B, B)          # the constants/sigmas cap is shared, as in an aggregation level
        d_proofs = (ctypes.c_char_p * B)(*[v["fri"] for v in vs])
        d_lens = (ctypes.c_size_t * B)(*[len(v["fri"]) for v in vs])
        d_res, d_rows, d_err = (ctypes.c_int * B)(), ctypes.create_string_buffer(200 * B), ctypes.create_string_buffer(200)
        wholes = [base[i % len(base)] for i in range(B)]
        # qpgpu_fri_verify's arguments per proof
        single = []
        for v in vs:
            keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in v["caps"]]
            arrs = [np.ascontiguousarray(np.array(x, dtype=np.uint64)) for x in (v["points"], v["openings"], v["chal"][0], v["chal"][1], v["chal"][3])]
            single.append((keep, (ctypes.c_void_p * 4)(*[k.ctypes.data for k in keep]), arrs, v["chal"][2], v["fri"]))

        def host_one(lo, hi):
            err = ctypes.create_string_buffer(200)
            for keep, cptr, (pts, ops, al, bt, ix), powr, fri in single[lo:hi]:
                assert lib.qpgpu_fri_verify(fv.h, cptr, pts.ctypes.data, ops.ctypes.data, al.ctypes.data, bt.ctypes.data, powr, ix.ctypes.data,
                                            fri, len(fri), err) == 0, err.value

        def host(pool):
            step = (B + THREADS - 1) // THREADS
            for f in [pool.submit(host_one, lo, min(B, lo + step)) for lo in range(0, B, step)]:
                f.result()

        def device():
            rc = lib.qpgpu_fri_verify_many_device(fv.h, gpu.ctx, B, d_cptr, d_counts, *[a.ctypes.data for a in d_arr], d_proofs, d_lens, d_res,
                                                  d_rows, d_err)
            assert rc == 0 and not any(d_res), (rc, d_err.value)

        def kernels(call, name):
            gpu.profile(True)
            call()
            ms = gpu.profile_read(name)[0]
            gpu.profile(False)
            return ms

        t = {k: [] for k in ("device_call_ms", "host_16_threads_ms", "generic_query_kernels_ms", "special_query_kernels_ms")}
        with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
            device(); host(pool); ver.verify_many(wholes, threads=THREADS, gpu=gpu)          # workspaces sized, threads started
            for _ in range(ROUNDS):
                t0 = time.perf_counter(); device(); t["device_call_ms"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); host(pool); t["host_16_threads_ms"].append((time.perf_counter() - t0) * 1e3)
                t["generic_query_kernels_ms"].append(kernels(device, "fri_verify_many_device.query"))
                t["special_query_kernels_ms"].append(kernels(lambda: ver.verify_many(wholes, threads=THREADS, gpu=gpu), "verify_many_device.query"))
        rec = {"B": B, "fri_proof_bytes": len(vs[0]["fri"]), "rounds": ROUNDS}
        for k, xs in t.items():
            rec[k] = {"min": round(min(xs), 3), "max": round(max(xs), 3)}
        g, s = t["generic_query_kernels_ms"], t["special_query_kernels_ms"]
        rec["generic_over_special"] = round(min(g) / min(s), 3)
        rec["within_spread_of_special"] = min(g) <= max(s)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("FRI-level verification at the bench shape (tools/fri_verify_time.py): times in ms, min and max of %d alternated rounds.\n"
                "device_call: qpgpu_fri_verify_many_device, the whole call. host_16_threads: qpgpu_fri_verify spread over 16 host threads.\n"
                "generic / special query kernels: the two launches of fri_verify_kernels.hip / verify_kernels.hip between HIP events, same proofs.\n" % ROUNDS)
        f.write("\n".join(lines) + "\n")
    fv.close(); ver.close(); tp.close(); gpu.close()


if __name__ == "__main__":
    main()
