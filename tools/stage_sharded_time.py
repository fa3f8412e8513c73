"""qpgpu_stage_quotient at a 2^13-row hash-gate pack (Poseidon and base-sum rows, rate_bits 3) on a plan of one context against the
same call on a plan over coset-sharded oracles (qpgpu_stage_plan_create_sharded) at G = 2, 4, 8, and the merge kernel on its own.

  stage_sharded_time.py [--degree-bits 13] [--shards 2 4 8] [--reps 10] [--out profiles/stage_sharded.txt]

The shards run on one context per visible device where there are at least G devices, otherwise all on device 0: then they share that
device, the sharded figures say what the split costs and not what it gains, and the output says in its first lines that the
multi-device time is unmeasured. The call time is a host clock around qpgpu_stage_quotient, which has synchronised every stream when
it returns; two warm-up calls of each plan, then plain and sharded alternated call by call, medians and ranges of --reps calls. The
chunks are compared with the plain plan's every time. The merge kernel's own time comes from a second series with the home
context's event timing on (qpgpu_profile_enable, "prove_quotient_merge"); beside it a device-to-device copy of the bytes the kernel
moves (it reads num_challenges * Nq words and writes as many: a copy of that many words moves the same bytes), timed with events in
the same process. Not a pass/fail figure. No GPU: it fails, it does not fall back."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

P = 0xFFFFFFFF00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, default=13)
    ap.add_argument("--shards", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stage_sharded_time: no GPU visible")
    pkg = ge.load_package()
    ndev = torch.cuda.device_count()
    head = ["devices visible: %d" % ndev]
    d, n = a.degree_bits, 1 << a.degree_bits
    pack, wires, pis = pkg.synth_circuit(d, seed=62, poseidon=True, base_sum=True)
    hdr = pkg.pack_header(pack)
    rate, cap_h, nch = hdr["rate_bits"], hdr["cap_height"], hdr["num_challenges"]
    ncs = hdr["num_selectors"] + hdr["num_constants"] + hdr["num_routed_wires"]
    end = 18 + hdr["num_arity_rounds"] + 8 * hdr["num_gates"] + hdr["num_routed_wires"] + 4
    cs = np.ascontiguousarray(pack[end:end + ncs * n].reshape(ncs, n))
    kw = dict(rate_bits=rate, cap_height=cap_h)
    rng = np.random.default_rng(5)
    betas, gammas, alphas = (rng.integers(1, P, size=nch, dtype=np.uint64) for _ in range(3))
    lines = []

    def flow(gpus):
        """The oracles and the plan of one route, up to the point where the quotient can be called; (call, close)."""
        home = gpus[0]
        commit = (lambda x, **k: pkg.PolyOracle(home, x, **kw, **k)) if len(gpus) == 1 else (lambda x, **k: home.commit_sharded(gpus, x, **kw, **k))
        o_cs = commit(cs)
        plan = pkg.StagePlan(home, pack, o_cs) if len(gpus) == 1 else pkg.StagePlan.create_sharded(home, pack, o_cs)
        o_w = commit(wires)
        d_zs = plan.partial_products(wires, betas, gammas)
        o_zs = commit((d_zs, plan.num_zs_pp, n))
        ch = pkg.Challenger(home)
        ch.observe(np.asarray(pis, dtype=np.uint64) % np.uint64(P)); ch.get()
        pih = np.array(list(ch.state.sponge_state)[:4], dtype=np.uint64)

        d_out = home.alloc(plan.num_quotient * n * 8)        # allocated once: the clock sees the call alone

        def call():
            t0 = time.perf_counter()
            rc = home.lib.qpgpu_stage_quotient(plan.h, o_w.h, o_zs.h, betas.ctypes.data, gammas.ctypes.data, alphas.ctypes.data, pih.ctypes.data, d_out.ptr)
            ms = 1e3 * (time.perf_counter() - t0)
            home._check(rc)
            return ms, d_out.download().copy()

        def close():
            d_out.free(); o_zs.close(); d_zs.free(); o_w.close(); plan.close(); o_cs.close()
        return plan, call, close

    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    one = pkg.QpGpu(0)
    plain_plan, plain_call, plain_close = flow([one])
    factor = plain_plan.quotient_degree_factor
    nq_words = nch * factor * n
    for G in a.shards:
        devs = list(range(G)) if ndev >= G else [0] * G
        if ndev < G:
            head.append("G = %d: %d device(s), the shards are contexts of device 0 and share it; the multi-device time is UNMEASURED" % (G, ndev))
        gpus = [one] + [pkg.QpGpu(dv) for dv in devs[1:]]
        plan, call, close = flow(gpus)
        for _ in range(2):
            want = plain_call()[1]
            assert np.array_equal(call()[1], want), "the sharded chunks differ"
        ta, tb = [], []
        for _ in range(a.reps):
            x = plain_call(); ta.append(x[0])
            y = call(); tb.append(y[0])
            assert np.array_equal(x[1], want) and np.array_equal(y[1], want)
        # the merge kernel alone: event timing on the home context, in calls of their own
        one.profile(True)
        before = one.profile_read("prove_quotient_merge")
        for _ in range(a.reps):
            call()
        after = one.profile_read("prove_quotient_merge")
        one.profile(False)
        launches = after[1] - before[1]
        merge_ms = (after[0] - before[0]) / launches if launches else None
        # the yardstick: a device-to-device copy that moves the same bytes (reads nq_words, writes nq_words)
        src = torch.empty(nq_words, dtype=torch.int64, device="cuda:0").random_()
        dst = torch.empty_like(src)
        copies = []
        for i in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); e1.synchronize()
            if i >= 2:
                copies.append(e0.elapsed_time(e1))
        moved = 2 * nq_words * 8
        rec = {"degree_bits": d, "rate_bits": rate, "quotient_degree_factor": factor, "num_challenges": nch, "shards": G, "devices": sorted(set(devs)),
               "reps": a.reps, "plain_quotient_wall_ms": stat(ta), "sharded_quotient_wall_ms": stat(tb),
               "merge_kernel_ms": None if merge_ms is None else round(merge_ms, 4), "merge_launches_timed": int(launches), "merge_bytes_moved": moved,
               "merge_GB_per_s": None if not merge_ms else round(moved / merge_ms / 1e6, 1),
               "d2d_copy_same_bytes_ms": stat(copies), "d2d_copy_GB_per_s": round(moved / float(np.median(copies)) / 1e6, 1)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        close()
        for c in gpus[1:]:
            c.close()
    plain_close()
    one.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(head) + "\n$ python tools/stage_sharded_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")
    print("\n".join(head))


if __name__ == "__main__":
    main()
