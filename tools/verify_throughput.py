#!/usr/bin/env python3
"""Batch verification throughput: host verify_many on 16 threads against the device path (qpgpu_verifier_verify_many_device,
query rounds on the GPU, head on 16 host threads), bench-shape proofs (2^13 rows, 135 wires, 80 routed, Poseidon, made by
TemplateProver.prove_many) replicated to B proofs. One JSON line per B: proofs/s of both, the device path's split (host head,
upload, kernels + read-back, reason assembly; from a separate profiled call) and whether every verdict agrees. No torch, nothing
from oracle/: usable under rocprofv3 --kernel-trace --stats. Usage: verify_throughput.py [B,B,...] (default 8,64,1024)

verify_throughput.py --head [B,B,...] [threads,threads,...] (default 8,64,1024 and 16,2): the host head against the device head
(qpgpu_verifier_verify_many_device_ex, QPGPU_VERIFY_HEAD_ON_DEVICE), calls ALTERNATED in one run; one JSON line per (B,
threads) with every call's time, the medians, the device head's split (copy, upload, transcript kernel, identity kernels,
query kernels) and `device_head_wins`: every device-head call faster than every host-head call of the run."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

THREADS = 16
SPLIT = ("head", "upload", "kernels", "reasons")


def head_main(argv):
    sizes = [int(x) for x in (argv[0] if argv else "8,64,1024").split(",")]
    thread_counts = [int(x) for x in (argv[1] if len(argv) > 1 else "16,2").split(",")]
    pkg = ge.load_package()
    agg = pkg.aggregation
    gpu = pkg.QpGpu(0)
    pack, wires, _ = pkg.synth_circuit(13, num_wires=135, num_routed=80, num_public_inputs=21, seed=1000, poseidon=True, base_sum=True)
    tp = agg.TemplateProver(gpu, pack, wires, max_batch=8)
    tp.commit_many([agg.leaf_public_inputs(i) for i in range(8)])
    base = tp.prove_many()
    v = pkg.Verifier(pack, circuit=tp.circ)
    lib = v.lib
    for B in sizes:
        proofs = [base[i % len(base)] for i in range(B)]
        ptrs = (ctypes.c_char_p * B)(*proofs)
        lens = (ctypes.c_size_t * B)(*[len(p) for p in proofs])
        res = [(ctypes.c_int * B)(), (ctypes.c_int * B)()]
        rows = ctypes.create_string_buffer(200 * B)
        err = ctypes.create_string_buffer(200)
        for threads in thread_counts:
            def call(flags):
                t0 = time.perf_counter()
                rc = lib.qpgpu_verifier_verify_many_device_ex(v.h, gpu.ctx, ptrs, lens, B, threads, flags, res[flags], rows, err)
                dt = time.perf_counter() - t0
                assert rc == 0, (rc, err.value)
                return dt * 1e3
            call(0); call(1)                                 # workspace sized once
            reps = 5 if B >= 512 else 9
            times = [[], []]
            for _ in range(reps):
                for flags in (0, 1):
                    times[flags].append(round(call(flags), 3))
            split = {}
            for flags, keys in ((0, ("head", "upload", "kernels")), (1, ("copy", "upload", "transcript", "identity", "query", "kernels"))):
                gpu.profile(True)
                call(flags)
                split["device_head" if flags else "host_head"] = {k: round(gpu.profile_read("verify_many_device." + k)[0], 3) for k in keys}
                gpu.profile(False)
            print(json.dumps({
                "B": B, "threads": threads, "proof_bytes": len(base[0]),
                "host_head_ms": times[0], "device_head_ms": times[1],
                "host_head_median_ms": statistics.median(times[0]), "device_head_median_ms": statistics.median(times[1]),
                "device_head_wins": max(times[1]) < min(times[0]), "split_ms": split,
                "verdicts_equal": list(res[0]) == list(res[1]) and all(r == 0 for r in res[1]),
            }), flush=True)
    v.close(); tp.close(); gpu.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--head":
        return head_main(sys.argv[2:])
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "8,64,1024").split(",")]
    pkg = ge.load_package()
    agg = pkg.aggregation
    gpu = pkg.QpGpu(0)
    pack, wires, _ = pkg.synth_circuit(13, num_wires=135, num_routed=80, num_public_inputs=21, seed=1000, poseidon=True, base_sum=True)
    tp = agg.TemplateProver(gpu, pack, wires, max_batch=8)
    tp.commit_many([agg.leaf_public_inputs(i) for i in range(8)])
    base = tp.prove_many()
    v = pkg.Verifier(pack, circuit=tp.circ)
    lib = v.lib
    for B in sizes:
        proofs = [base[i % len(base)] for i in range(B)]
        ptrs = (ctypes.c_char_p * B)(*proofs)
        lens = (ctypes.c_size_t * B)(*[len(p) for p in proofs])
        res_h, res_d = (ctypes.c_int * B)(), (ctypes.c_int * B)()
        rows = ctypes.create_string_buffer(200 * B)
        err = ctypes.create_string_buffer(200)

        def host():
            return lib.qpgpu_verifier_verify_many(v.h, ptrs, lens, B, THREADS, res_h, err)

        def device():
            return lib.qpgpu_verifier_verify_many_device(v.h, gpu.ctx, ptrs, lens, B, THREADS, res_d, rows, err)

        def timed(fn, reps):
            out = []
            for _ in range(reps):
                t0 = time.perf_counter()
                rc = fn()
                out.append(time.perf_counter() - t0)
                assert rc in (0, -6), (rc, err.value)
            return statistics.median(out)

        reps = 3 if B >= 512 else 7
        device()                                            # workspace sized once
        t_host = timed(host, reps)
        t_dev = timed(device, reps)
        gpu.profile(True)
        device()
        split = {k: round(gpu.profile_read("verify_many_device." + k)[0], 3) for k in SPLIT}
        gpu.profile(False)
        print(json.dumps({
            "B": B, "proof_bytes": len(base[0]), "threads": THREADS,
            "host_proofs_per_s": round(B / t_host, 1), "device_proofs_per_s": round(B / t_dev, 1),
            "speedup": round(t_host / t_dev, 2), "host_ms": round(t_host * 1e3, 2), "device_ms": round(t_dev * 1e3, 2),
            "device_split_ms": split, "verdicts_equal": list(res_h) == list(res_d) and all(r == 0 for r in res_d),
        }), flush=True)
    v.close(); tp.close(); gpu.close()


if __name__ == "__main__":
    main()
