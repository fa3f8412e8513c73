"""Two timers that share a name for historical reasons.

  leaf_time.py <label> [reps]
      Wall time of the wires-shaped commitment of one lockstep batch (2^21 leaves x 135 columns, cap height 4) and of its leaf level
      alone, host timers around a synchronised loop.

  leaf_time.py --config {leaf,zk} [--min-degree-bits N] [--rate-bits R] [--copies K|dense] [--hints] [--proofs N] [--workers W] [--max-batch B] [--pool-proofs N] [--batch-probe B]
      The leaf PROVER under a CircuitConfig (WormholeProver::new(config)): "leaf" is wormhole_leaf_circuit_config(), "zk" the
      zero-knowledge wormhole_private_batch_circuit_config() of the reference's prover_create_proof_zk bench target. Prints one JSON
      line: single-proof latency of commit -> stage s1 -> s2..s12 (median, host timer), the share of stage s1 (host timer around the
      synchronised witness call, which for a zero-knowledge circuit includes the draw and the scatter of the blinding cells, and the
      library's own "witness_generate" profile region, which covers the generator levels only), the rate of a pool of W workers in
      lockstep batches of B, dependency levels, blinding rows and cells, and the device memory one proof of a B-proof lockstep handle
      takes (free-memory difference around loading it).
      --copies K: the density-matched leaf of K copies (LeafCircuit(copies=K): a measurement object, K statements of which one is public);
      --copies dense: as many copies as fit 2^min-degree-bits rows. With copies, stage s1 is also timed for one witness and for a lockstep
      batch of --max-batch with QPGPU_WITNESS_WIDE_ROWS at 0 and at 1, alternated inside this one call on freshly loaded handles."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
pkg = ge.load_package()


def device_free_bytes():
    """hipMemGetInfo of the HIP runtime the library already runs on (found in this process's maps: no second runtime is loaded)."""
    import ctypes
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def prover_mode(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("leaf", "zk"), required=True)
    ap.add_argument("--min-degree-bits", type=int, default=0)
    ap.add_argument("--rate-bits", type=int, default=0, help="with --config leaf: the leaf config at another rate_bits (3..8)")
    ap.add_argument("--hints", action="store_true")
    ap.add_argument("--copies", default="1")
    ap.add_argument("--proofs", type=int, default=20)
    ap.add_argument("--workers", type=int, default=6)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--pool-proofs", type=int, default=384)
    ap.add_argument("--batch-probe", type=int, default=64)
    a = ap.parse_args(argv)
    L = pkg.leaf
    cfg = "private_batch" if a.config == "zk" else "leaf"
    if a.rate_bits:
        assert a.config == "leaf"
        cfg = pkg.circuit_config("leaf", rate_bits=a.rate_bits)
    c = L.LeafCircuit.dense(a.min_degree_bits, config=cfg) if a.copies == "dense" else L.LeafCircuit(min_degree_bits=a.min_degree_bits, config=cfg, copies=int(a.copies))
    x = L.dummy_circuit_inputs()
    out = {"config": a.config, "rate_bits": int(pkg.pack_header(c.pack)["rate_bits"]), "copies": c.copies, "rows_poseidon2": c.info["rows_poseidon2"], "hash_hints": a.hints, "degree_bits": c.info["degree_bits"], "rows_before_padding": c.info["rows_before_padding"],
           "blinding_cells": int(c.blinding_cells.size), "zero_knowledge": c.zero_knowledge}
    if c.zero_knowledge:
        routed = int(c.config.num_routed_wires)
        regular = int((c.blinding_cells % np.uint64(135) >= np.uint64(routed)).sum()) // (135 - routed)
        out["blinding_rows"] = regular + 2 * ((int(c.blinding_cells.size) - regular * 135) // routed)
    with pkg.QpGpu(0) as gpu:
        pr = L.LeafProver(pkg, gpu, c, hash_hints=a.hints)
        for _ in range(3):
            pr.prove(x)
        out["generator_instances"], out["dependency_levels"] = pr.circ.witness_info()[:2]
        lat, s1 = [], []
        for _ in range(a.proofs):
            gpu.sync(); t0 = time.perf_counter()
            pr.generate_witness(x); gpu.sync(); t1 = time.perf_counter()
            pr.prove(x); gpu.sync(); t2 = time.perf_counter()
            s1.append(t1 - t0); lat.append(t2 - t1)
        out["single_proof_ms"] = round(1e3 * float(np.median(lat)), 3)
        out["stage_s1_ms"] = round(1e3 * float(np.median(s1)), 3)
        gpu.profile(True)
        for _ in range(5):
            pr.generate_witness(x)
        gpu.sync()
        ms, n = gpu.profile_read("witness_generate")
        out["witness_generate_region_ms"] = round(ms / max(n, 1), 3)
        gpu.profile(False)
        pr.close()
        if c.copies > 1 and not c.zero_knowledge:
            from witness_wide_rows_ab import wide_rows_ab      # tools/ is this script's directory
            cells, values, pis = c.commit(x, hash_hints=a.hints)
            out["stage_s1_wide_rows_ab_ms"] = wide_rows_ab(pkg, gpu, c.pack, c.info["degree_bits"], cells, values, pis, a.max_batch)
        free0 = device_free_bytes()
        big = pkg.Circuit(gpu, c.pack, max_batch=a.batch_probe)
        cells = c.commit(x, hash_hints=a.hints, device_blinding=c.zero_knowledge)[0]
        big.witness_partial_prepare(cells, a.batch_probe)
        gpu.sync()
        out["lockstep_%d_device_bytes_per_proof" % a.batch_probe] = int((free0 - device_free_bytes()) // a.batch_probe)
        big.close()
        pr = L.LeafProver(pkg, gpu, c, hash_hints=a.hints)
        pool = pr.pool(workers=a.workers, max_batch=a.max_batch)
        for t in [pr.submit(pool, x) for _ in range(a.workers * a.max_batch)]:
            pool.wait(t, copy=False)
        t0 = time.perf_counter()
        for t in [pr.submit(pool, x) for _ in range(a.pool_proofs)]:
            pool.wait(t, copy=False)
        dt = time.perf_counter() - t0
        pool.close(); pr.close()
        out["pool"] = {"workers": a.workers, "max_batch": a.max_batch, "proofs": a.pool_proofs, "proofs_per_s": round(a.pool_proofs / dt, 1)}
    print(json.dumps(out))


if any(v.startswith("--config") for v in sys.argv[1:]):
    prover_mode(sys.argv[1:])
    sys.exit(0)
gpu = pkg.QpGpu(0)
LOG, W = 21, 135
n = 1 << LOG
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
cols = gpu.alloc(n * W * 8)
rng = np.random.default_rng(1)
for c in range(W):
    chunk = rng.integers(0, pkg.P, n, dtype=np.uint64)
    gpu._check(gpu.lib.qpgpu_memcpy_h2d(gpu.ctx, cols.ptr + c * n * 8, chunk.ctypes.data, n * 8))
dig = gpu.alloc(gpu.merkle_digest_count(LOG, 4) * 32)
cap = gpu.merkle_build_dev(cols, n, W, LOG, 4, dig)
gpu.sync()
t0 = time.perf_counter()
for _ in range(reps):
    gpu.merkle_build_dev(cols, n, W, LOG, 4, dig)
gpu.sync()
ms = (time.perf_counter() - t0) / reps * 1e3
perms = n * 17 + n - 16
print(json.dumps({"label": sys.argv[1], "tree_ms": round(ms, 3), "G_perm_per_s": round(perms / ms / 1e6, 3), "cap0": hex(int(cap[0][0]))}))
