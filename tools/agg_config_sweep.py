"""The reference's aggregation-config sweep (wormhole/memprof: AggConfigArgs over the private-batch circuit) on the device.

Input: tests/golden/memprof_sweep_grid.json, the rows the reference recorded (sweep, label, peak_mb, wall_ms, args). Every row's
flags go through the reference's knob policy on the host (qpgpu_agg_config_validate / _build); the private-batch circuit (complete
in-circuit verifier + build_private_batch_constraints) is built under the resulting config over the restated leaf circuit padded to
2^13 rows at the row's --num-leaf-proofs, loaded, and proven once warm and five times timed. Printed per row: the effective config,
degree bits, rows before blinding and padding, blinding rows, proof bytes, build seconds, median prove ms, and the bytes the
context's buffer registry tracks once the circuit is loaded (qpgpu_ctx_residue_scan over every region with one needle >= 2^32: its
byte total is the registry's; one context serves every row and its scratch and pinned regions stay at their high-water mark, so equal
configs differ by what earlier rows left). Rows this backend cannot run are printed with the refusal's text. Nothing is compared against a
threshold: the output is the record (profiles/agg_config_sweep.txt).

usage: python tools/agg_config_sweep.py [--rows FIRST:LAST] [--jobs J] [--leaf-degree-bits 13]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "memprof_sweep_grid.json")
CONFIG_KEYS = ("zero_knowledge", "num_wires", "num_routed_wires", "max_quotient_degree_factor", "security_bits", "num_challenges", "rate_bits", "cap_height", "num_query_rounds")
_tiny = {}


def builder_refusal(pkg, config):
    """The text qpgpu_wrapper_circuit_build_cfg refuses `config` with, or None. Asked of a one-proof wrapper over the fake leaf without
    the arithmetic half: a refusal comes before anything is laid out, and the tool only asks when it expects one."""
    if "fake" not in _tiny:
        _tiny["fake"] = pkg.leaf.LeafCircuit(fragment=pkg.leaf.FRAGMENT_FAKE_LEAF)
        _tiny["ver"] = pkg.Verifier(_tiny["fake"].pack)
    try:
        pkg.recursion.WrapperCircuit(_tiny["fake"].pack, _tiny["ver"], 1, logic="private_batch", config=config)
    except pkg.QpGpuError as e:
        return str(e)
    return None


def plan_row(pkg, row):
    """{refusal, kind, config, num_leaf_proofs, real_proofs}: what the tool does with one recorded row. refusal: None, or the text the
    row is printed with (kind: "polyfri", "rayon_threads", "validate", "max_quotient_degree_factor" or "builder")."""
    plan = dict(refusal=None, kind=None, config=None, num_leaf_proofs=None, real_proofs=1)
    if "polyfri" in row["label"]:
        plan.update(kind="polyfri", refusal="zk mode polyfri: the fork's second zero-knowledge mode is un-vendored; this backend builds rowblinding "
                                            "(upstream CircuitBuilder::blind's rows) or disabled")
        return plan
    try:
        args, other = pkg.parse_agg_config_flags(row["args"].split())
    except ValueError as e:
        plan.update(kind="flags", refusal=str(e))
        return plan
    plan["num_leaf_proofs"] = int(other.get("num_leaf_proofs", 16))
    plan["real_proofs"] = int(other.get("real_proofs", 1))
    if "rayon_threads" in other:
        plan.update(kind="rayon_threads", refusal="--rayon-threads %s: a knob of the CPU prover's host thread pool; the device prover has no such pool to size" % other["rayon_threads"])
        return plan
    why = pkg.agg_config_validate(args)
    if why is not None:
        plan.update(kind="validate", refusal=why)
        return plan
    plan["config"] = pkg.agg_config_build(args)
    if plan["config"].max_quotient_degree_factor != 8:
        plan.update(kind="max_quotient_degree_factor", refusal=builder_refusal(pkg, plan["config"]))
    return plan


def config_text(c):
    d = c.as_dict()
    return " ".join("%s=%d" % (k, d[k]) for k in CONFIG_KEYS) + " fri.product=%d" % (d["rate_bits"] * d["num_query_rounds"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=":", help="FIRST:LAST (0-based, LAST exclusive) of the fixture's rows")
    ap.add_argument("--jobs", type=int, default=8, help="host threads that build circuits ahead of the device")
    ap.add_argument("--leaf-degree-bits", type=int, default=13)
    ap.add_argument("--timed", type=int, default=5)
    opt = ap.parse_args()
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import leaf_cases as lc
    from concurrent.futures import ThreadPoolExecutor
    pkg = ge.load_package()
    L, R = pkg.leaf, pkg.recursion
    from qp_zk_circuits_amd.binding import residue_regions
    with open(FIXTURE) as f:
        rows = json.load(f)["rows"]
    first, last = (opt.rows.split(":") + [""])[:2]
    first, last = int(first or 0), int(last or len(rows))
    picked = list(range(first, min(last, len(rows))))
    plans = {i: plan_row(pkg, rows[i]) for i in picked}

    gpu = pkg.QpGpu(0)
    leaf = L.LeafCircuit(min_degree_bits=opt.leaf_degree_bits)
    lp = L.LeafProver(pkg, gpu, leaf)
    lver = pkg.Verifier(leaf.pack, circuit=lp.circ)
    max_real = max([p["real_proofs"] for p in plans.values() if p["refusal"] is None] + [1])
    real = [lp.prove(x)[0] for x in lc.shared_tree_inputs(L, max_real)]
    dummy = lp.prove(L.dummy_circuit_inputs())[0]
    assert all(lver.verify(p) for p in real + [dummy])
    print("# aggregation-config sweep: private-batch circuit over the restated leaf (2^%d rows, proof %d bytes), one MI355X" % (leaf.info["degree_bits"], len(dummy)))
    print("# reference columns (peak_mb, wall_ms): the fork's circuit on a CPU, recorded in its sweep-results/data.csv; they are here for the SHAPE of the curve only")
    print("# build_s: host seconds of one qpgpu_wrapper_circuit_build_cfg call pair (size query + build), %d builds running side by side" % opt.jobs)

    def build(i):
        p = plans[i]
        if p["refusal"] is not None:
            return None
        t0 = time.perf_counter()
        try:
            w = R.WrapperCircuit(leaf.pack, lver, p["num_leaf_proofs"], logic="private_batch", verify=True, config=p["config"])
        except pkg.QpGpuError as e:
            p.update(kind="builder", refusal=str(e))
            return None
        return w, time.perf_counter() - t0

    with ThreadPoolExecutor(max_workers=max(1, opt.jobs)) as ex:
        built = dict(zip(picked, ex.map(build, picked)))
    mask = (1 << len(residue_regions())) - 1
    for i in picked:
        row, p = rows[i], plans[i]
        head = "row %2d  %-16s %-18s" % (i, row["sweep"], row["label"])
        ref = "reference peak_mb=%.1f wall_ms=%d" % (row["peak_mb"], row["wall_ms"])
        if p["refusal"] is not None:
            print("%s NOT RUN (%s): %s | %s | args: %s" % (head, p["kind"], p["refusal"], ref, row["args"]), flush=True)
            continue
        w, build_s = built[i]
        N = p["num_leaf_proofs"]
        k = min(p["real_proofs"], N)
        slots = real[:k] + [dummy] * (N - k)
        pre = np.random.default_rng(i).integers(0, 1 << 63, (N, 4), dtype=np.uint64)
        try:
            circ = pkg.Circuit(gpu, w.pack)
        except pkg.QpGpuError as e:
            print("%s NOT RUN (load): %s | %s | %s" % (head, e, config_text(p["config"]), ref), flush=True)
            continue
        _, _, tracked = gpu.residue_scan(np.array([1 << 40], dtype=np.uint64), regions=mask, cap=0)
        d = gpu.alloc(8 * (w.num_wires << w.info["degree_bits"]))
        ver = pkg.Verifier(w.pack, circuit=circ)
        ms, proof = [], None
        for r in range(1 + opt.timed):
            com = w.commit(slots, preimages=pre, device_blinding=True, derive_public_inputs=True)
            t0 = time.perf_counter()
            st = R.generate_wrapper_witnesses(circ, w, [com], d)
            if any(st):
                raise pkg.QpGpuError(-4, gpu.last_error())
            proof = circ.prove_dev(d, circ.witness_public_inputs_dev(d)[0])
            ms.append(1e3 * (time.perf_counter() - t0))
        ok = ver.verify(proof)
        print("%s %s | degree_bits=%d rows=%d blinding_rows=%d proof_bytes=%d build_s=%.2f prove_ms_median=%.1f (warm-up %.1f) registry_bytes=%d verified=%s | %s"
              % (head, config_text(p["config"]), w.info["degree_bits"], w.info["rows_before_padding"], w.info["rows_blinding"], len(proof), build_s,
                 statistics.median(ms[1:]), ms[0], tracked, "yes" if ok else "NO: " + ver.reason, ref), flush=True)
        ver.close(); circ.close(); d.free(scrub=True)
        built[i] = None
    lver.close(); lp.close(); gpu.close()


if __name__ == "__main__":
    main()
