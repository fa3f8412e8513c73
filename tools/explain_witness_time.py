"""Wall time of qpgpu_circuit_explain_witness (include/qpgpu.h) with one flipped cell, at max_rows 1 and 64, beside the cost of the
witness-check pass on the same pack (qpgpu_prove_dev with the check on minus off): the 2^13-row leaf pack and a 2^17-row pack. One MI355X.
usage: python tools/explain_witness_time.py [OUTPUT.txt]      (profiles/witness_explain.txt is its output)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
pkg = g.load_package()
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
def say(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n"); out.flush()
def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); f(); ts.append((time.perf_counter() - t) * 1e3)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)
def run(gpu, name, pack, wires, pis, hash_type):
    h = pkg.pack_header(pack)
    n = 1 << h["degree_bits"]
    circ = pkg.Circuit(gpu, pack)
    try:
        row = int(circ.gate_rows(hash_type)[0])
        bad = wires.copy(); bad[h["num_wires"] - 1, row] ^= np.uint64(1)
        d_ok, d_bad = gpu.to_device(wires), gpu.to_device(bad)
        assert circ.explain_witness(d_ok, pis) == ([], 0, 0)
        f1 = circ.explain_witness(d_bad, pis, max_rows=1)
        assert f1[1] == 1 and f1[2] == 0 and f1[0] and all(x.row == row for x in f1[0]), f1[1:]
        say("%s: 2^%d rows x %d wires, %d gate constraints, %d challenges; one flipped cell (row %d, wire %d) -> %d findings"
            % (name, h["degree_bits"], h["num_wires"], h["num_gate_constraints"], h["num_challenges"], row, h["num_wires"] - 1, len(f1[0])))
        for mr in (1, 64):
            m = med(lambda: circ.explain_witness(d_bad, pis, max_rows=mr), 7)
            say("  explain_witness wires_on_device=1 max_rows=%-3d  median %.3f ms (min %.3f, max %.3f) of 7" % ((mr,) + m))
        m = med(lambda: circ.explain_witness(bad, pis, max_rows=1), 5)
        say("  explain_witness host wires        max_rows=1    median %.3f ms (min %.3f, max %.3f) of 5" % m)
        circ.prove_dev(d_ok, pis)
        off = med(lambda: circ.prove_dev(d_ok, pis), 5)
        circ.set_witness_check(True)
        circ.prove_dev(d_ok, pis)
        on = med(lambda: circ.prove_dev(d_ok, pis), 5)
        circ.set_witness_check(False)
        say("  prove_dev, witness check off / on               median %.3f / %.3f ms of 5: the check pass costs %.3f ms" % (off[0], on[0], on[0] - off[0]))
        d_ok.free(scrub=True); d_bad.free(scrub=True)
    finally:
        circ.close()
with pkg.QpGpu(0) as gpu:
    try:
        import leaf_cases
        lcirc = pkg.leaf.LeafCircuit(min_degree_bits=13)
        lp = pkg.leaf.LeafProver(pkg, gpu, lcirc)
        x = leaf_cases.dummy_inputs(pkg.leaf)
        lp.prove(x); wires = lp.witness().copy(); lp.close()
        run(gpu, "leaf pack", lcirc.pack, wires, lcirc.commit(x)[2], 14)
    except Exception as e:
        say("leaf pack: FAILED %r" % (e,))
    try:
        pack, wires, pis = pkg.synth_circuit(17, seed=5, poseidon=True, base_sum=True, ext_arith=True, recursion=True, poseidon2=True)
        run(gpu, "synthetic 15-gate pack (stand-in for a private-batch pack of the same size)", pack, wires, pis, 4)
    except Exception as e:
        say("synthetic pack: FAILED %r" % (e,))
if out:
    out.close()
