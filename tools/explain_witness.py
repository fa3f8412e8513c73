#!/usr/bin/env python3
"""Explain an unsatisfied witness from files: which gate constraints fail on which rows, which copy constraints are broken.

The first proof attempt on a pack from the fork will most likely end in QPGPU_EUNSAT "gate constraints fail at row N"; this
prints what qpgpu_circuit_explain_witness (include/qpgpu.h) finds instead: row, gate (named as tools/pack_dump.py names it),
constraint index and value, and for a copy constraint both cells with their values. Needs the MI355X (the gate kernels that judge
the witness produce the values); no torch.

usage: explain_witness.py PACK WIRES [PIS] [--max-rows N] [--cap N]
  PACK   circuit pack, little-endian u64 words (what pack_dump.py reads)
  WIRES  the witness, little-endian u64 words, [num_wires][2^degree_bits] (the layout qpgpu_prove takes)
  PIS    the public inputs, little-endian u64 words (omit for a circuit without any)
exit status: 0 satisfied, 1 findings printed, 2 usage or library error. The output holds witness values: treat it like the witness."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    opts = {"--max-rows": 8, "--cap": 4096}
    files = []
    i = 0
    while i < len(argv):
        if argv[i] in opts:
            if i + 1 >= len(argv):
                raise SystemExit(__doc__)
            opts[argv[i]] = int(argv[i + 1]); i += 2
        else:
            files.append(argv[i]); i += 1
    if len(files) not in (2, 3):
        raise SystemExit(__doc__)
    import __graft_entry__ as g
    pkg = g.load_package()
    pack = np.fromfile(files[0], dtype="<u8")
    h = pkg.pack_header(pack)
    num_wires, n = int(h["num_wires"]), 1 << int(h["degree_bits"])
    wires = np.fromfile(files[1], dtype="<u8")
    if wires.size != num_wires * n:
        print("explain_witness: %s holds %d words, the pack's witness is %d x %d" % (files[1], wires.size, num_wires, n), file=sys.stderr)
        return 2
    pis = np.fromfile(files[2], dtype="<u8") if len(files) == 3 else np.zeros(0, dtype=np.uint64)
    if pis.size != int(h["num_public_inputs"]):
        print("explain_witness: %d public inputs given, the pack has %d" % (pis.size, int(h["num_public_inputs"])), file=sys.stderr)
        return 2
    try:
        with pkg.QpGpu(0) as gpu:
            circ = pkg.Circuit(gpu, pack)
            try:
                found, rows, copies = circ.explain_witness(wires.reshape(num_wires, n), pis, max_rows=opts["--max-rows"], cap=opts["--cap"])
            finally:
                circ.close()
    except pkg.QpGpuError as e:
        print("explain_witness: %s" % e, file=sys.stderr)
        return 2
    for f in found:
        print(pkg.format_finding(pack, f))
    gate_rows = len(set(f.row for f in found if f.kind == pkg.FINDING_GATE))
    print("%d row(s) with failing gate constraints (%d expanded), %d copy mismatch(es) (%d shown)"
          % (rows, gate_rows, copies, sum(1 for f in found if f.kind == pkg.FINDING_COPY)))
    return 1 if rows or copies else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
