#!/usr/bin/env python3
"""Counters of the largest launch of every NTT kernel (the wires commitment of a lockstep batch) from rocprofv3 --pmc
--output-format csv passes over examples/leaf_prove_example.c (one worker, lockstep 32, 2^13 rows).
usage: lde_column_pmc_summary.py <label> <counter_collection.csv> [...]   -> JSON on stdout"""
import csv, json, sys
from collections import defaultdict

label, paths = sys.argv[1], sys.argv[2:]
vals = defaultdict(lambda: defaultdict(list))     # kernel -> counter -> values of its largest launches, scaled to the largest grid seen
name = lambda r: r["Kernel_Name"].split("(anonymous namespace)::")[-1].split("(")[0]
files = [[r for r in csv.DictReader(open(path, newline="")) if "ntt_" in r["Kernel_Name"]] for path in paths]
grid = {}
for rows in files:
    for r in rows:
        grid[name(r)] = max(grid.get(name(r), 0), int(r["Grid_Size"]))
for rows in files:
    own = {}                                      # the pool does not fill every batch: a pass may see 24 or 27 proofs, not 32
    for r in rows:
        own[name(r)] = max(own.get(name(r), 0), int(r["Grid_Size"]))
    for r in rows:
        k = name(r)
        if int(r["Grid_Size"]) != own[k]:
            continue
        f = grid[k] / own[k]
        vals[k][r["Counter_Name"]].append(float(r["Counter_Value"]) * f)
        vals[k]["duration_ns_under_pmc"].append((float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) * f)
        vals[k]["_meta"] = [int(r["Workgroup_Size"]), int(r["LDS_Block_Size"]), int(r["VGPR_Count"]), int(r["Scratch_Size"])]
out = {"source": f"rocprofv3 --kernel-trace --pmc <counters> --output-format csv -- leaf_prove_example 13 0 1 32 2, MI355X, {label}; "
                 "per kernel: mean over each pass's launches of its largest grid (the wires commitment), scaled linearly to the largest grid of all passes "
                 "(135 x 32 columns when a pass saw a full batch); FETCH_SIZE / WRITE_SIZE in KB",
       "kernels": {}}
for k, cs in sorted(vals.items()):
    wg, lds, vgpr, scratch = cs.pop("_meta")
    e = {"grid_threads": grid[k], "workgroup": wg, "lds_bytes": lds, "vgpr": vgpr, "scratch": scratch}
    for c, v in sorted(cs.items()):
        e[c] = round(sum(v) / len(v), 1)
    out["kernels"][k] = e
print(json.dumps(out, indent=1))
