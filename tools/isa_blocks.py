#!/usr/bin/env python3
"""Vector instructions per basic block of the gfx950 kernels of one .hip file (or of an assembly file made with hipcc -S), in
program order, with the registers, scratch, occupancy and code size the compiler's kernel metadata states. Where isa_hist.py counts
a kernel as a whole, this shows WHERE a change removed instructions: loop bodies and straight-line sections keep their place, so
two trees' lines can be read side by side and loop trip counts applied per block. Blocks below --min instructions (default 30)
are summed: in the hashing kernels these are the out-of-line rare folds of the S-box products.
usage: isa_blocks.py <file.hip | file.s> [kernel-name substring] [--min N]"""
import os, re, subprocess, sys, tempfile
args = [a for a in sys.argv[1:]]
least = int(args.pop(args.index("--min") + 1)) if "--min" in args else 30
if "--min" in args:
    args.remove("--min")
src, sub = args[0], args[1] if len(args) > 1 else ""
if src.endswith(".s"):
    text = open(src).read()
else:
    with tempfile.TemporaryDirectory(prefix="isa_blocks_") as work:
        asm = os.path.join(work, os.path.basename(src) + ".s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-S", src, "-o", asm,
                               "-I", os.path.dirname(os.path.abspath(src))], stderr=subprocess.DEVNULL)
        text = open(asm).read()
for m in re.finditer(r"^(_Z\S+):\s*;[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel(.*?); codeLenInByte = (\d+)(.*?); Occupancy: (\d+)", text, re.S | re.M):
    name, body, meta = m.group(1), m.group(2), m.group(5)
    if sub and sub not in name:
        continue
    shown = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "")
    blocks, cur = [], 0
    for line in body.split("\n"):
        t = line.strip()
        if re.match(r"^\.LBB\S+:", t):
            blocks.append(cur); cur = 0
        elif t.startswith("v_"):
            cur += 1
    blocks.append(cur)
    get = lambda k: re.search(k + r": (\d+)", meta).group(1)
    print(f"{shown}: {sum(blocks)} vector instructions, {get('NumVgprs')} VGPRs, scratch {get('ScratchSize')} B/lane, {m.group(6)} waves/SIMD, code {m.group(4)} B")
    print(f"    blocks: {' '.join(str(c) for c in blocks if c >= least)} | {sum(1 for c in blocks if 0 < c < least)} blocks below {least}: {sum(c for c in blocks if c < least)}")
