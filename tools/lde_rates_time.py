"""Device time of coset LDEs (qpgpu_lde_batch_dev, leaf order) by route, device events of the library's own profile regions.

  lde_rates_time.py [rounds]
      The shapes both routes can take, (13,4)..(13,7), (12,4)..(12,8), (11,4)..(11,8), (14,4)..(14,6) and FRI-layer sizes 2^7..2^10 at rates 4..8, at
      135 and at 2 columns: QPGPU_NTT_LDE_COSETS=2 (the pruned full-size plan) against =1 (column-resident kernel for d = 11..13, coset
      passes elsewhere), alternated `rounds` times (default 3) in fresh child processes, since the switch is read once per process.
      Then the shapes only the decomposition takes, (13,8) x 135 and (16,5) x 135, on the default route, and the column-resident
      kernel's two workgroup orders (QPGPU_NTT_LDE_COLUMN=2 against =1) at 136 columns. Prints the tables.
  lde_rates_time.py --child
      One pass over all shapes under the environment it was given; prints one JSON line."""
import json, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTH = [(13, r) for r in (4, 5, 6, 7)] + [(12, r) for r in (4, 5, 6, 7, 8)] + [(11, r) for r in (4, 5, 6, 7, 8)] + [(14, r) for r in (4, 5, 6)] + \
       [(d, r) for d in (7, 8, 9, 10) for r in (4, 5, 6, 7, 8)]
ONLY_NEW = [(13, 8), (16, 5)]
XCD = [(13, 5, 136), (13, 8, 136), (11, 8, 136)]    # column counts the XCD-aware workgroup order takes (multiples of 8)
REGIONS = ("ntt_lde_column", "ntt_pass_single", "ntt_pass_strided", "ntt_pass_rows", "ntt_pass_outer")


def child():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    out = {}
    rng = np.random.default_rng(3)
    with pkg.QpGpu(0) as gpu:
        shapes = [(d, r, c) for d, r in BOTH for c in ((135, 2) if d > 10 else (2,))] + [(d, r, 135) for d, r in ONLY_NEW]
        if "--xcd" in sys.argv:
            shapes = XCD
        for d, r, cols in shapes:
            a = rng.integers(0, pkg.P, (cols, 1 << d), dtype=np.uint64)
            d_c = gpu.to_device(a); d_o = gpu.alloc(a.nbytes << r)
            for _ in range(3):
                gpu.lde_dev(d_c, d_o, d, r, cols, bitrev=True)
            gpu.sync()
            gpu.profile(True)                      # starts the regions from zero
            reps = 10
            for _ in range(reps):
                gpu.lde_dev(d_c, d_o, d, r, cols, bitrev=True)
            gpu.sync()
            after = [gpu.profile_read(k)[0] for k in REGIONS]
            gpu.profile(False)
            out["%d,%d,%d" % (d, r, cols)] = round(sum(after) / reps, 5)
            d_c.free(); d_o.free()
    print(json.dumps(out))


def run_child(mode, column=None):
    env = dict(os.environ)
    env.pop("QPGPU_NTT_LDE_COSETS", None)
    if mode is not None:
        env["QPGPU_NTT_LDE_COSETS"] = str(mode)
    if column is not None:
        env["QPGPU_NTT_LDE_COLUMN"] = str(column)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--xcd"] if column is not None else []), env=env, capture_output=True, text=True, timeout=280, check=True)
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    series = {"old": [], "new": []}
    for _ in range(rounds):
        series["old"].append(run_child(2))
        series["new"].append(run_child(1))
    dflt = run_child(None)
    print("ms per LDE, leaf order, device events; old = QPGPU_NTT_LDE_COSETS=2 (pruned full-size plan), new = 1 (decomposition)")
    print("%-14s %-34s %-34s %s" % ("d,r,columns", "old (each round)", "new (each round)", "median new/old"))
    for key in series["old"][0]:
        d, r, _ = (int(x) for x in key.split(","))
        o = [s[key] for s in series["old"]]; n = [s[key] for s in series["new"]]
        if (d, r) in ONLY_NEW:
            print("%-14s %-34s %-34s %s" % (key, "-", " ".join("%.4f" % v for v in o + n), "only route (default: %.4f)" % dflt[key]))
        else:
            print("%-14s %-34s %-34s %.3f" % (key, " ".join("%.4f" % v for v in o), " ".join("%.4f" % v for v in n), float(np.median(n) / np.median(o))))
    xcd = {1: [], 2: []}
    for _ in range(rounds):
        for m in (2, 1):
            xcd[m].append(run_child(None, column=m))
    print("column-resident kernel, workgroup order: plain = QPGPU_NTT_LDE_COLUMN=2, xcd = 1 (the cosets of a column on one XCD)")
    print("%-14s %-34s %-34s %s" % ("d,r,columns", "plain (each round)", "xcd (each round)", "median xcd/plain"))
    for key in xcd[1][0]:
        o = [s[key] for s in xcd[2]]; n = [s[key] for s in xcd[1]]
        print("%-14s %-34s %-34s %.3f" % (key, " ".join("%.4f" % v for v in o), " ".join("%.4f" % v for v in n), float(np.median(n) / np.median(o))))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
