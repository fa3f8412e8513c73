"""Commit of 135 columns at 2^16 and 2^19 rows (rate_bits 3, cap_height 4) on one context against the same commitment sharded by
cosets over several (qpgpu_oracle_commit_sharded).

  oracle_sharded_time.py [--degree-bits 16 19] [--cols 135] [--reps 6] [--out profiles/oracle_sharded.txt]

The shards run on one context per visible device, or on two contexts of device 0 when there is one device: then they share that
device, no speed-up is expected, and the output says in its first lines that the multi-device time is unmeasured. The values lie
on the home device before the clock starts (QPGPU_ORACLE_DEVICE_INPUT). Each context works on a torch stream of its own, so that
HIP events can be recorded around the call on every stream: the device time of a commit is the longest of its streams' start-to-end
intervals, the wall time a host clock around the call (which has synchronised every stream when it returns). Two warm-up calls of
each, then the two alternated call by call, medians and ranges of --reps calls. The caps are compared every time. Writes --out afresh:
the device count on the first line, then one JSON line per size. Not a pass/fail figure. No GPU: it fails, it does not fall back."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

P = 0xFFFFFFFF00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree-bits", type=int, nargs="+", default=[16, 19])
    ap.add_argument("--cols", type=int, default=135)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("oracle_sharded_time: no GPU visible")
    pkg = ge.load_package()
    ndev = torch.cuda.device_count()
    shard_devs = list(range(1 << (min(ndev, 8).bit_length() - 1))) if ndev > 1 else [0, 0]
    head = ["devices visible: %d; shards on devices %s" % (ndev, shard_devs)]
    if ndev == 1:
        head.append("one device: the shards are contexts of the same device and share it; the multi-device time is UNMEASURED")
    streams = [torch.cuda.Stream(device=dv) for dv in [0] + shard_devs]
    ctxs = [pkg.QpGpu(dv, stream=s.cuda_stream) for dv, s in zip([0] + shard_devs, streams)]
    one, group, group_streams = ctxs[0], ctxs[1:], streams[1:]
    kw = dict(rate_bits=3, cap_height=4)
    lines = []

    def timed(make, on):
        """(device ms, wall ms, cap) of one commit; `on`: the streams it works on."""
        ev = []
        for s in on:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.device(s.device):
                e0.record(s)
            ev.append((s, e0, e1))
        t0 = time.perf_counter()
        o = make()
        wall = 1e3 * (time.perf_counter() - t0)
        for s, e0, e1 in ev:
            with torch.cuda.device(s.device):
                e1.record(s)
        for s, e0, e1 in ev:
            e1.synchronize()
        dev = max(e0.elapsed_time(e1) for s, e0, e1 in ev)
        cap = o.cap()
        o.close()
        return dev, wall, cap

    for d in a.degree_bits:
        rng = np.random.default_rng(d)
        vals = rng.integers(0, P, size=(a.cols, 1 << d), dtype=np.uint64)
        # the home contexts of the two commitments are different contexts of device 0: one upload serves both
        buf = one.to_device(vals)
        src = (buf, a.cols, 1 << d)
        plain = lambda: pkg.PolyOracle(one, src, **kw)
        sharded = lambda: group[0].commit_sharded(group, src, **kw)
        for _ in range(2):
            want = timed(plain, streams[:1])[2]
            assert np.array_equal(timed(sharded, group_streams)[2], want), "the sharded cap differs"
        ta, tb = [], []
        for _ in range(a.reps):
            x = timed(plain, streams[:1]); ta.append(x[:2])
            y = timed(sharded, group_streams); tb.append(y[:2])
            assert np.array_equal(x[2], want) and np.array_equal(y[2], want)
        buf.free()
        stat = lambda v, k: {"median": round(float(np.median([t[k] for t in v])), 3), "min": round(min(t[k] for t in v), 3), "max": round(max(t[k] for t in v), 3)}
        lines.append(json.dumps({"degree_bits": d, "cols": a.cols, "rate_bits": 3, "cap_height": 4, "reps": a.reps, "shards": len(group),
                                 "devices": ndev, "unsharded_device_ms": stat(ta, 0), "unsharded_wall_ms": stat(ta, 1),
                                 "sharded_device_ms": stat(tb, 0), "sharded_wall_ms": stat(tb, 1)}))
        print(lines[-1], flush=True)
    for c in ctxs:
        c.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(head) + "\n$ python tools/oracle_sharded_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")
    print("\n".join(head))


if __name__ == "__main__":
    main()
