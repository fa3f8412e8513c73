"""The index arithmetic of a coset-sharded oracle (qpgpu_oracle_commit_sharded; csrc/oracle_shard_map.hpp), the part that needs no
device: tests/native/oracle_shard_map_main.cpp compiled with the header alone under AddressSanitizer and
UndefinedBehaviorSanitizer prints, for every (d, r, G) with d in 1..6, r in 1..4, G in {2, 4, 8}, G <= 2^r, the shards' leaf ranges,
cosets and shifts, the leaf -> (shard, local leaf) map and the split of a Merkle path for cap heights 0..min(4, d + r); every line is
checked here against a few lines of Python integers. Plus the new exports' refusal of NULL handles. The commitment itself is tested
on the device by tests/test_oracle_sharded_gpu.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(d, r, G) for d in range(1, 7) for r in range(1, 5) for G in (2, 4, 8) if G <= 1 << r]


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """The program's output, split by case: {(d, r, G): [fields of each line]}, and the lines before the first case."""
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("shard_map") / "oracle_shard_map")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "oracle_shard_map_main.cpp"), "-o", exe])
    r = subprocess.run([exe, "6", "4", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["oracle shard map: ok", ""]
    by_case, head, cur = {}, [], None
    for ln in lines[:-2]:
        f = ln.split()
        if f[0] == "case":
            cur = by_case.setdefault(tuple(int(x) for x in f[1:]), [])
        else:
            (head if cur is None else cur).append(f)
    return by_case, head


def of_kind(recs, kind):
    return [[int(x) for x in f[1:]] for f in recs if f[0] == kind]


def test_every_case_is_there(records):
    by_case, _ = records
    assert sorted(by_case) == sorted(CASES) and len(CASES) == 54


def test_shard_counts_that_are_refused(records):
    _, head = records
    got = {(G, r): v for G, r, v in of_kind(head, "refused")}
    for r in range(1, 5):
        for G in (0, 1, 3, 6, 12, 2 << r):
            assert got[(G, r)] == -1, (G, r)


@pytest.mark.parametrize("d,r,G", CASES)
def test_leaf_ranges_tile_the_leaves(records, d, r, G):
    N = 1 << (d + r)
    ranges = of_kind(records[0][(d, r, G)], "range")
    assert [g for g, _, _ in ranges] == list(range(G))
    at = 0
    for g, first, num in ranges:
        assert first == at and num == N // G
        at += num
    assert at == N


@pytest.mark.parametrize("d,r,G", CASES)
def test_cosets_of_a_shard(records, d, r, G):
    lg = G.bit_length() - 1
    recs = records[0][(d, r, G)]
    cosets = {f[0]: f[1:] for f in of_kind(recs, "cosets")}
    owns = {f[0]: f[1:] for f in of_kind(recs, "owns")}
    shifts = {f[0]: f[1:] for f in of_kind(recs, "shift")}
    seen = []
    for g in range(G):
        want = {k for k in range(1 << r) if brev(k, r) >> (r - lg) == g}
        assert set(cosets[g]) == want and len(cosets[g]) == len(want) == (1 << r) // G
        assert owns[g] == [1 if k in want else 0 for k in range(1 << r)]
        # in the shard's leaf order block j holds the coset whose global block is g 2^(r - lg) + j
        assert [brev(k, r) for k in cosets[g]] == [g * ((1 << r) // G) + j for j in range((1 << r) // G)]
        # ... and they are the cosets e + G k' of the rate 2^r / G LDE on the shift w^e, e = brev(g), block j holding k' = brev(j)
        e, local_r, local_L = shifts[g]
        assert e == brev(g, lg) and local_r == r - lg and local_L == d + r - lg
        assert cosets[g] == [e + G * brev(j, r - lg) for j in range(1 << (r - lg))]
        seen += cosets[g]
    assert sorted(seen) == list(range(1 << r))


@pytest.mark.parametrize("d,r,G", CASES)
def test_leaf_to_shard_round_trips(records, d, r, G):
    N = 1 << (d + r)
    per = N // G
    leaves = of_kind(records[0][(d, r, G)], "leaf")
    assert len(leaves) == N
    for i, (leaf, g, local, back) in enumerate(leaves):
        assert leaf == i and g == i // per and local == i % per and back == i


@pytest.mark.parametrize("d,r,G", CASES)
def test_path_split(records, d, r, G):
    lg = G.bit_length() - 1
    recs = records[0][(d, r, G)]
    paths = {f[0]: f[1:] for f in of_kind(recs, "path")}
    sibs = {(f[0], f[1]): f[2:] for f in of_kind(recs, "siblings")}
    caps = list(range(0, min(4, d + r) + 1))
    assert sorted(paths) == caps
    for cap in caps:
        local_cap, local_len, merge, total, merge_digests = paths[cap][:5]
        offsets = paths[cap][5:]
        assert local_cap == max(0, cap - lg) and merge == max(0, lg - cap)
        assert local_len == (d + r - lg) - local_cap
        assert total == local_len + merge == d + r - cap
        # a shard's roots are 2^local_cap: cap entries as they are, or the leaves of the merge levels
        assert (1 << local_cap) == max(1, (1 << cap) // G)
        assert merge_digests == (sum(G >> t for t in range(merge + 1)) if merge else 0)
        assert offsets == [sum(G >> u for u in range(t)) for t in range(merge)]
        for g in range(G):
            assert sibs[(cap, g)] == [(g >> t) ^ 1 for t in range(merge)]


def test_new_exports_refuse_null_handles(pkg):
    lib = pkg.load_library()
    names = pkg.binding.exported_symbols()
    for n in ("qpgpu_oracle_commit_sharded", "qpgpu_oracle_shards", "qpgpu_oracle_shard_range", "qpgpu_oracle_shard_device_ptrs"):
        assert n in names and hasattr(lib, n), n
    handle = ctypes.c_void_p(0x1234)
    polys = (ctypes.c_uint64 * 8)()
    two = (ctypes.c_void_p * 2)(None, None)
    assert lib.qpgpu_oracle_commit_sharded(None, 2, polys, 1, 3, 1, 0, 0, 0, 0, ctypes.byref(handle)) == -1 and handle.value == 0x1234
    assert lib.qpgpu_oracle_commit_sharded(two, 2, polys, 1, 3, 1, 0, 0, 0, 0, ctypes.byref(handle)) == -1 and handle.value == 0x1234
    assert lib.qpgpu_oracle_commit_sharded(two, 2, polys, 1, 3, 1, 0, 0, 0, 0, None) == -1
    assert lib.qpgpu_oracle_commit_sharded(None, 0, None, 0, 0, 0, 0, 0, 0, 0, None) == -1
    a, b = ctypes.c_uint64(77), ctypes.c_uint64(77)
    assert lib.qpgpu_oracle_shards(None) == 0
    assert lib.qpgpu_oracle_shard_range(None, 0, ctypes.byref(a), ctypes.byref(b)) == -1 and (a.value, b.value) == (77, 77)
    p, q = ctypes.c_void_p(5), ctypes.c_void_p(5)
    assert lib.qpgpu_oracle_shard_device_ptrs(None, 0, ctypes.byref(p), ctypes.byref(q)) == -1 and (p.value, q.value) == (5, 5)
    assert callable(pkg.QpGpu.commit_sharded) and callable(pkg.binding.PolyOracle.commit_sharded)
