"""The index arithmetic of stage s6 over coset-sharded oracles (qpgpu_stage_plan_create_sharded; csrc/quotient_shard_map.hpp), the
part that needs no device: tests/native/quotient_shard_map_main.cpp compiled with the header alone under AddressSanitizer and
UndefinedBehaviorSanitizer prints, for every d in 1..4, r in 1..5, qbits in 0..min(r, 3) and every shard count G = 1 .. 2^r (G = 1: the
stage on one context, whose plan takes its geometry from the same arithmetic), which shards hold quotient points, each working shard's launch (local LDE size, rate, q_shift, number of points M, exponent e), the
quotient index of each of its points and the merge's read blocks and write positions; every line is checked here against a few
lines of Python integers. The merge formula itself (the shards' size-M inverse transforms, the (g_mult w^e)^-j scaling on the shard
and the Gq-point inverse transform with g_mult^(-cM) / Gq on the home context) is run in Python integers against directly chosen
coefficients. Plus: the new exports refuse NULL, and the C example compiles against the headers. The stage itself is tested on the
device by tests/test_stage_sharded_gpu.py."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
MULT_GEN = 14293326489335486720
ROOT_2_32 = 7277203076849721926
CASES = [(d, r, q, 1 << lg) for d in range(1, 5) for r in range(1, 6) for q in range(0, min(r, 3) + 1) for lg in range(0, r + 1)]


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def root(bits):
    return pow(ROOT_2_32, 1 << (32 - bits), P)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("quotient_shard_map") / "quotient_shard_map")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "quotient_shard_map_main.cpp"), "-o", exe])
    r = subprocess.run([exe, "4", "5", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["quotient shard map: ok", ""]
    by_case, cur = {}, None
    for ln in lines[:-2]:
        f = ln.split()
        if f[0] == "case":
            cur = by_case.setdefault(tuple(int(x) for x in f[1:]), [])
        else:
            cur.append(f)
    return by_case


def of_kind(recs, kind):
    return [[int(x) for x in f[1:]] for f in recs if f[0] == kind]


def test_every_case_is_there(records):
    assert sorted(records) == sorted(CASES)


@pytest.mark.parametrize("d,r,q,G", CASES)
def test_working_shards_and_their_launches(records, d, r, q, G):
    recs = records[(d, r, q, G)]
    lg = G.bit_length() - 1
    q_shift, N, Nq = r - q, 1 << (d + r), 1 << (d + q)
    # which global natural indices are quotient points, and which shard holds natural index i: the one with brev_lg(g) = i mod G
    holders = {}
    for i in range(0, N, 1 << q_shift):
        holders.setdefault(brev(i % G, lg), []).append(i)
    Gq = max(1, G >> q_shift)
    assert sorted(holders) == list(range(Gq)), "the shards that hold quotient points are the first Gq"
    M = Nq // Gq
    (dom,) = of_kind(recs, "domain")
    assert dom == [q_shift, Nq, Gq.bit_length() - 1, Gq, M]
    shards = of_kind(recs, "shard")
    points = {f[0]: f[1:] for f in of_kind(recs, "points")}
    assert [s[0] for s in shards] == list(range(G))
    for s in shards:
        g = s[0]
        if g >= Gq:
            assert s[1:] == [0] and g not in points
            continue
        local_q_shift = max(0, q_shift - lg)
        e = brev(g, Gq.bit_length() - 1)
        assert s[1:] == [1, d + r - lg, r - lg, local_q_shift, (d + q) - (Gq.bit_length() - 1), e, brev(g, lg)]
        # the launch walks the local natural indices 0 mod 2^local_q_shift; local i' is global brev_lg(g) + G i'
        local = [i for i in range(N // G) if i % (1 << local_q_shift) == 0]
        assert len(local) == M == len(holders[g])
        glob = [brev(g, lg) + G * i for i in local]
        assert glob == holders[g]
        assert points[g] == [x >> q_shift for x in glob] == [e + Gq * k for k in range(M)]
        # the shard's shift is the quotient coset's shift times w_(d+q)^e
        assert pow(root(d + r), brev(g, lg), P) == pow(root(d + q), e, P)


@pytest.mark.parametrize("d,r,q", sorted({c[:3] for c in CASES}))
def test_one_shard_is_the_unsharded_stage(records, d, r, q):
    """lg = 0 is where a plan on one context takes its s6 geometry from: one working shard whose launch is the circuit's own LDE
    (2^(d + r) leaves at rate 2^r on the shift g_mult itself, the quotient on every 2^(r - qbits)-th point), its points the
    quotient domain in order, and a merge that moves nothing."""
    recs = records[(d, r, q, 1)]
    Nq = 1 << (d + q)
    assert of_kind(recs, "domain") == [[r - q, Nq, 0, 1, Nq]], "one working shard, M = Nq"
    assert of_kind(recs, "shard") == [[0, 1, d + r, r, r - q, d + q, 0, 0]], "the circuit's LDE, exponent and shift exponent 0"
    assert of_kind(recs, "points") == [[0] + list(range(Nq))], "local point i is quotient index i"
    assert of_kind(recs, "out") == [[0] + list(range(Nq))], "the single merge line is the identity"
    assert of_kind(recs, "blocks") == [[0]]


@pytest.mark.parametrize("d,r,q,G", CASES)
def test_merge_positions(records, d, r, q, G):
    recs = records[(d, r, q, G)]
    Gq = max(1, G >> (r - q))
    M = (1 << (d + q)) // Gq
    outs = of_kind(recs, "out")
    assert [o[0] for o in outs] == list(range(Gq))
    assert sorted(x for o in outs for x in o[1:]) == list(range(Gq * M)), "every coefficient is written once"
    for o in outs:
        assert o[1:] == [o[0] * M + j for j in range(M)]
    (blocks,) = of_kind(recs, "blocks")
    assert blocks == [brev(e, Gq.bit_length() - 1) for e in range(Gq)]


def idft(vals, w):
    """Inverse transform of len(vals) values at the powers of w, in Python integers."""
    m = len(vals)
    minv, winv = pow(m, P - 2, P), pow(w, P - 2, P)
    return [minv * sum(v * pow(winv, i * j, P) for i, v in enumerate(vals)) % P for j in range(m)]


@pytest.mark.parametrize("d,q,r,lg", [(2, 2, 2, 1), (2, 2, 2, 2), (3, 3, 3, 3), (2, 2, 4, 1), (2, 2, 4, 2), (2, 2, 4, 3), (2, 2, 4, 4), (3, 1, 3, 2)])
def test_merge_formula_in_integers(d, q, r, lg):
    """q_(j + cM) = g^-(j + cM) Gq^-1 sum_e w_Gq^(-e c) w^(-e j) A_(g(e))[j], with A the plain size-M inverse transform of the shard's
    values in natural order, split as the library splits it: (g w^e)^-j on the shard, the rest on the home context."""
    rng = random.Random(1000 * d + 100 * q + 10 * r + lg)
    G, q_shift, Nq = 1 << lg, r - q, 1 << (d + q)
    Gq = max(1, G >> q_shift)
    lq, M = Gq.bit_length() - 1, Nq // Gq
    coeffs = [rng.randrange(P) for _ in range(Nq)]
    w, wL = root(d + q), root(d + r)
    ev = lambda x: sum(c * pow(x, k, P) for k, c in enumerate(coeffs)) % P
    blocks = []
    for g in range(Gq):
        e = brev(g, lq)
        # the shard's quotient points, through the LDE's own indexing: local natural i', global brev_lg(g) + G i', every 2^q_shift-th
        local_q_shift = max(0, q_shift - lg)
        pts = [MULT_GEN * pow(wL, brev(g, lg) + G * i, P) % P for i in range(0, (1 << (d + r)) // G, 1 << local_q_shift)]
        assert pts == [MULT_GEN * pow(w, e + Gq * k, P) % P for k in range(M)]
        a = idft([ev(x) for x in pts], pow(w, Gq, P))
        sinv = pow(MULT_GEN * pow(w, e, P) % P, P - 2, P)
        blocks.append([a[j] * pow(sinv, j, P) % P for j in range(M)])
    wq_inv, ginv, gq_inv = pow(pow(w, M, P), P - 2, P), pow(MULT_GEN, P - 2, P), pow(Gq, P - 2, P)
    got = [0] * Nq
    for c in range(Gq):
        scale = pow(ginv, c * M, P) * gq_inv % P
        for j in range(M):
            got[c * M + j] = scale * sum(pow(wq_inv, e * c, P) * blocks[brev(e, lq)][j] for e in range(Gq)) % P
    assert got == coeffs


def test_new_exports_refuse_null(pkg):
    lib = pkg.load_library()
    names = pkg.binding.exported_symbols()
    for n in ("qpgpu_stage_plan_create_sharded", "qpgpu_stage_plan_shards"):
        assert n in names and hasattr(lib, n), n
    assert lib.qpgpu_stage_plan_shards(None) == 0
    h = ctypes.c_void_p(0x1234)
    err = ctypes.create_string_buffer(pkg.binding.STAGE_ERR_CAP)
    words = (ctypes.c_uint64 * 4)()
    assert lib.qpgpu_stage_plan_create_sharded(None, None, 0, None, None, None) == -1
    assert lib.qpgpu_stage_plan_create_sharded(None, None, 0, None, ctypes.byref(h), err) == -1 and h.value is None
    assert b"stage_plan_create_sharded: null words" in err.value
    # the header is looked at before the context and the oracle: four zero words are no pack
    assert lib.qpgpu_stage_plan_create_sharded(None, words, 4, None, ctypes.byref(h), err) == -1 and h.value is None
    assert err.value.startswith(b"stage_plan_create_sharded: ") and b"null context" not in err.value
    assert callable(pkg.binding.StagePlan.create_sharded)


def test_sharded_stage_example_compiles_against_the_headers(tmp_path):
    """examples/sharded_stage_prove_example.c uses only include/; it must compile and link with plain gcc."""
    out = str(tmp_path / "qpgpu_sharded_stage_prove_example")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sharded_stage_prove_example.c"),
                           "-L", os.path.join(ROOT, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "qp-zk-circuits_amd"), "-o", out])
    assert os.path.exists(out)
