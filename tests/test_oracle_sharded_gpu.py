"""qpgpu_oracle_commit_sharded: one polynomial commitment whose leaves are split by cosets over several contexts (here all of
them on device 0), held to qpgpu_oracle_commit on one context, which is unchanged code that the rest of the suite pins to the CPU
restatement: the cap, the coefficients, the whole LDE, the leaf width, evaluations, and every opened leaf, salt and path must be
equal word for word; qpgpu_fri_prove and the stepwise session over a mix of sharded and plain oracles must give the bytes of the
all-plain call. One cap is pinned to the CPU restatement directly. Exact arithmetic: every comparison is equality. The largest
shape has 2^17 leaves of 9 columns."""
import ctypes

import numpy as np
import pytest

import fri_schedules as fs

pytestmark = pytest.mark.gpu
P = fs.P
EINVAL, EVERIFY = -1, -6
MULT_GEN = 14293326489335486720

# (degree_bits, rate_bits, columns, cap_height, shards): the smallest shapes that reach each transform regime of a shard's own LDE
# (rate 2^r / G) and each routing branch
SHAPES = [
    (5, 3, 3, 4, 2),      # rows of at most 4 elements, no permutation
    (5, 3, 9, 4, 8),      # one coset per shard: the shard's LDE is a plain coset transform
    (5, 3, 9, 0, 4),      # two home merge levels
    (6, 4, 20, 2, 8),     # one home merge level
    (12, 3, 20, 4, 4),    # the column-resident LDE kernel
    (14, 3, 9, 4, 2),     # two-pass transforms, 2^16 leaves per shard
    (5, 1, 9, 1, 2),      # rate 2, the cap is the shards' roots
]
VARIANTS = {"values": SHAPES, "coeffs_blinded": [SHAPES[2], SHAPES[4]], "poseidon2": [SHAPES[0], SHAPES[2]]}
CASES = [(v, s) for v, shapes in VARIANTS.items() for s in shapes]


@pytest.fixture(scope="module")
def ctxs(pkg, gpu):
    """Eight contexts on device 0, the session's first: the home context of every sharded oracle here."""
    more = [pkg.QpGpu(0) for _ in range(7)]
    yield [gpu] + more
    for c in more:
        c.close()


@pytest.fixture(scope="module")
def ctxs_p2(pkg):
    prm = pkg.poseidon2_qp_params()
    cs = [pkg.QpGpu(0, hasher=prm) for _ in range(4)]
    yield cs
    for c in cs:
        c.close()


def pair(pkg, cs, polys, rate, cap, G, **kw):
    """The same polynomials committed on one context and over G of them."""
    plain = pkg.PolyOracle(cs[0], polys, rate_bits=rate, cap_height=cap, **kw)
    try:
        return plain, cs[0].commit_sharded(cs[:G], polys, rate_bits=rate, cap_height=cap, **kw)
    except Exception:
        plain.close()
        raise


@pytest.mark.parametrize("variant,shape", CASES, ids=["%s-d%d_r%d_c%d_h%d_G%d" % ((v,) + s) for v, s in CASES])
def test_sharded_equals_unsharded(pkg, ctxs, ctxs_p2, variant, shape):
    d, r, cols, cap_h, G = shape
    N = 1 << (d + r)
    rng = np.random.default_rng(1000 * d + 100 * r + 10 * cap_h + G)
    polys = rng.integers(0, P, size=(cols, 1 << d), dtype=np.uint64)
    kw = dict(coeffs=True, blinding=True, blinding_seed=77, blinding_stream=2) if variant == "coeffs_blinded" else {}
    plain, sh = pair(pkg, ctxs_p2 if variant == "poseidon2" else ctxs, polys, r, cap_h, G, **kw)
    try:
        assert plain.shards == 1 and plain.shard_range(0) == (0, N)
        assert sh.shards == G and [sh.shard_range(g) for g in range(G)] == [(g * (N // G), N // G) for g in range(G)]
        assert np.array_equal(sh.cap(), plain.cap())
        assert np.array_equal(sh.read(lde=False), plain.read(lde=False))
        if variant == "coeffs_blinded":
            assert np.array_equal(sh.read(lde=False), polys)
        assert np.array_equal(sh.read(lde=True), plain.read(lde=True))
        assert np.array_equal(sh.read(lde=True, first=1, count=cols - 1), plain.read(lde=True, first=1, count=cols - 1))
        assert sh.leaf_width == plain.leaf_width == cols + (4 if kw else 0)
        for pt in ((3, 5), tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64))):
            assert np.array_equal(sh.eval(pt), plain.eval(pt))
        if d <= 6:
            idx = np.arange(N, dtype=np.uint64)
        else:       # 64 indices, the first and last leaf of every shard among them, in no order
            edge = [g * (N // G) + e for g in range(G) for e in (0, N // G - 1)]
            idx = np.concatenate([np.array(edge, dtype=np.uint64), rng.integers(0, N, size=64 - len(edge), dtype=np.uint64)])
            rng.shuffle(idx)
        rows_s, paths_s = sh.open(idx)
        rows_p, paths_p = plain.open(idx)
        assert rows_s.shape == (idx.size, cols + (4 if kw else 0)) and paths_s.shape == (idx.size, d + r - cap_h, 4)
        assert np.array_equal(rows_s, rows_p)          # the salt words of a blinded oracle are the last four of each row
        assert np.array_equal(paths_s, paths_p)
        # either output alone, in the caller's order
        back = idx[::-1][:33]
        assert np.array_equal(sh.open(back, paths=False)[0], rows_p[::-1][:33])
        assert np.array_equal(sh.open(back, rows=False)[1], paths_p[::-1][:33])
    finally:
        sh.close()
        plain.close()


def test_cap_against_the_cpu_restatement(pkg, ctxs, orc):
    """(5, 3, 9, 4, 8): the cap of the sharded commitment from the restatement's LDE and Merkle tree."""
    d, r, cols, cap_h, G = SHAPES[1]
    L = d + r
    vals = np.random.default_rng(58).integers(0, P, size=(cols, 1 << d), dtype=np.uint64)
    _, lde = orc.lde_batch(vals, d, r, MULT_GEN)
    rev = np.array([int(format(i, "0%db" % L)[::-1], 2) for i in range(1 << L)])
    _, cap_want = orc.merkle(np.ascontiguousarray(lde.T[rev]), cap_h)
    sh = ctxs[0].commit_sharded(ctxs[:G], vals, rate_bits=r, cap_height=cap_h)
    try:
        assert np.array_equal(sh.cap(), cap_want)
        assert np.array_equal(sh.read(lde=True), lde[:, rev])
    finally:
        sh.close()


FRI_ROWS = {6: dict(rate=3, cap=1, arity=[2, 1]), 12: dict(rate=3, cap=4, arity=[4, 3])}
NQ, POW = 4, 4


def fri_oracles(pkg, ctxs, d, sharded):
    """Two oracles: five plain columns (sharded over four contexts or not), three blinded ones on the home context."""
    row = FRI_ROWS[d]
    rng = np.random.default_rng(600 + d)
    a = rng.integers(0, P, size=(5, 1 << d), dtype=np.uint64)
    b = rng.integers(0, P, size=(3, 1 << d), dtype=np.uint64)
    kw = dict(rate_bits=row["rate"], cap_height=row["cap"])
    o0 = ctxs[0].commit_sharded(ctxs[:4], a, **kw) if sharded else pkg.PolyOracle(ctxs[0], a, **kw)
    o1 = pkg.PolyOracle(ctxs[0], b, blinding=True, blinding_seed=9, blinding_stream=1, **kw)
    return [o0, o1]


FRI_BATCHES = [[(0, 0, 5), (1, 0, 3)], [(0, 1, 2)]]
FRI_POINTS = [(11, 13), (0x1234567890, 17)]


@pytest.mark.parametrize("d", sorted(FRI_ROWS))
def test_fri_over_a_sharded_and_a_plain_oracle(pkg, ctxs, d):
    row = FRI_ROWS[d]
    kw = dict(rate_bits=row["rate"], cap_height=row["cap"])
    N = 1 << (d + row["rate"])
    got = {}
    for sharded in (False, True):
        oracles = fri_oracles(pkg, ctxs, d, sharded)
        try:
            batches = list(zip(FRI_POINTS, FRI_BATCHES))
            ch = pkg.Challenger(ctxs[0])
            ch.observe(np.arange(5, 16, dtype=np.uint64))
            before = fs.copy_challenger(pkg, ch)
            proof = pkg.fri_prove(ctxs[0], oracles, batches, ch, row["arity"], proof_of_work_bits=POW, num_query_rounds=NQ, **kw)
            caps = [o.cap() for o in oracles]
            openings = np.concatenate([oracles[o].eval(pt, f, c) for pt, rg in batches for o, f, c in rg])
            # the same one step at a time, with an alpha, betas and indices no challenger produced: the first and last leaf of the LDE
            # and of a shard, and a repeated one
            indices = [0, N - 1, N // 4, N // 2 - 1, 3 * N // 4 + 5, 3 * N // 4 + 5]
            with pkg.FriSession(ctxs[0], oracles, batches, (21, 23), row["arity"], **kw) as s:
                step_caps = []
                for beta in [(3, 5), (P - 1, 1)]:
                    step_caps.append(s.round_commit())
                    s.round_fold(beta)
                queries = s.open(indices)
                final = s.final_poly()
            got[sharded] = (proof, caps, openings, before, [c.tobytes() for c in step_caps], queries, final.tobytes())
        finally:
            for o in oracles:
                o.close()
    assert got[True][0] == got[False][0], "qpgpu_fri_prove bytes"
    assert all(np.array_equal(a, b) for a, b in zip(got[True][1], got[False][1]))
    assert got[True][4:] == got[False][4:], "the stepwise session's caps, query bytes and final polynomial"
    proof, caps, openings, before = got[True][:4]
    shapes = [(5, False), (3, True)]
    with pkg.FriVerifier(d, shapes, FRI_BATCHES, row["arity"], proof_of_work_bits=POW, num_query_rounds=NQ, **kw) as fv:
        assert fv.proof_size() == len(proof)
        alpha, betas, powr, idx = fv.challenges(fs.copy_challenger(pkg, before), proof)
        assert fv.verify(caps, FRI_POINTS, openings, alpha, betas, powr, idx, proof), fv.reason


def test_a_flipped_word_in_a_shard_is_rejected(pkg, ctxs):
    """One word of shard 2's LDE overwritten on its device: a proof that opens that leaf no longer verifies; one that does not, does."""
    d, rate, cap, arity, G = 6, 3, 1, [2, 1], 4
    N = 1 << (d + rate)
    kw = dict(rate_bits=rate, cap_height=cap)
    polys = np.random.default_rng(71).integers(0, P, size=(3, 1 << d), dtype=np.uint64)
    sh = ctxs[0].commit_sharded(ctxs[:G], polys, **kw)
    try:
        first, num = sh.shard_range(2)
        leaf = first + 37
        lde_ptr, dig_ptr = sh.shard_device_ptrs(2)
        assert lde_ptr and dig_ptr
        word = np.array([(int(sh.read(lde=True)[1, leaf]) + 1) % P], dtype=np.uint64)
        ctxs[2]._check(ctxs[2].lib.qpgpu_memcpy_h2d(ctxs[2].ctx, ctypes.c_void_p(lde_ptr + 8 * (1 * num + 37)), word.ctypes.data, 8))
        assert int(sh.read(lde=True)[1, leaf]) == int(word[0])
        point, alpha, betas = (11, 13), (21, 23), [(3, 5), (P - 1, 1)]
        verdicts = {}
        with pkg.FriVerifier(d, [(3, False)], [[(0, 0, 3)]], arity, proof_of_work_bits=0, num_query_rounds=NQ, **kw) as fv:
            for name, indices in (("opens_it", [0, leaf, N - 1, 5]), ("elsewhere", [0, leaf - 1, N - 1, 5])):
                with pkg.FriSession(ctxs[0], [sh], [(point, [(0, 0, 3)])], alpha, arity, **kw) as s:
                    caps = []
                    for b in betas:
                        caps.append(s.round_commit())
                        s.round_fold(b)
                    queries = s.open(indices)
                    final = s.final_poly()
                fri = b"".join(c.tobytes() for c in caps) + queries + final.tobytes() + bytes(8)
                ok = fv.verify([sh.cap()], [point], sh.eval(point), alpha, betas, 0, indices, fri)
                verdicts[name] = (ok, fv.code)
        assert verdicts["elsewhere"] == (True, 0)
        assert verdicts["opens_it"] == (False, EVERIFY)
    finally:
        sh.close()


def raw_commit(pkg, cs, polys, d, rate, cap):
    """qpgpu_oracle_commit_sharded as the C caller sees it: (code, handle left behind, message on ctxs[0])."""
    lib = cs[0].lib
    arr = (ctypes.c_void_p * len(cs))(*[c.ctx for c in cs])
    h = ctypes.c_void_p(0x1234)
    rc = lib.qpgpu_oracle_commit_sharded(arr, len(cs), polys.ctypes.data, polys.shape[0], d, rate, cap, 0, 0, 0, ctypes.byref(h))
    return rc, h.value, cs[0].last_error()


def test_refusals(pkg, ctxs, ctxs_p2):
    d, rate, cap = 5, 2, 1
    N = 1 << (d + rate)
    polys = np.random.default_rng(5).integers(0, P, size=(3, 1 << d), dtype=np.uint64)
    c = ctxs
    for cs, words in (([c[0]], ("one context", "qpgpu_oracle_commit")),
                      ([c[0], c[1], c[2]], ("n_ctx = 3", "power of two")),
                      (c[:8], ("n_ctx = 8", "2^rate_bits = 4")),
                      ([c[0], c[1], c[2], c[1]], ("ctxs[1] and ctxs[3]", "same context")),
                      ([c[0], ctxs_p2[0]], ("ctxs[1]", "another hasher"))):
        rc, h, msg = raw_commit(pkg, cs, polys, d, rate, cap)
        assert rc == EINVAL and h is None and all(w in msg for w in words), (len(cs), msg)
    with pytest.raises(pkg.QpGpuError, match="qpgpu_oracle_commit"):
        c[0].commit_sharded([c[0]], polys, rate_bits=rate, cap_height=cap)

    sh = c[0].commit_sharded(c[:4], polys, rate_bits=rate, cap_height=cap)
    lib = c[0].lib
    try:
        p = [ctypes.c_void_p(5) for _ in range(3)]
        assert lib.qpgpu_oracle_device_ptrs(sh.h, *[ctypes.byref(x) for x in p]) == EINVAL and [x.value for x in p] == [5, 5, 5]
        assert "qpgpu_oracle_shard_device_ptrs" in c[0].last_error() and "4 contexts" in c[0].last_error()
        assert lib.qpgpu_oracle_shard_range(sh.h, 4, None, None) == EINVAL and lib.qpgpu_oracle_shard_device_ptrs(sh.h, 4, None, None) == EINVAL
        # the stage plan: the oracle is looked at once the header has passed
        pack = pkg.synth_circuit(8, seed=64, poseidon=True)[0]
        with pytest.raises(pkg.QpGpuError, match="cs_oracle is sharded over 4 contexts: sharded oracles are not taken here yet") as e:
            pkg.StagePlan(c[0], pack, sh)
        assert e.value.code == EINVAL
        # the lockstep entries
        idx = np.array([1, 2], dtype=np.uint64)
        rows = np.full((2, 3), 7, dtype=np.uint64); paths = np.full((2, d + rate - cap, 4), 7, dtype=np.uint64)
        assert lib.qpgpu_oracle_open_batch(sh.h, idx.ctypes.data, 2, rows.ctypes.data, paths.ctypes.data) == EINVAL
        assert "oracle_open_batch: sharded oracles are not taken here yet" in c[0].last_error() and (rows == 7).all() and (paths == 7).all()
        pt = np.array([3, 5], dtype=np.uint64); ev = np.full((3, 2), 7, dtype=np.uint64)
        assert lib.qpgpu_oracle_eval_batch(sh.h, pt.ctypes.data, 0, 3, ev.ctypes.data) == EINVAL and (ev == 7).all()
        assert "oracle_eval_batch: sharded oracles are not taken here yet" in c[0].last_error()
        batches = [((3, 5), [(0, 0, 3)])]
        with pytest.raises(pkg.QpGpuError, match="fri_prove_batch: oracle 0 is sharded; sharded oracles are not taken here yet"):
            pkg.fri_prove_batch(c[0], [sh], [(np.array([[3, 5]], dtype=np.uint64), [(0, 0, 3)])], [pkg.Challenger(c[0])], [2],
                                rate_bits=rate, cap_height=cap, proof_of_work_bits=0, num_query_rounds=2)
        with pytest.raises(pkg.QpGpuError, match="sharded oracles are not taken here yet"):
            pkg.FriSession(c[0], [sh], [(np.array([[3, 5]], dtype=np.uint64), [(0, 0, 3)])], np.array([[7, 11]], dtype=np.uint64), [2],
                           rate_bits=rate, cap_height=cap, batch=1)
        # an index past the last leaf: refused as qpgpu_oracle_open refuses it, outputs untouched
        bad = np.array([0, N], dtype=np.uint64)
        assert lib.qpgpu_oracle_open(sh.h, bad.ctypes.data, 2, rows.ctypes.data, paths.ctypes.data) == EINVAL
        assert "indices[1] = %d is not below 2^%d" % (N, d + rate) in c[0].last_error() and (rows == 7).all() and (paths == 7).all()
        # a FRI call on a context that is not the oracle's home
        ch = pkg.Challenger(c[1])
        state = bytes(ch.state)
        with pytest.raises(pkg.QpGpuError, match="ctx is not the home context .* of sharded oracle 0"):
            pkg.fri_prove(c[1], [sh], batches, ch, [2], rate_bits=rate, cap_height=cap, proof_of_work_bits=0, num_query_rounds=2)
        assert bytes(ch.state) == state
        with pytest.raises(pkg.QpGpuError, match="ctx is not the home context"):
            pkg.FriSession(c[1], [sh], batches, (7, 11), [2], rate_bits=rate, cap_height=cap)
        # and the oracle still answers
        assert sh.open([N - 1])[0].shape == (1, 3)
    finally:
        sh.close()


def test_free_scrubs_every_shard(pkg, ctxs):
    """The polynomial words lie on the home context and, as each shard's copy, on every other; qpgpu_ctx_residue_scan lists them under
    the context that owns the buffer, and after qpgpu_oracle_free finds them on none."""
    G = 4
    polys = np.random.default_rng(23).integers(1 << 32, P, size=(4, 64), dtype=np.uint64)     # the scan takes needles above 2^32
    needles = np.array(list(dict.fromkeys(int(v) for v in polys.ravel()))[:6], dtype=np.uint64)
    sh = ctxs[0].commit_sharded(ctxs[:G], polys, rate_bits=3, cap_height=1, coeffs=True)
    try:
        for g in range(G):
            hits, first, _ = ctxs[g].residue_scan(needles)
            assert hits >= needles.size and {h["region"] for h in first} == {"oracle"}, g
    finally:
        sh.close()
    for g in range(G):
        assert ctxs[g].residue_scan(needles)[0] == 0, g
