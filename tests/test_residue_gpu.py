"""The secret residue audit on the device (include/qpgpu.h "secret residue audit"; csrc/residue.hpp, residue_kernels.hip): the
counterpart of the reference's wormhole/circuit/tests/heap_zeroization.rs (a custom allocator scans every freed block for the
secret) and of the zeroizing wrappers of wormhole/circuit/src/sensitive.rs. The library lists every device and pinned buffer it
allocates for a context; qpgpu_ctx_residue_scan looks for witness-derived 64-bit words in them, the release audit scans each
buffer once more right before it is freed.

Needles (never public): the four limbs of the spend secret, the four elements of the inner digest H("wormhole" || secret) (the
account itself is H(H(..)) and public), three capacity-lane outputs of Poseidon2 gate rows read from a generated witness; for the
blinded entry the four 64-bit words of a seeded ChaCha key and a drawn blinding value.

Every test that expects "0 hits" has a positive control next to it (the same scan finds the same needles where the contract says
they are resident), so a scan that sees nothing cannot pass. Shapes: the leaf circuit at its own 2^8 rows on test_inputs_0, a pool
of 2 workers x max_batch 2, a 4-column oracle at 2^8 rows and rate 3. Each test gets a context of its own: nothing an earlier test
left resident can be found by a later one."""
import ctypes

import numpy as np
import pytest

import leaf_cases as lc
import oracle_binding as ob
import test_stage_plan_gpu as sp

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
NW = 135


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


@pytest.fixture(scope="module")
def full(L):
    return L.LeafCircuit()


@pytest.fixture()
def ctx(pkg):
    g = pkg.QpGpu(0)
    yield g
    g.close()


def inner_digest(pkg, secret):
    """H(felts("wormhole") || secret) with qpgpu_poseidon2_hash_pad10 on the host: the preimage of the unspendable account."""
    lib = pkg.leaf._lib()
    pre = (ctypes.c_uint64 * 7)()
    lib.qpgpu_bytes_to_felts.restype = ctypes.c_size_t
    lib.qpgpu_bytes_to_felts.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    lib.qpgpu_bytes_to_digest.restype = None
    lib.qpgpu_bytes_to_digest.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    lib.qpgpu_poseidon2_hash_pad10.restype = ctypes.c_int
    lib.qpgpu_poseidon2_hash_pad10.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert lib.qpgpu_bytes_to_felts(b"wormhole", 8, pre, 3) == 3
    lib.qpgpu_bytes_to_digest(bytes(secret), ctypes.byref(pre, 24))
    out = (ctypes.c_uint64 * 4)()
    assert lib.qpgpu_poseidon2_hash_pad10(None, 0, pre, 7, out) == 0
    # and it IS the preimage of the public account: H(inner) == unspendable_account(secret)
    acc = ctypes.create_string_buffer(32)
    lib.qpgpu_poseidon2_hash_bytes.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    assert lib.qpgpu_poseidon2_hash_bytes(None, 0, out, 4, acc) == 0 and acc.raw == pkg.leaf.unspendable_account(secret)
    return [int(v) for v in pre[3:7]], [int(v) for v in out]


@pytest.fixture(scope="module")
def case(pkg, L, full):
    """test_inputs_0 committed, its witness generated once on a throwaway context and read back with qpgpu_memcpy_d2h, the needles."""
    x = lc.test_inputs(L, 0)
    cells, values, pis = full.commit(x)
    n = 1 << full.info["degree_bits"]
    assert n == 256
    g = pkg.QpGpu(0)
    circ = pkg.Circuit(g, full.pack)
    d = g.alloc(NW * n * 8)
    circ.generate_witness_partial_dev(cells, values, pis, d)
    wires = d.download().reshape(NW, n).copy()
    rows = circ.gate_rows(14)
    d.free(scrub=True); circ.close(); g.close()
    secret_limbs, inner = inner_digest(pkg, x.get32("secret"))
    lay = pkg.pack_p2_layout(full.pack)
    w_out = lay["w_output"] if lay else 12
    assert rows.size >= 3
    gate_out = [int(wires[w_out + 8 + k, int(rows[k])]) for k in range(3)]          # capacity lanes: never part of a digest
    needles = secret_limbs + inner + gate_out
    assert all(v >= 1 << 32 for v in needles) and len(set(needles)) == len(needles)
    public = set(int(v) for v in pis)
    assert not public & set(needles)
    # the needles are in the witness (this is what makes them needles), the inner digest as a gate row's output
    flat = set(int(v) for v in wires.ravel())
    assert all(v in flat for v in needles)
    return dict(x=x, cells=cells, values=values, pis=pis, wires=wires, n=n, needles=np.array(needles, dtype=np.uint64))


def regions(first):
    return sorted(set(h["region"] for h in first))


def test_scan_sees_a_resident_witness_and_scrub_removes_it(pkg, ctx, full, case):
    """1. qpgpu_prove_batch_dev over two separately allocated witnesses gathers them into the workspace: the scan finds them there."""
    circ = pkg.Circuit(ctx, full.pack, max_batch=2)
    bufs = [ctx.alloc(NW * case["n"] * 8) for _ in range(2)]
    bufs.sort(key=lambda b: -b.ptr)                   # the second one lies below the first: never the dense [2][..] layout
    for b in bufs:
        circ.generate_witness_partial_dev(case["cells"], case["values"], case["pis"], b)
    proofs = circ.prove_batch_dev([b.ptr for b in bufs], [case["pis"], case["pis"]])
    assert proofs[0] == proofs[1]
    hits, first, nbytes = ctx.residue_scan(case["needles"], cap=64)
    assert hits >= 1 and "circuit-workspace" in regions(first), (hits, first)
    for h in first:
        assert h["word"] in set(int(v) for v in case["needles"])
        assert h["offset_words"] * 8 + 8 <= h["alloc_bytes"]
    ws = [h for h in first if h["region"] == "circuit-workspace" and not h["pinned"]]
    assert ws and max(h["alloc_bytes"] for h in ws) >= 2 * NW * case["n"] * 8         # the gathered witnesses' buffer
    # bytes_scanned: the tracked sizes of the scanned regions, region by region
    names = pkg.binding.residue_regions()
    per = {r: ctx.residue_scan(case["needles"], regions=[r])[2] for r in names}
    default = [r for r in names if r not in ("circuit-setup", "tables", "zk-tree", "verify-staging")]
    assert nbytes == sum(per[r] for r in default)
    assert ctx.residue_scan(case["needles"], regions=(1 << len(names)) - 1)[2] == sum(per.values())
    assert per["circuit-workspace"] >= 2 * NW * case["n"] * 8 and per["circuit-setup"] > 0
    # sizes known from outside the scan: the bounce buffer of a fresh context is its 1 MiB floor (two leaf proofs need less), and
    # every hit's alloc_bytes is a size the region's total is made of
    assert per["ctx-pinned"] == 1 << 20
    assert 2 * pkg.pack_header(full.pack)["num_wires"] * case["n"] * 8 == 2 * NW * case["n"] * 8 in [h["alloc_bytes"] for h in ws]      # d_wires_vals: [max_batch][num_wires][n]
    assert per["oracle"] == per["pool-witness"] == per["fri-session"] == per["stage-plan"] == 0
    # the caller's own buffers are not the library's: the witnesses in `bufs` are not scanned (hits only in tracked regions)
    assert set(regions(first)) <= set(names)
    circ.scrub()
    hits, first, nbytes2 = ctx.residue_scan(case["needles"])
    assert hits == 0 and first == [] and nbytes2 == nbytes
    for b in bufs:
        b.free(scrub=True)
    circ.close()


def test_host_prove_entry_leaves_nothing(pkg, ctx, full, case):
    """2. qpgpu_prove (host witness in, proof out) scrubs: workspace, stage s1 buffers, the context's scratch and bounce buffer."""
    circ = pkg.Circuit(ctx, full.pack)
    # stage s1 first, so that the witness plan and the bounce buffer have been used with these inputs
    d = ctx.alloc(NW * case["n"] * 8)
    circ.generate_witness_partial_dev(case["cells"], case["values"], case["pis"], d)
    d.free(scrub=True)
    proof = circ.prove(case["wires"], case["pis"])
    hits, first, nbytes = ctx.residue_scan(case["needles"])
    assert hits == 0, first
    assert nbytes > NW * case["n"] * 8
    ver = pkg.Verifier(full.pack, circuit=circ)
    assert ver.verify(proof)
    ver.close(); circ.close()
    # qpgpu_generate_witness, host form ("uploaded, generated, downloaded, device copy scrubbed"), on a circuit whose free cells
    # are a wire-matrix mask: the generated witness is in no library-owned buffer afterwards
    pack, wires, pis = pkg.synth_circuit(8, seed=4, poseidon=True, base_sum=True, ext_arith=True, recursion=True, poseidon2=True)
    sc = pkg.Circuit(ctx, pack)
    mask = sc.witness_free_mask(*wires.shape)
    got = sc.generate_witness(np.where(mask == 1, wires, 0).astype(np.uint64), pis)
    assert np.array_equal(got, wires)
    pub = set(int(v) for v in pis)                            # public inputs are public: the plan keeps their values
    gen = words_of([v for v in wires[mask == 0] if int(v) not in pub], 8)       # words the device generated
    free = words_of([v for v in wires[mask == 1] if int(v) not in pub], 8)      # words the caller supplied
    hits, first, _ = ctx.residue_scan(np.concatenate([gen, free]))
    assert hits == 0, first
    sc.close()


def test_partial_witness_entry_leaves_no_assignment_behind(pkg, ctx, L, full, case):
    """3. qpgpu_generate_witness_partial_batch_dev, batch 2: the assignments (the secret's limbs among them) went through the pinned
    bounce buffer and the prepared value buffers; both are clean when the call has returned, also for an unsatisfiable witness."""
    circ = pkg.Circuit(ctx, full.pack, max_batch=2)
    d = ctx.alloc(2 * NW * case["n"] * 8)
    vals = np.stack([case["values"], case["values"]]); pis = np.stack([case["pis"], case["pis"]])
    only = ["partial-witness", "ctx-pinned"]
    assert circ.generate_witness_partial_batch_dev(case["cells"], vals, pis, d) == [0, 0]
    hits, first, nbytes = ctx.residue_scan(case["needles"], regions=only)
    assert hits == 0 and nbytes > 0, first
    got = d.download().reshape(2, NW, case["n"])
    assert np.array_equal(got[0], case["wires"]) and np.array_equal(got[1], case["wires"])       # d_wires is the caller's: not scanned, not touched
    assert ctx.residue_scan(case["needles"])[0] == 0                                              # nothing else of the library's holds them either
    # one witness with a conflicting assignment: a secret the account is not derived from (a dummy still binds the unspendable account)
    bad = case["x"].copy(); bad.secret[31] ^= 0x10
    cb = full.commit(bad)
    assert np.array_equal(cb[0], case["cells"])
    st = circ.generate_witness_partial_batch_dev(case["cells"], np.stack([case["values"], cb[1]]), np.stack([case["pis"], cb[2]]), d)
    assert st == [0, -4]
    hits, first, _ = ctx.residue_scan(case["needles"], regions=only)
    assert hits == 0, first
    assert ctx.residue_scan(case["needles"])[0] == 0
    d.free(scrub=True); circ.close()


def test_blinded_entry_leaves_neither_keys_nor_draws(pkg, ctx, case):
    """4. ..._partial_batch_blinded_dev with seeds: the ChaCha key words and a drawn value are in no library-owned buffer afterwards."""
    import test_builder_gadgets_gpu as bg
    pack, cells, ni, no = bg.gadget_circuit(pkg, 0)
    cin = cells[:ni.value]
    nb = 2                                             # its last two inputs are drawn on the device
    rng = np.random.default_rng(41)
    vals = rng.integers(1 << 32, P, (2, cin.size - nb), dtype=np.uint64)
    seeds = rng.integers(1 << 32, 1 << 63, 8, dtype=np.uint64)       # two keys of four 64-bit words
    circ = pkg.Circuit(ctx, pack, max_batch=2)
    rows = 1 << int(pack[1])
    d = ctx.alloc(2 * NW * rows * 8)
    st = circ.generate_witness_partial_batch_blinded_dev(cin, vals, None, d, nb, seeds.tobytes())
    assert st == [0, 0], ctx.last_error()
    w = d.download().reshape(2, NW, rows)
    drawn = [int(w[b, int(c) % NW, int(c) // NW]) for b in range(2) for c in cin[-nb:]]
    assert len(set(drawn)) == 4 and all(v >= 1 << 32 for v in drawn)                   # the draw happened, per witness
    assert [int(w[0, int(c) % NW, int(c) // NW]) for c in cin[:-nb]] == [int(v) for v in vals[0]]
    needles = np.concatenate([seeds, np.array(drawn, dtype=np.uint64), vals[0][:4]])
    assert needles.size <= 16
    hits, first, nbytes = ctx.residue_scan(needles)
    assert hits == 0 and nbytes > 0, first
    # reproducible under the same seeds (the keys were used, not ignored)
    d2 = ctx.alloc(2 * NW * rows * 8)
    assert circ.generate_witness_partial_batch_blinded_dev(cin, vals, None, d2, nb, seeds.tobytes()) == [0, 0]
    assert np.array_equal(d2.download(), d.download())
    assert ctx.residue_scan(needles)[0] == 0
    d.free(scrub=True); d2.free(scrub=True); circ.close()


def words_of(arr, k=6):
    out = [int(v) for v in np.asarray(arr, dtype=np.uint64).ravel() if int(v) >= 1 << 32]
    out = list(dict.fromkeys(out))[:k]
    assert len(out) == k
    return np.array(out, dtype=np.uint64)


def test_audit_at_release(pkg, ctx, orc, full, case):
    """5. The promises that end in a free: the buffer is scanned after the release path's scrub, right before the allocator gets it."""
    rng = np.random.default_rng(17)
    polys = rng.integers(1 << 32, P, size=(4, 256), dtype=np.uint64)
    # qpgpu_oracle_free
    o = pkg.PolyOracle(ctx, polys, rate_bits=3, cap_height=4)
    needles = words_of(o.read(lde=False))
    hits, first, _ = ctx.residue_scan(needles)
    assert hits >= needles.size and regions(first) == ["oracle"]
    with ctx.residue_audit(needles) as a:
        o.close()
    assert a.buffers_released >= 1 and a.hits == 0, a.first_hits
    assert ctx.residue_scan(needles, regions=["oracle"])[1:] == ([], 0)                  # the entry went with the buffer
    # qpgpu_fri_session_free: the session's workspace holds the final polynomial it handed out
    o = pkg.PolyOracle(ctx, polys, rate_bits=3, cap_height=4)
    s = pkg.FriSession(ctx, [o], [([3, 5], [(0, 0, 4)])], [7, 11], [2], rate_bits=3, cap_height=4)
    s.round_commit(); s.round_fold([13, 17])
    fin = words_of(s.final_poly())
    hits, first, _ = ctx.residue_scan(fin)
    assert hits >= 1 and "fri-session" in regions(first), first
    with ctx.residue_audit(np.concatenate([fin, needles])) as a:
        s.close()
    assert a.buffers_released >= 2 and a.hits == 0, a.first_hits                          # the workspace and its pinned ring
    assert ctx.residue_scan(fin, regions=["fri-session"])[1:] == ([], 0)                 # (the bounce buffer it was read back through still has it: proof data)
    o.close()
    # qpgpu_stage_plan_free: the plan's copy of a host witness
    pack, wires, pis = pkg.synth_circuit(8, seed=64, poseidon=True)
    fl = sp.Flow(pkg, ctx, orc, pack)
    ones = [1] * fl.plan.num_challenges
    d_zs = fl.plan.partial_products(wires, ones, ones)
    consts = set(int(v) for v in np.asarray(fl.h["constants_sigmas"]).ravel())           # a wire that carries a circuit constant is public
    wn = words_of([v for v in wires[:, 3:].ravel() if int(v) not in consts])
    hits, first, _ = ctx.residue_scan(wn, regions=["stage-plan"])
    assert hits >= wn.size and regions(first) == ["stage-plan"]
    with ctx.residue_audit(wn) as a:
        fl.plan.close()
    assert a.buffers_released >= 1 and a.hits == 0, a.first_hits
    fl.o_cs.close(); d_zs.free(scrub=True)
    # qpgpu_circuit_free after qpgpu_prove_dev (and a scattered batch before it, so that the workspace holds a witness copy)
    circ = pkg.Circuit(ctx, full.pack, max_batch=2)
    bufs = sorted([ctx.alloc(NW * case["n"] * 8) for _ in range(2)], key=lambda b: -b.ptr)
    for b in bufs:
        circ.generate_witness_partial_dev(case["cells"], case["values"], case["pis"], b)
    circ.prove_batch_dev([b.ptr for b in bufs], [case["pis"], case["pis"]])
    circ.prove_dev(bufs[0], case["pis"])
    hits, first, _ = ctx.residue_scan(case["needles"])
    assert hits >= 1 and "circuit-workspace" in regions(first)
    with ctx.residue_audit(case["needles"]) as a:
        circ.close()
    assert a.buffers_released >= 10 and a.hits == 0, a.first_hits
    for b in bufs:
        b.free(scrub=True)
    assert ctx.residue_scan(case["needles"])[0] == 0


def test_more_hits_in_a_buffer_than_the_kernel_records(pkg, ctx):
    """The kernel keeps the first 64 hits of a buffer and counts all of them: with a larger cap the caller gets 64 real entries, none
    made up. A constant polynomial's low-degree extension is that constant at all 2^11 points. Five columns, so that a Merkle leaf is
    hashed (a leaf of four elements or fewer is its own digest in plonky2, hash_or_noop, and the constant would be in the tree too)."""
    C = 0xC0FFEE0123456789
    polys = np.random.default_rng(3).integers(1 << 32, P, size=(5, 256), dtype=np.uint64)
    polys[2, :] = C
    o = pkg.PolyOracle(ctx, polys, rate_bits=3, cap_height=4)
    assert int(o.read(lde=False)[2, 0]) == C
    hits, first, nbytes = ctx.residue_scan([C], regions=["oracle"], cap=100)
    assert hits == 2048 + 1 and len(first) == 64             # every LDE point and the constant coefficient
    assert all(h["word"] == C and h["region"] == "oracle" and h["alloc_bytes"] == nbytes and h["offset_words"] * 8 < nbytes for h in first)
    assert len(set(h["offset_words"] for h in first)) == 64
    hits2, first2, _ = ctx.residue_scan([C], regions=["oracle"], cap=10)
    assert hits2 == hits and len(first2) == 10
    with ctx.residue_audit([C]) as a:
        o.close()
    assert a.hits == 0 and a.buffers_released == 1


def test_pool_scrub(pkg, ctx, L, full, case):
    """6. A pool keeps its workers' workspaces resident by contract; qpgpu_pool_scrub clears them between jobs and breaks nothing."""
    prover = L.LeafProver(pkg, ctx, full)
    pool = prover.pool(workers=2, max_batch=2)
    xs = [case["x"], lc.dummy_inputs(L), case["x"], lc.test_inputs(L, 1)]
    first4 = [pool.wait(t) for t in [prover.submit(pool, x) for x in xs]]
    hits, first, nbytes = pool.residue_scan(case["needles"], cap=32)
    assert hits >= 1 and "pool-witness" in regions(first), first
    # bytes_scanned against sizes known from outside: per worker max_batch wire matrices, and the 1 MiB bounce buffer
    assert pool.residue_scan(case["needles"], regions=["pool-witness"])[2] == 2 * 2 * NW * case["n"] * 8
    assert pool.residue_scan(case["needles"], regions=["ctx-pinned"])[2] == 2 << 20
    assert all(h["alloc_bytes"] == 2 * NW * case["n"] * 8 for h in first if h["region"] == "pool-witness")
    assert set(regions(first)) <= {"pool-witness", "circuit-workspace"}, first          # stage s1's staging is clean between jobs
    pool.scrub()
    assert pool.residue_scan(case["needles"]) == (0, [], nbytes)
    again = [pool.wait(t) for t in [prover.submit(pool, x) for x in xs]]
    assert again == first4
    assert first4[0] == first4[2] and first4[0] != first4[1]
    assert pool.residue_scan(case["needles"])[0] >= 1
    prover.scrub()                                                                       # LeafProver.scrub forwards to its pools
    assert pool.residue_scan(case["needles"])[0] == 0
    with pytest.raises(pkg.QpGpuError) as e:
        pool.residue_scan([5])
    assert e.value.code == -1 and "needle 0" in str(e.value)
    pool.close(); prover.close()


def test_refusals(pkg, ctx):
    """7."""
    good = [0xDEADBEEFCAFEF00D, 1 << 32]
    assert ctx.residue_scan(good)[0] == 0
    for bad, what in (([good[0], 0xFFFFFFFF], "needle 1"), ([7], "needle 0"), ([], "needle count"), ([good[0]] * 17, "needle count")):
        with pytest.raises(pkg.QpGpuError) as e:
            ctx.residue_scan(bad)
        assert e.value.code == -1 and what in str(e.value), str(e.value)
    assert ctx.residue_scan([good[0]] * 16)[0] == 0
    nreg = len(pkg.binding.residue_regions())
    for mask in (1 << nreg, 1 << 63, (1 << nreg) | 2):
        with pytest.raises(pkg.QpGpuError) as e:
            ctx.residue_scan(good, regions=mask)
        assert e.value.code == -1 and "region" in str(e.value)
    assert ctx.residue_scan(good, regions=(1 << nreg) - 1)[0] == 0
    hits, rel = ctypes.c_uint64(), ctypes.c_uint64()
    assert ctx.lib.qpgpu_ctx_residue_audit_end(ctx.ctx, ctypes.byref(hits), None, 0, ctypes.byref(rel)) == -1
    assert "audit_end without audit_begin" in ctx.last_error()
    with pytest.raises(pkg.QpGpuError):
        with ctx.residue_audit([3]):
            pass
    with ctx.residue_audit(good) as a:
        nd = np.array(good, dtype=np.uint64)
        assert ctx.lib.qpgpu_ctx_residue_audit_begin(ctx.ctx, nd.ctypes.data, 2) == -1         # one audit at a time
    assert (a.hits, a.buffers_released, a.first_hits) == (0, 0, [])


def test_proof_bytes_are_the_oracles_with_an_audit_open(pkg, ctx, orc, L, full, case):
    """8. Nothing observable changes: the leaf proof equals the CPU oracle's byte for byte, also while an audit is open."""
    wires, want, pis = None, None, None
    cells, values, pis = full.commit(case["x"])
    rc, wires, _ = orc.generate_witness(full.pack, cells, values, pis)
    assert rc == orc.WIT_OK and np.array_equal(wires, case["wires"])
    oc = ob.OracleCircuit(orc, full.pack)
    want = oc.prove(wires, pis)
    assert oc.verify(want) == 0
    oc.close()
    prover = L.LeafProver(pkg, ctx, full)
    assert prover.prove(case["x"])[0] == want
    with ctx.residue_audit(case["needles"]) as a:
        assert prover.prove(case["x"])[0] == want
        assert np.array_equal(prover.witness(), wires)
    assert a.hits == 0
    prover.close()
