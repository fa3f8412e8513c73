"""The FRI opening proof one step at a time on the device (qpgpu_fri_session, qpgpu_fri_grind, qpgpu_oracle_open): the steps, driven
by the host challenger in qpgpu_fri_prove's order, give qpgpu_fri_prove's bytes and leave the challenger where it leaves it; inside the
whole stage flow they give the CPU restatement's proof; with betas and indices no challenger produced they still give a FriProof the
Python-integer replay of tests/fri_schedules.py accepts. Exact arithmetic: every comparison is equality. Shapes: 2^5 .. 2^9 rows, three
or four query indices."""
import ctypes

import numpy as np
import pytest

import fri_schedules as fs
import leaf_cases as lc
import test_stage_plan_gpu as sp
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu
P = fs.P


def steps_fri_prove(gpu, oracles, batches, challenger, reduction_arity_bits, rate_bits=3, cap_height=4, proof_of_work_bits=16,
                    num_query_rounds=28, pkg=None, between=None):
    """pkg.fri_prove's signature and result through the step entries: the specification of include/qpgpu.h. `between` is called
    with (session, stage name) before each step (the misuse test makes its out-of-order calls there)."""
    ch, arity = challenger, list(reduction_arity_bits)
    between = between or (lambda s, where: None)
    alpha = ch.get_n(2)
    caps = []
    with pkg.FriSession(gpu, oracles, batches, alpha, arity, rate_bits=rate_bits, cap_height=cap_height) as s:
        for r in range(len(arity)):
            between(s, "commit")
            caps.append(s.round_commit())
            ch.observe(caps[-1])
            between(s, "fold")
            s.round_fold(ch.get_n(2))
        between(s, "end")
        final = s.final_poly()
        ch.observe(final)
        nonce = pkg.fri_grind(gpu, ch, proof_of_work_bits)
        ch.observe([nonce])
        ch.get()
        queries = s.open([ch.get() % s.lde_size for _ in range(num_query_rounds)])
    return b"".join(c.tobytes() for c in caps) + queries + final.tobytes() + np.uint64(nonce).tobytes()


def state_fields(ch):
    s = ch.state
    return dict(sponge_state=list(s.sponge_state), input_buffer=list(s.input_buffer)[:s.input_len],
                output_buffer=list(s.output_buffer)[:s.output_len], input_len=s.input_len, output_len=s.output_len)


def one_oracle(pkg, gpu, degree_bits, rate_bits, cap_height, seed, **kw):
    rng = np.random.default_rng(seed)
    polys = rng.integers(0, P, size=(3, 1 << degree_bits), dtype=np.uint64)
    point = [int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64)]
    return pkg.PolyOracle(gpu, polys, rate_bits=rate_bits, cap_height=cap_height, **kw), point


def started_challenger(pkg, gpu, seed):
    ch = pkg.Challenger(gpu)
    ch.observe(np.arange(seed, seed + 11, dtype=np.uint64))
    ch.get()
    ch.observe([seed, 7])                       # FRI begins with inputs buffered, as after the openings
    return ch


# (degree_bits, rate_bits, cap_height, schedule, proof_of_work_bits): each listed value of each parameter at least once; [8] at
# (9, 3, 4) leaves a tree that is the cap itself (path length 0); [4, 4] at degree 8 a final polynomial of one coefficient
STEP_CASES = [
    (5, 1, 0, [], 0),
    (5, 3, 2, [1], 4),
    (8, 1, 4, [4], 10),
    (8, 3, 2, [3, 2], 0),
    (9, 3, 4, [1, 2, 3], 4),
    (8, 3, 0, [4, 4], 10),
    (9, 3, 4, [8], 4),
    (9, 1, 0, [3, 2], 10),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "d%d_r%d_c%d_%s_pow%d" % (c[0], c[1], c[2], "-".join(map(str, c[3])) or "none", c[4]))
def test_steps_equal_the_single_call(pkg, gpu, case):
    d, rate, cap, arity, pow_bits = case
    o, point = one_oracle(pkg, gpu, d, rate, cap, seed=100 + d + rate + cap + len(arity))
    try:
        batches = [(point, [(0, 0, 3)])]
        kw = dict(rate_bits=rate, cap_height=cap, proof_of_work_bits=pow_bits, num_query_rounds=3)
        ch_a, ch_b = started_challenger(pkg, gpu, 5), started_challenger(pkg, gpu, 5)
        want = pkg.fri_prove(gpu, [o], batches, ch_a, arity, **kw)
        got = steps_fri_prove(gpu, [o], batches, ch_b, arity, pkg=pkg, **kw)
        lay = fs.FriLayout(d, rate, cap, arity, 3, [3])
        assert len(want) == lay.total == len(got)
        assert got == want, "steps differ from qpgpu_fri_prove at byte %d" % next(i for i in range(len(got)) if got[i] != want[i])
        if arity == [8]:
            assert lay.rounds[0][1] == 0 and got[lay.queries_pos + lay.rounds[0][0] + 16 * 256] == 0     # the last tree is the cap
        a, b = state_fields(ch_a), state_fields(ch_b)
        for k in a:
            assert a[k] == b[k], k
        assert bytes(ch_a.state) == bytes(ch_b.state)
    finally:
        o.close()


class Counted:
    def __init__(self, pkg):
        self.pkg, self.calls = pkg, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return steps_fri_prove(*a, pkg=self.pkg, **kw)


@pytest.mark.parametrize("zk", [False, True], ids=["plain", "zero_knowledge"])
def test_stage_flow_over_the_steps_reproduces_the_cpu_proof(pkg, gpu, orc, monkeypatch, zk):
    """Two opening points, four oracles, salted leaves under zero knowledge: the Flow of tests/test_stage_plan_gpu.py with the
    steps in place of its pkg.fri_prove call, against the CPU restatement's proof."""
    pack, wires, pis = pkg.synth_circuit(8, seed=64, poseidon=True)
    seed = 0
    if zk:
        pack = pack.copy(); pack[14] = 1
        seed = 4242
    oc = OracleCircuit(orc, pack)
    want = oc.prove(wires, pis, seed=seed) if zk else oc.prove(wires, pis)
    stepped = Counted(pkg)
    monkeypatch.setattr(pkg, "fri_prove", stepped)
    fl = sp.Flow(pkg, gpu, orc, pack)
    try:
        got = fl.prove(wires, pis, seed=seed)[0]
        assert stepped.calls == 1
        assert len(got) == len(want)
        assert got == want, "stage flow over the steps differs from the CPU proof at byte %d" % next(i for i in range(len(got)) if got[i] != want[i])
        assert oc.verify(got) == 0
    finally:
        fl.close(); oc.close()


def test_leaf_circuit_flow_over_the_steps(pkg, gpu, orc, monkeypatch):
    """The restated leaf circuit at its own 2^8 rows, witness made on the device: the flow over the steps equals qpgpu_prove_dev."""
    L = pkg.leaf
    leaf = L.LeafCircuit(min_degree_bits=8)
    hdr = pkg.pack_header(leaf.pack)
    assert hdr["degree_bits"] == 8
    cells, values, pis = leaf.commit(lc.real_inputs(L, depth=3))
    circ = pkg.Circuit(gpu, leaf.pack)
    d_w = gpu.alloc(hdr["num_wires"] * 256 * 8)
    stepped = Counted(pkg)
    fl = sp.Flow(pkg, gpu, orc, leaf.pack)
    try:
        circ.generate_witness_partial_dev(cells, values, pis, d_w)
        want = circ.prove_dev(d_w, pis)
        monkeypatch.setattr(pkg, "fri_prove", stepped)
        got = fl.prove(None, pis, d_wires=d_w)[0]
        assert stepped.calls == 1 and got == want
    finally:
        fl.close(); d_w.free(scrub=True); circ.close()


@pytest.mark.parametrize("arity", [[4], [3, 2], [1, 2, 3]], ids=lambda a: "-".join(map(str, a)))
def test_session_assumes_nothing_about_the_transcript(pkg, gpu, arity):
    """Betas and query indices that no challenger produced. The FriProof assembled from the caps, the openings and the final
    polynomial passes the Python-integer replay of the commit phase."""
    d, rate, cap = 6, 3, 2
    o, point = one_oracle(pkg, gpu, d, rate, cap, seed=31)
    fixed = [(3, 5), (P - 1, 1), (0x123456789, 0)]
    betas = fixed[:len(arity)]
    indices = [0, (1 << (d + rate)) - 1, 77, 77]
    try:
        with pkg.FriSession(gpu, [o], [(point, [(0, 0, 3)])], (11, 13), arity, rate_bits=rate, cap_height=cap) as s:
            caps = []
            for b in betas:
                caps.append(s.round_commit())
                s.round_fold(b)
            queries = s.open(indices)
            final = s.final_poly()
            again = s.open(indices[2:])                                  # any number of times, after the final polynomial too
            assert s.query_size * 4 == len(queries) and again == queries[2 * s.query_size:]
            assert queries[2 * s.query_size:3 * s.query_size] == queries[3 * s.query_size:]      # the repeated index
        fri = b"".join(c.tobytes() for c in caps) + queries + final.tobytes() + bytes(8)
        lay = fs.FriLayout(d, rate, cap, arity, len(indices), [3])
        assert lay.q_bytes * 4 == len(queries)
        assert fs.python_fri_check(fri, lay, betas, indices) == []
        # the check sees a wrong value: one evaluation of the last round, of the last query, changed
        off = lay.queries_pos + 3 * lay.q_bytes + lay.rounds[-1][0]
        broken = bytearray(fri); broken[off] ^= 1
        assert fs.python_fri_check(bytes(broken), lay, betas, indices) != []
    finally:
        o.close()


def read_digests(pkg, gpu, o):
    """The oracle's digest array straight from the device: a list of levels, leaf layer first, the cap last."""
    L = o.degree_bits + o.rate_bits
    d_dig = ctypes.c_void_p()
    gpu._check(gpu.lib.qpgpu_oracle_device_ptrs(o.h, None, None, ctypes.byref(d_dig)))
    words = ((2 << L) - (1 << o.cap_height)) * 4
    flat = np.empty(words, dtype=np.uint64)
    gpu._check(gpu.lib.qpgpu_memcpy_d2h(gpu.ctx, flat.ctypes.data, d_dig, flat.nbytes))
    levels, at = [], 0
    for lvl in range(L - o.cap_height + 1):
        cnt = 1 << (L - lvl)
        levels.append(flat[at:at + 4 * cnt].reshape(cnt, 4))
        at += 4 * cnt
    assert at == words
    return levels


@pytest.mark.parametrize("blinded", [False, True], ids=["plain", "blinded"])
def test_oracle_open(pkg, gpu, blinded):
    d, rate, cap = 6, 3, 2
    L = d + rate
    o, point = one_oracle(pkg, gpu, d, rate, cap, seed=41, **(dict(blinding=True, blinding_seed=99, blinding_stream=1) if blinded else {}))
    try:
        width = 3 + (4 if blinded else 0)
        assert o.leaf_width == width
        # the queries of a fri_prove over this oracle: its indices are the ones opened, so that its bytes give the salt words
        ch = started_challenger(pkg, gpu, 9)
        replay = fs.copy_challenger(pkg, ch)
        proof = pkg.fri_prove(gpu, [o], [(point, [(0, 0, 3)])], ch, [2], rate_bits=rate, cap_height=cap, proof_of_work_bits=0, num_query_rounds=4)
        lay = fs.FriLayout(d, rate, cap, [2], 4, [width])
        _, qidx = fs.replay_transcript(replay, proof, lay)
        indices = qidx + [0, (1 << L) - 1, qidx[0]]                       # the first and last leaf, and a repeated index
        rows, paths = o.open(indices)
        lde = o.read(lde=True)
        levels = read_digests(pkg, gpu, o)
        assert rows.shape == (7, width) and paths.shape == (7, L - cap, 4)
        for k, idx in enumerate(indices):
            assert np.array_equal(rows[k, :3], lde[:, idx]), k
            for lvl in range(L - cap):
                assert np.array_equal(paths[k, lvl], levels[lvl][(idx >> lvl) ^ 1]), (k, lvl)
        for q in range(4):                                                 # the leaf and the path as the proof carries them
            at = lay.queries_pos + q * lay.q_bytes
            assert rows[q].tobytes() == proof[at:at + 8 * width], q
            assert proof[at + 8 * width] == L - cap and paths[q].tobytes() == proof[at + 8 * width + 1:at + 8 * width + 1 + 32 * (L - cap)]
        if blinded:
            assert len({rows[k, 3:].tobytes() for k in range(6)}) == len(set(indices[:6]))   # salts differ from leaf to leaf
        assert np.array_equal(rows[6], rows[0]) and np.array_equal(paths[6], paths[0])
        # either output alone; none at all
        only_rows, none = o.open(indices, paths=False)
        assert none is None and np.array_equal(only_rows, rows)
        none, only_paths = o.open(indices, rows=False)
        assert none is None and np.array_equal(only_paths, paths)
        r0, p0 = o.open([])
        assert r0.shape == (0, width) and p0.shape == (0, L - cap, 4)
        # an index out of range at entry 2 of 4: named, nothing written
        bad = np.array([1, 2, 1 << L, 3], dtype=np.uint64)
        r_fill, p_fill = np.full((4, width), 0xA5A5, dtype=np.uint64), np.full((4, L - cap, 4), 0xA5A5, dtype=np.uint64)
        rc = gpu.lib.qpgpu_oracle_open(o.h, bad.ctypes.data, 4, r_fill.ctypes.data, p_fill.ctypes.data)
        assert rc == -1 and "oracle_open" in gpu.last_error() and "indices[2]" in gpu.last_error() and str(1 << L) in gpu.last_error()
        assert (r_fill == 0xA5A5).all() and (p_fill == 0xA5A5).all()
    finally:
        o.close()


def brute_force_nonce(pkg, ch, bits, limit=1 << 14):
    for w in range(limit):
        c = fs.copy_challenger(pkg, ch)
        c.observe([w])
        if c.get() >> (64 - bits) == 0:
            return w
    raise AssertionError("no nonce below %d" % limit)


@pytest.mark.parametrize("input_len", range(8))
def test_grind_is_the_minimum_nonce(pkg, gpu, input_len):
    ch = pkg.Challenger(gpu)
    ch.observe(np.arange(3, 20, dtype=np.uint64))
    ch.get()
    if input_len:
        ch.observe(np.arange(1000, 1000 + input_len, dtype=np.uint64))
    assert ch.state.input_len == input_len
    before = bytes(ch.state)
    assert pkg.fri_grind(gpu, ch, 0) == 0
    for bits in (1, 6, 8):
        want = brute_force_nonce(pkg, ch, bits)
        got = pkg.fri_grind(gpu, ch, bits)
        print("input_len %d bits %d: nonce %d (brute force %d)" % (input_len, bits, got, want))
        assert got == want, (input_len, bits)
        assert bytes(ch.state) == before
    if input_len == 0:
        with pytest.raises(pkg.QpGpuError) as e:
            pkg.fri_grind(gpu, ch, 41)
        assert e.value.code == -1 and "proof_of_work_bits" in str(e.value)
        full = fs.copy_challenger(pkg, ch)
        full.state.input_len = 8
        with pytest.raises(pkg.QpGpuError) as e:
            pkg.fri_grind(gpu, full, 4)
        assert e.value.code == -1 and "challenger state" in str(e.value)
        assert bytes(ch.state) == before


def test_misuse_on_a_live_session(pkg, gpu):
    """Every out-of-order call is refused with its message, wrong buffer sizes name the argument, nothing is written, and the
    session goes on to produce the bytes of the first test's [3, 2] case."""
    d, rate, cap, arity, pow_bits = STEP_CASES[3]
    o, point = one_oracle(pkg, gpu, d, rate, cap, seed=100 + d + rate + cap + len(arity))
    lib = gpu.lib
    fill = np.full(4096, 0xA5, dtype=np.uint8)
    seen = []

    def refused(rc, *parts):
        msg = gpu.last_error()
        assert rc == -1 and all(p in msg for p in parts), (rc, msg)
        assert (fill == 0xA5).all()
        seen.append(msg)

    def between(s, where):
        two = np.array([1, 2], dtype=np.uint64)
        n = ctypes.c_size_t(55)
        capw, buf = 4 << cap, fill.ctypes.data
        if where == "commit":               # a round waits to be committed
            refused(lib.qpgpu_fri_round_fold(s.h, two.ctypes.data), "fri_round_fold", "no committed round", "qpgpu_fri_round_commit")
            refused(lib.qpgpu_fri_final_poly(s.h, buf, 2 * s.final_len, ctypes.byref(n)), "fri_final_poly", "before the last fold")
            refused(lib.qpgpu_fri_open(s.h, two.ctypes.data, 2, buf, 4096, ctypes.byref(n)), "fri_open", "before the last fold")
            refused(lib.qpgpu_fri_round_commit(s.h, buf, capw + 1), "fri_round_commit", "cap_words")
            refused(lib.qpgpu_fri_round_commit(s.h, None, capw), "fri_round_commit", "cap_out")
        elif where == "fold":               # a committed round waits for its beta
            refused(lib.qpgpu_fri_round_commit(s.h, buf, capw), "fri_round_commit", "waits for its fold", "qpgpu_fri_round_fold")
            refused(lib.qpgpu_fri_final_poly(s.h, buf, 2 * s.final_len, ctypes.byref(n)), "fri_final_poly", "qpgpu_fri_round_fold")
            refused(lib.qpgpu_fri_open(s.h, two.ctypes.data, 2, buf, 4096, ctypes.byref(n)), "fri_open", "qpgpu_fri_round_fold")
            refused(lib.qpgpu_fri_round_fold(s.h, None), "fri_round_fold", "beta")
        else:                               # after the last fold
            refused(lib.qpgpu_fri_round_commit(s.h, buf, capw), "fri_round_commit", "rounds are folded")
            refused(lib.qpgpu_fri_round_fold(s.h, two.ctypes.data), "fri_round_fold", "no committed round")
            refused(lib.qpgpu_fri_final_poly(s.h, buf, 2 * s.final_len - 1, ctypes.byref(n)), "fri_final_poly", "out_words")
            refused(lib.qpgpu_fri_final_poly(s.h, buf, 2 * s.final_len + 2, ctypes.byref(n)), "fri_final_poly", "out_words")
            refused(lib.qpgpu_fri_open(s.h, two.ctypes.data, 2, buf, 2 * s.query_size - 1, ctypes.byref(n)), "fri_open", "out_cap")
            out_of_range = np.array([0, 1, 1 << (d + rate), 2], dtype=np.uint64)
            big = np.full(4 * s.query_size, 0xA5, dtype=np.uint8)
            refused(lib.qpgpu_fri_open(s.h, out_of_range.ctypes.data, 4, big.ctypes.data, big.size, ctypes.byref(n)), "fri_open", "indices[2]")
            assert (big == 0xA5).all()
            assert lib.qpgpu_fri_open(s.h, None, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0     # n = 0 is an empty answer
            n.value = 55
        assert n.value == 55

    try:
        batches = [(point, [(0, 0, 3)])]
        kw = dict(rate_bits=rate, cap_height=cap, proof_of_work_bits=pow_bits, num_query_rounds=3)
        ch_a, ch_b = started_challenger(pkg, gpu, 5), started_challenger(pkg, gpu, 5)
        want = pkg.fri_prove(gpu, [o], batches, ch_a, arity, **kw)
        got = steps_fri_prove(gpu, [o], batches, ch_b, arity, pkg=pkg, between=between, **kw)
        assert len(seen) == 2 * 5 + 2 * 4 + 6
        assert got == want and bytes(ch_a.state) == bytes(ch_b.state)
        # what qpgpu_fri_prove refuses, qpgpu_fri_begin refuses in the same words; *out stays NULL
        for bad_arity in ([9], [5, 5]):
            with pytest.raises(pkg.QpGpuError) as e_one:
                pkg.fri_prove(gpu, [o], batches, started_challenger(pkg, gpu, 5), bad_arity, **kw)
            with pytest.raises(pkg.QpGpuError) as e_step:
                pkg.FriSession(gpu, [o], batches, (1, 2), bad_arity, rate_bits=rate, cap_height=cap)
            assert str(e_one.value) == str(e_step.value) and e_step.value.code == -1
        with pytest.raises(pkg.QpGpuError) as e_step:
            pkg.FriSession(gpu, [o], [(point, [(0, 2, 2)])], (1, 2), arity, rate_bits=rate, cap_height=cap)
        assert "polynomial range outside its oracle" in str(e_step.value)
    finally:
        o.close()


def test_stage_example_in_c_with_the_fri_steps(tmp_path):
    """examples/stage_prove_example.c with its second argument: the FRI part from the step entries, the transcript kept in C; the
    example compares its bytes with qpgpu_prove's itself."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "qpgpu_stage_prove_example_steps")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "stage_prove_example.c"),
                           "-L", os.path.join(root, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(root, "qp-zk-circuits_amd"), "-o", out])
    res = subprocess.run([out, "8", "steps"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "staged flow, FRI step by step, == qpgpu_prove" in res.stdout
