"""qpgpu_fri_verifier_* / qpgpu_fri_verify on the host (include/qpgpu_verify.h): the FRI part of whole proofs of the CPU oracle,
sliced out and described as a 4-oracle, 2-batch instance, is accepted; the challenges are the transcript's; after every tamper of
the FRI part the verdict and its text are the whole-proof verifier's on the tampered whole proof, and the Python-integer model's
(tests/fri_verify_model.py). Refusals of _create in qpgpu_fri_prove's words, the EINVALs for the caller's own garbage, sizes.
Exact arithmetic: every comparison is equality. Shapes: the 24-wire synthetic circuit at 2^6 rows, plain and salted."""
import ctypes

import numpy as np
import pytest

import fri_schedules as fs
import fri_verify_model as fm
from oracle_binding import OracleCircuit

P = fs.P
EINVAL, EVERIFY = -1, -6


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "salted"])
def case(request, pkg, orc):
    """A whole proof of the oracle prover, its FRI view, the whole-proof verifier and the FRI verifier of the view's instance."""
    pack, wires, pis = pkg.synth_circuit(6, num_wires=24, num_routed=16, num_public_inputs=3, seed=17)
    if request.param:
        pack = pack.copy(); pack[14] = 1
    oc = OracleCircuit(orc, pack)
    proof = oc.prove(wires, pis, seed=991) if request.param else oc.prove(wires, pis)
    pi_hash = oc.trace("pi_hash").copy()
    indices = [int(x) for x in oc.trace("query_indices")]
    oc.close()
    ver = pkg.Verifier(pack)
    cap = np.zeros(4 << int(pack[11]), dtype=np.uint64)
    assert ver.lib.qpgpu_verifier_constants_sigmas_cap(ver.h, cap.ctypes.data, cap.size) == 0
    view = fm.plonk_view(pkg, pack, proof, pi_hash, cap)
    h, lay = view["header"], view["lay"]
    kw = dict(rate_bits=h["rate_bits"], cap_height=h["cap_height"], proof_of_work_bits=h["proof_of_work_bits"], num_query_rounds=h["num_query_rounds"])
    fv = pkg.FriVerifier(h["degree_bits"], view["oracles"], view["batches"], lay.arity_bits, **kw)
    inst = fm.Instance(h["degree_bits"], h["rate_bits"], h["cap_height"], lay.arity_bits, h["num_query_rounds"], view["oracles"], view["batches"],
                       pow_bits=h["proof_of_work_bits"])
    yield dict(pkg=pkg, pack=pack, proof=proof, view=view, ver=ver, fv=fv, inst=inst, indices=indices, kw=kw)
    fv.close(); ver.close()


def fri_verdict(c, fri):
    """(code, reason) of the FRI-level check of `fri` with the challenges re-derived from it, as a whole-proof verifier does."""
    v, fv = c["view"], c["fv"]
    alpha, betas, powr, idx = fv.challenges(fs.copy_challenger(c["pkg"], v["challenger"]), fri)
    fv.verify(v["caps"], v["points"], v["openings"], alpha, betas, powr, idx, fri)
    return fv.code, fv.reason, (alpha, betas, powr, idx)


def test_sizes(case):
    fv, v = case["fv"], case["view"]
    assert fv.proof_size() == len(v["fri"]) == v["lay"].total == case["inst"].lay.total
    assert fv.num_openings() == len(v["openings"]) == case["inst"].num_openings
    assert fv.lib.qpgpu_fri_verifier_proof_size(None) == 0 and fv.lib.qpgpu_fri_verifier_num_openings(None) == 0


def test_challenges_reproduce_the_transcript(case):
    pkg, v, fv = case["pkg"], case["view"], case["fv"]
    a, b = fs.copy_challenger(pkg, v["challenger"]), fs.copy_challenger(pkg, v["challenger"])
    want_alpha = tuple(fs.copy_challenger(pkg, v["challenger"]).get_n(2))
    want_betas, want_idx = fs.replay_transcript(a, v["fri"], v["lay"])
    alpha, betas, powr, idx = fv.challenges(b, v["fri"])
    assert alpha == want_alpha and betas == want_betas and idx == want_idx == case["indices"]
    assert bytes(a.state) == bytes(b.state)                       # advanced in place, to where the prover's transcript ends
    bits = case["kw"]["proof_of_work_bits"]
    assert bits > 0 and powr >> (64 - bits) == 0
    # a proof of another length, a full input buffer: refused, the state untouched
    before = bytes(b.state)
    with pytest.raises(pkg.QpGpuError) as e:
        fv.challenges(b, v["fri"][:-1])
    assert e.value.code == EINVAL and "bytes" in str(e.value) and bytes(b.state) == before
    full = fs.copy_challenger(pkg, b); full.state.input_len = 8
    with pytest.raises(pkg.QpGpuError) as e:
        fv.challenges(full, v["fri"])
    assert e.value.code == EINVAL and "challenger state" in str(e.value)


def test_accepts_and_the_model_accepts(case, orc):
    v, fv = case["view"], case["fv"]
    code, reason, (alpha, betas, powr, idx) = fri_verdict(case, v["fri"])
    assert (code, reason) == (0, "")
    assert fm.verify(orc, case["inst"], v["caps"], v["points"], v["openings"], alpha, betas, powr, idx, v["fri"]) is None


def tampers(inst, queries, indices):
    """(name, byte offset, bit) in every region of the FRI part at `queries`, the caps, the final polynomial and the nonce; both
    a path length one bit off and one out of range."""
    out = []
    for name, pos, n in inst.regions():
        if name.startswith("q") and int(name[1:name.index(".")]) not in queries:
            continue
        out.append((name, pos, 0))
        if n > 8:
            out.append((name + ".last", pos + n - 8, 1))
        if name.endswith("plen"):
            out.append((name + ".far", pos, 7))
        if name.startswith("q") and name.split(".")[1][0] == "r" and name.endswith("row"):             # the evaluation the previous round continues into
            q, r = int(name[1:name.index(".")]), int(name.split(".")[1][1:])
            within = (indices[q] >> sum(inst.arity_bits[:r])) & ((1 << inst.arity_bits[r]) - 1)
            out.append((name + ".within", pos + 16 * within, 0))
    return out


def test_tampers_give_the_whole_proof_verdict_and_text(case, orc):
    v, ver, inst, proof = case["view"], case["ver"], case["inst"], case["proof"]
    nq = inst.num_queries
    cases = tampers(inst, {0, nq // 2, nq - 1}, case["indices"])
    assert len(cases) > 100
    seen = set()
    for k, (name, pos, bit) in enumerate(cases):
        fri = bytearray(v["fri"]); fri[pos] ^= 1 << bit
        whole = bytearray(proof); whole[v["base"] + pos] ^= 1 << bit
        assert not fm.noncanonical(inst, bytes(fri)), name       # one low bit: the word stays a field element
        assert not ver.verify(bytes(whole)), name
        code, reason, ch = fri_verdict(case, bytes(fri))
        assert code == EVERIFY and reason == ver.reason, (name, reason, ver.reason)
        if k % 7 == 0 or "plen" in name:                         # the model on a part of them (it is slow), every kind among them
            assert fm.reason_of(fm.verify(orc, inst, v["caps"], v["points"], v["openings"], *ch, bytes(fri))) == reason, name
        seen.add(fm.verdict_of(reason)[0])
    assert seen >= {"oracle_plen", "oracle_path", "round_plen", "round_cont", "round_path", "pow"}, seen


def test_final_polynomial_and_noncanonical_and_length(case, orc):
    """With the challenges held fixed (a caller that derived them elsewhere) a changed final coefficient reaches the final
    check; a non-canonical word anywhere is named before anything else; so is another length."""
    v, fv, inst = case["view"], case["fv"], case["inst"]
    _, _, ch = fri_verdict(case, v["fri"])
    lay = inst.lay
    fri = bytearray(v["fri"]); fri[lay.final_pos] ^= 1
    assert not fv.verify(v["caps"], v["points"], v["openings"], *ch, bytes(fri))
    assert fv.code == EVERIFY and fv.reason == "query 0: the final polynomial does not match the last FRI round"
    assert fm.verify(orc, inst, v["caps"], v["points"], v["openings"], *ch, bytes(fri)) == ("final", 0, None)
    for name, pos, n in [r for r in inst.regions() if r[2] >= 8][::37]:
        fri = bytearray(v["fri"]); fri[pos:pos + 8] = (P + 1).to_bytes(8, "little")
        assert not fv.verify(v["caps"], v["points"], v["openings"], *ch, bytes(fri))
        assert (fv.code, fv.reason) == (EVERIFY, "proof holds a non-canonical field element"), name
    assert not fv.verify(v["caps"], v["points"], v["openings"], *ch, v["fri"] + b"\0")
    assert fv.code == EVERIFY and fv.reason == "FRI proof has %d bytes, this instance's proofs have %d" % (lay.total + 1, lay.total)
    # the nonce is bound through the challenges only: with them fixed a changed nonce is accepted, re-derived it is not
    fri = bytearray(v["fri"]); fri[lay.pow_pos] ^= 1
    assert fv.verify(v["caps"], v["points"], v["openings"], *ch, bytes(fri))
    assert fri_verdict(case, bytes(fri))[0] == EVERIFY


def test_the_callers_own_garbage_is_einval(case):
    v, fv = case["view"], case["fv"]
    _, _, (alpha, betas, powr, idx) = fri_verdict(case, v["fri"])
    good = dict(caps=v["caps"], points=v["points"], openings=v["openings"], alpha=alpha, betas=betas, pow_response=powr, indices=idx, proof=v["fri"])

    def refused(part, **change):
        assert not fv.verify(**dict(good, **change))
        assert fv.code == EINVAL and part in fv.reason, (part, fv.code, fv.reason)

    caps = [c.copy() for c in v["caps"]]; caps[2][1, 3] = P
    refused("cap of oracle 2", caps=caps)
    refused("point of batch 1", points=[v["points"][0], (5, P)])
    ops = v["openings"].copy(); ops[7, 1] = 2**64 - 1
    refused("opening 7", openings=ops)
    refused("alpha", alpha=(P, 0))
    if betas:
        refused("beta 0", betas=[(1, P + 1)] + betas[1:])
    refused("proof-of-work response", pow_response=P)
    lde = 1 << (case["inst"].degree_bits + case["inst"].rate_bits)
    refused("indices[3] = %d" % lde, indices=idx[:3] + [lde] + idx[4:])
    # garbage of the caller's comes before any verdict on the proof
    refused("alpha", alpha=(P, 0), proof=v["fri"] + b"\0")
    err = ctypes.create_string_buffer(200)
    assert fv.lib.qpgpu_fri_verify(fv.h, None, None, None, None, None, 0, None, None, 0, err) == EINVAL and b"null argument" in err.value
    assert fv.verify(**good) and fv.reason == ""


# what qpgpu_fri_prove refuses (csrc/fri_api.cpp, fri_prover.cpp, oracle_api.cpp), in its words behind the verifier's prefix
BAD = "bad oracles or FRI parameters"
REFUSALS = [
    (dict(reduction_arity_bits=[9]), BAD),
    (dict(reduction_arity_bits=[0]), BAD),
    (dict(reduction_arity_bits=[4, 4]), BAD),                         # more than degree_bits 6
    (dict(reduction_arity_bits=[3, 3], cap_height=4), BAD),           # the last tree is smaller than the cap
    (dict(proof_of_work_bits=41), BAD),
    (dict(num_query_rounds=0), BAD),
    (dict(num_query_rounds=4097), BAD),
    (dict(oracles=[]), BAD),
    (dict(oracles=[(3, False)] * 256), "more than 255 oracles"),      # a verdict names its oracle in eight bits
    (dict(degree_bits=21, reduction_arity_bits=[4]), "LDE sizes up to 2^23 supported"),
    (dict(batches=[[]]), "a batch needs 1..8 polynomial ranges"),
    (dict(batches=[[(0, 0, 1)] * 9]), "a batch needs 1..8 polynomial ranges"),
    (dict(batches=[[(1, 0, 1)]]), "polynomial range outside its oracle"),
    (dict(batches=[[(0, 2, 2)]]), "polynomial range outside its oracle"),
    (dict(batches=[[(0, 0, 0)]]), "polynomial range outside its oracle"),
    (dict(hasher=7), "unknown hasher kind"),
    (dict(hasher=1, params=np.zeros(5, dtype=np.uint64)), "bad Poseidon2 parameter block"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_create_refuses_what_fri_prove_refuses(pkg, change, message):
    good = dict(degree_bits=6, oracles=[(3, False)], batches=[[(0, 0, 3)]], reduction_arity_bits=[2], rate_bits=3, cap_height=2,
                proof_of_work_bits=4, num_query_rounds=3)
    with pkg.FriVerifier(**good) as fv:
        assert fv.proof_size() == fs.FriLayout(6, 3, 2, [2], 3, [3]).total and fv.num_openings() == 3
    with pytest.raises(pkg.QpGpuError) as e:
        pkg.FriVerifier(**dict(good, **change))
    prefixed = message if "hasher" in message or "Poseidon2" in message else "fri_verifier_create: " + message
    assert e.value.code == EINVAL and str(e.value) == "qpgpu error -1: " + prefixed


def test_create_copies_the_instance_and_takes_nulls(pkg):
    lib = pkg.load_library()
    err = ctypes.create_string_buffer(200); h = ctypes.c_void_p(1)
    assert lib.qpgpu_fri_verifier_create(None, 0, None, 0, ctypes.byref(h), err) == EINVAL and b"null argument" in err.value
    lib.qpgpu_fri_verifier_free(None)
    # 16 rounds of one bit, blinded and plain oracles, a split range: sizes against the layout restated in Python
    fv = pkg.FriVerifier(16, [(5, False), (8, True)], [[(0, 0, 2), (1, 1, 7), (0, 2, 3)]], [1] * 16, rate_bits=1, cap_height=0, num_query_rounds=2)
    assert fv.proof_size() == fs.FriLayout(16, 1, 0, [1] * 16, 2, [5, 12]).total and fv.num_openings() == 12
    fv.close()


def test_host_check_under_the_sanitizers(tmp_path):
    """tools/host_checks/fri_verify_check.cpp: the host verifier on proofs no prover made (random canonical words, every
    path-length byte wrong in turn), built from the library's host-only sources with AddressSanitizer and UBSan: a read outside
    the proof, the caps or the caller's arrays aborts the program."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "fri_verify_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc,
                           os.path.join(root, "tools", "host_checks", "fri_verify_check.cpp")] +
                          [os.path.join(csrc, f) for f in ("fri_verify.cpp", "verifier.cpp", "circuit.cpp", "poseidon_constants.cpp")] + ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "6 instances" in r.stdout and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
