"""The two batch layers under a caller's CircuitConfig (include/qpgpu_batch.h: qpgpu_wrapper_circuit_build_cfg; the reference's
PrivateBatchCircuit::new(config, ..) / PublicBatchCircuit::new(config, ..)) and the reference's knob policy on the host
(include/qpgpu_wire.h: qpgpu_agg_config_validate / _build; wormhole/memprof/src/config.rs), on the CPU. The inner circuit is the fake
leaf (2^5 rows), the wrappers verify N = 2 proofs completely (transcript, arithmetic half) and carry the layer's logic: the
smallest circuits that hold every gadget of the verifier part. tests/test_wrapper_config_gpu.py proves them on the device."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle_binding as ob
from test_batch_circuits_fake_leaf import EXITS, leaf_pis

T_, PRIVATE, PUBLIC, VERIFY, ZK = 1, 2, 4, 8, 16          # QPGPU_WRAPPER_*
N = 2
PRE = np.arange(4 * N, dtype=np.uint64).reshape(N, 4) + 1
ROWS = [leaf_pis(101, out=(100, 5), exits=(EXITS[0], EXITS[1])), leaf_pis(102, out=(7, 8), exits=(EXITS[0], EXITS[2]))]
NONE = np.zeros(0, dtype=np.uint64)
GRID = [(r, nw) for r in (37, 47, 48, 54) for nw in (135, 143)]


def grid_config(pkg, routed, num_wires):
    return pkg.circuit_config("private_batch", num_routed_wires=routed, num_wires=num_wires, num_challenges=3, cap_height=2, rate_bits=4)


def fake_leaf(pkg):
    """The fake leaf (2^5 rows) with a final polynomial of 2 coefficients, so that its FRI proof has a reduction step at all: one of arity
    16 — the wrapper then holds the CosetInterpolationGate over 16 points whose 37 routed wires are the reference's floor."""
    L = pkg.leaf
    fake = L.LeafCircuit(fragment=L.FRAGMENT_FAKE_LEAF, config=pkg.circuit_config("leaf", reduction_final_poly_bits=1))
    h = pkg.pack_header(fake.pack)
    assert h["degree_bits"] == 5 and [int(a) for a in fake.pack[18:18 + h["num_arity_rounds"]]] == [4]
    return fake


def prove_fake(orc, pack, rows):
    oc = ob.OracleCircuit(orc, pack)
    out = []
    for pis in rows:
        rc, wires, _ = orc.generate_witness(pack, NONE, NONE, pis)
        assert rc == orc.WIT_OK
        out.append(oc.prove(wires, pis))
    oc.close()
    return out


def constants_sigmas_cap(pkg, pack, ver):
    cap = np.empty(4 << int(pack[11]), dtype=np.uint64)
    assert pkg.recursion._lib().qpgpu_verifier_constants_sigmas_cap(ver.h, cap.ctypes.data, cap.size) == 0
    return cap


def raw_build(pkg, inner_pack, cap, routed, flags, cfg="legacy", num_proofs=N):
    """One call of the C entry with room for everything: (rc, err, pack, target map with the blinding cells, info).
    cfg: "legacy" = qpgpu_wrapper_circuit_build; None / a CircuitConfig = qpgpu_wrapper_circuit_build_cfg with that pointer."""
    L = pkg.recursion._lib()
    pack = np.empty(1 << 23, dtype=np.uint64); tmap = np.empty(1 << 22, dtype=np.uint64); info = np.zeros(16, dtype=np.uint64)
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(400)
    head = (inner_pack.ctypes.data, inner_pack.size, cap.ctypes.data, cap.size, num_proofs, routed, 0, 0, flags)
    tail = (pack.ctypes.data, pack.size, ctypes.byref(n), tmap.ctypes.data, tmap.size, ctypes.byref(m), info.ctypes.data, err)
    if isinstance(cfg, str):
        rc = L.qpgpu_wrapper_circuit_build(*head, *tail)
    else:
        rc = L.qpgpu_wrapper_circuit_build_cfg(*head, None if cfg is None else ctypes.byref(cfg), *tail)
    return rc, err.value.decode(), pack[:n.value].copy(), tmap[:m.value].copy(), info


@pytest.fixture(scope="module")
def env(pkg, orc):
    L = pkg.leaf
    fake = fake_leaf(pkg)
    ver = pkg.Verifier(fake.pack)
    proofs = prove_fake(orc, fake.pack, ROWS)
    assert all(ver.verify(p) for p in proofs)
    yield fake, ver, proofs, constants_sigmas_cap(pkg, fake.pack, ver)
    ver.close()


def is_canonical(pkg, pack, level):
    L = pkg.load_library()
    L.qpgpu_pack_config_is_canonical.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p]
    err = ctypes.create_string_buffer(400)
    return L.qpgpu_pack_config_is_canonical(pack.ctypes.data, pack.size, level, err), err.value.decode()


def test_default_config_is_the_existing_entry_word_for_word(pkg, orc, env):
    fake, ver, proofs, cap = env
    # the private layer: (60 routed wires, the zero-knowledge flag) by argument == the level's config
    flags = T_ | VERIFY | PRIVATE
    want = raw_build(pkg, fake.pack, cap, 60, flags | ZK)
    assert want[0] == 0 and want[4][11] > 0                    # blinding rows: the cells follow the query-index block
    for got in (raw_build(pkg, fake.pack, cap, 60, flags | ZK, cfg=None), raw_build(pkg, fake.pack, cap, 0, flags, cfg=pkg.circuit_config("private_batch"))):
        assert got[0] == 0, got[1]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4][:12].tolist() == want[4][:12].tolist()
    assert want[4][12:].tolist() == [0] * 4                     # the existing entry writes its 12 info words, no more
    assert is_canonical(pkg, want[2], 1)[0] == 0
    rc, why = is_canonical(pkg, want[2], 2)
    assert rc != 0 and "num_routed_wires" in why
    # the public layer over a circuit with a private batch's 21 N + 8 public inputs: 80 and 0 by argument == the level's config
    import test_builder_gadgets_gpu as bg
    inner = bg.gadget_circuit(pkg, 3000 + 21 * 2 + 8)[0]
    iver = pkg.Verifier(inner)
    icap = constants_sigmas_cap(pkg, inner, iver)
    iver.close()
    flags = T_ | VERIFY | PUBLIC
    want = raw_build(pkg, inner, icap, 80, flags)
    assert want[0] == 0, want[1]
    for got in (raw_build(pkg, inner, icap, 0, flags), raw_build(pkg, inner, icap, 0, flags, cfg=None), raw_build(pkg, inner, icap, 0, flags, cfg=pkg.circuit_config("public_batch"))):
        assert got[0] == 0, got[1]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4][:12].tolist() == want[4][:12].tolist()
    assert is_canonical(pkg, want[2], 2)[0] == 0 and is_canonical(pkg, want[2], 1)[0] != 0


def test_argument_conflicts_name_the_argument(pkg, env):
    fake, ver, proofs, cap = env
    cfg = pkg.circuit_config("private_batch")
    rc, why = raw_build(pkg, fake.pack, cap, 60, T_ | VERIFY | PRIVATE, cfg=cfg)[:2]
    assert rc == -1 and "num_routed_wires must be 0" in why
    rc, why = raw_build(pkg, fake.pack, cap, 0, T_ | VERIFY | PRIVATE | ZK, cfg=cfg)[:2]
    assert rc == -1 and "QPGPU_WRAPPER_ZERO_KNOWLEDGE must be clear" in why
    with pytest.raises(pkg.QpGpuError) as e:
        pkg.recursion.WrapperCircuit(fake.pack, ver, N, num_routed_wires=60, logic="private_batch", verify=True, config="private_batch")
    assert "num_routed_wires" in str(e.value)


@pytest.mark.parametrize("fields,needle", [
    (dict(security_bits=90), "security_bits (90) is not modelled"),
    (dict(use_base_arithmetic_gate=0), "use_base_arithmetic_gate = false is not modelled"),
    (dict(max_quotient_degree_factor=7), "max_quotient_degree_factor must be 8"),
    (dict(num_wires=134), "circuit config num_wires (134) must be >= 135 (Poseidon gate floor)"),
    (dict(num_routed_wires=36), "circuit config num_routed_wires (36) must be >= 37 (recursion gate floor"),
    (dict(rate_bits=2), "circuit config fri_config.rate_bits (2) must be >= ceil(log2(max_quotient_degree_factor = 8)) = 3"),
    (dict(num_constants=3), "num_constants must be 2"),
    (dict(reduction_arity_bits=5), "arity_bits (5) must be 1..4"),
    (dict(reduction_final_poly_bits=9), "final_poly_bits (9) must be <= 8"),
    (dict(proof_of_work_bits=33), "proof_of_work_bits (33) must be <= 32"),
])
def test_builder_refusals_name_the_field(pkg, env, fields, needle):
    fake, ver, proofs, cap = env
    rc, why = raw_build(pkg, fake.pack, cap, 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch", **fields))[:2]
    assert rc == -1 and needle in why, why
    # the leaf entry refuses the same config with the same words behind its own name (one shared policy)
    with pytest.raises(pkg.QpGpuError) as e:
        pkg.leaf.LeafCircuit(fragment=pkg.leaf.FRAGMENT_FAKE_LEAF, config=pkg.circuit_config("private_batch", **fields))
    assert str(e.value) == "qpgpu error -1: " + why.replace("wrapper_circuit_build", "leaf_circuit_build")


def test_inner_cap_that_leaves_random_access_no_copy(pkg, env):
    """RandomAccessGate::new_from_config has num_routed_wires / (2 + 2^bits) copies: an inner cap of height 6 needs 66 routed wires."""
    L = pkg.leaf
    fake6 = L.LeafCircuit(fragment=L.FRAGMENT_FAKE_LEAF, config=pkg.circuit_config("leaf", cap_height=6))
    v6 = pkg.Verifier(fake6.pack)
    cap6 = constants_sigmas_cap(pkg, fake6.pack, v6)
    rc, why = raw_build(pkg, fake6.pack, cap6, 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch"))[:2]
    assert rc == -1 and "cap_height 6" in why and "66" in why and "60" in why and "logic_error" not in why
    # with room for one copy the gate is one the proof system does not carry (RandomAccessGates of up to 2^5 entries): refused by name too
    rc, why = raw_build(pkg, fake6.pack, cap6, 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch", num_routed_wires=66))[:2]
    assert rc == -1 and "cap_height 6" in why and "up to 2^5 entries" in why
    v6.close()
    # cap height 5 (34 routed wires per copy) is the largest inner cap: one copy at 60 routed wires
    fake5 = L.LeafCircuit(fragment=L.FRAGMENT_FAKE_LEAF, config=pkg.circuit_config("leaf", cap_height=5))
    v5 = pkg.Verifier(fake5.pack)
    rc, why, pack = raw_build(pkg, fake5.pack, constants_sigmas_cap(pkg, fake5.pack, v5), 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch"))[:3]
    v5.close()
    assert rc == 0, why
    at = 18 + int(pack[17])
    assert (10, 5, 1) in [tuple(int(x) for x in pack[at + 8 * g:at + 8 * g + 3]) for g in range(int(pack[16]))]      # RandomAccessGate { bits: 5, num_copies: 1 }


@pytest.fixture(scope="module")
def grid(pkg, orc, env):
    """Every wrapper of the grid, built once: (WrapperCircuit, the oracle's witness, the public inputs read from the trace)."""
    fake, ver, proofs, cap = env
    out = {}
    for routed, nw in GRID:
        w = pkg.recursion.WrapperCircuit(fake.pack, ver, N, logic="private_batch", verify=True, config=grid_config(pkg, routed, nw))
        cells, vals, _ = w.commit(proofs, preimages=PRE, public_inputs=np.zeros(21 * N + 8, dtype=np.uint64), blinding_seed=bytes([routed] * 32))
        rc, wires, _ = orc.generate_witness(w.pack, cells, vals, None)            # not handed public inputs: the generators produce them
        pic = pkg.pack_public_input_cells(w.pack)
        out[routed, nw] = (w, rc, wires, wires[(pic % nw).astype(np.int64), (pic // nw).astype(np.int64)])
    return out


@pytest.mark.parametrize("routed,num_wires", GRID)
def test_builder_grid(pkg, orc, grid, routed, num_wires):
    w, rc, wires, pis = grid[routed, num_wires]
    h = pkg.pack_header(w.pack)
    assert (h["num_wires"], h["num_routed_wires"], h["num_challenges"], h["cap_height"], h["rate_bits"], h["num_query_rounds"], h["zero_knowledge"]) == (num_wires, routed, 3, 2, 4, 28, 1)
    assert w.num_wires == num_wires and w.info["rows_blinding"] > 0
    L = pkg.load_library()
    L.qpgpu_pack_validate.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    err = ctypes.create_string_buffer(200)
    assert L.qpgpu_pack_validate(w.pack.ctypes.data, w.pack.size, err) == 0, err.value
    rc_c, why = is_canonical(pkg, w.pack, 1)
    assert rc_c != 0 and ("num_wires" in why if num_wires != 135 else "num_routed_wires" in why)     # the first field that differs, by name
    assert rc == orc.WIT_OK
    assert pis.tolist() == pkg.aggregation.private_batch_outputs(np.stack(ROWS), PRE).tolist()
    # PoseidonMdsGate needs 24 D = 48 routed wires; below, the MDS layer of the inner PoseidonGate at zeta is arithmetic
    assert (w.info["rows_poseidon_mds"] == 0) == (routed < 48)
    assert w.info["rows_coset_interpolation"] > 0 and w.info["rows_reducing"] > 0 and w.info["rows_random_access"] > 0
    # the gates' sizes by upstream's new_from_config rules
    at = 18 + h["num_arity_rounds"]
    gates = {int(w.pack[at + 8 * g]): tuple(int(x) for x in w.pack[at + 8 * g + 1:at + 8 * g + 3]) for g in range(h["num_gates"]) if int(w.pack[at + 8 * g]) in (3, 6, 8, 9, 13)}
    assert gates[3][0] == routed // 4 and gates[6][0] == routed // 8 and gates[13] == (4, 6)        # ArithmeticGate, ArithmeticExtensionGate, CosetInterpolationGate::with_max_degree(4, 8): 2 intermediates, degree 6
    assert gates[8][0] == min((num_wires - 4) // 3, routed - 6) and gates[9][0] == min((num_wires - 4) // 4, (routed - 6) // 2)


def test_oracle_proves_the_narrowest_wrapper(pkg, orc, grid):
    w, rc, wires, pis = grid[37, 135]
    oc = ob.OracleCircuit(orc, w.pack)
    proof = oc.prove(wires, pis, seed=3)
    assert oc.verify(proof) == 0
    oc.close()
    v = pkg.Verifier(w.pack)
    assert v.verify(proof), v.reason
    bad = bytearray(proof); bad[len(bad) // 3] ^= 1
    assert not v.verify(bytes(bad))
    v.close()


def test_other_knobs_build(pkg, env):
    """num_challenges 1..4, the wrapper's own cap_height 0..8, num_query_rounds free."""
    fake, ver, proofs, cap = env
    for fields in (dict(num_challenges=1, cap_height=0, num_query_rounds=5), dict(num_challenges=4, cap_height=8, num_query_rounds=84, rate_bits=8)):
        rc, why, pack = raw_build(pkg, fake.pack, cap, 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch", **fields))[:3]
        assert rc == 0, why
        h = pkg.pack_header(pack)
        assert all(h[k] == v for k, v in fields.items())
    rc, why = raw_build(pkg, fake.pack, cap, 0, T_ | VERIFY | PRIVATE, cfg=pkg.circuit_config("private_batch", num_challenges=5))[:2]
    assert rc == -1 and "num_challenges" in why


# ---- the knob policy: the scenarios of wormhole/memprof/src/config.rs's own tests, message for message ----

def validate(pkg, allow=False, **knobs):
    return pkg.agg_config_validate(pkg.agg_config_args(allow_weakening_security=allow, **knobs))


def test_knob_policy_scenarios(pkg):
    base = pkg.circuit_config("private_batch")
    # num_wires_below_poseidon_floor_is_rejected
    assert validate(pkg, num_wires=1) == "--num-wires must be >= 135 (Poseidon gate floor), got 1"
    assert ">= 135" in validate(pkg, num_wires=134)
    # quotient_degree_below_poseidon_constraint_degree_is_rejected
    assert validate(pkg, max_quotient_degree_factor=6) == "--max-quotient-degree-factor must be >= 7 (Poseidon constraint degree), got 6"
    # routed_wires_below_recursion_gate_floor_are_rejected
    for routed in (1, 2, 3, 4, 17, 36):
        assert validate(pkg, num_routed_wires=routed) == ("--num-routed-wires must be >= 37 (recursion gate floor: the FRI coset-interpolation gate routes 37 wires, "
                                                           "and narrower widths leave slot-packed gates with zero operation slots), got %d" % routed)
    assert validate(pkg, num_routed_wires=37) is None
    # routed_wires_exceeding_num_wires_is_rejected: against the override, and against the baseline
    assert validate(pkg, num_wires=135, num_routed_wires=136) == "--num-routed-wires (136) must be <= num_wires (135); routed wires are a subset of the wire columns"
    assert "must be <= num_wires (%d)" % base.num_wires in validate(pkg, num_routed_wires=base.num_wires + 1)
    # production_and_swept_values_are_accepted
    assert validate(pkg) is None
    assert validate(pkg, num_wires=135, num_routed_wires=54, max_quotient_degree_factor=7) is None
    # zero_knobs_are_still_rejected
    assert validate(pkg, rate_bits=0) == "--rate-bits must be greater than 0"
    for knob in pkg.AggConfigArgs.KNOBS:
        assert validate(pkg, allow=True, **{knob: 0}) == "--%s must be greater than 0" % knob.replace("_", "-")
    # oversized_fri_exponents_are_rejected / fri_exponent_ceilings_are_accepted
    for bits in (9, 20, 63, 2 ** 64 - 1):
        assert validate(pkg, rate_bits=bits) == ("--rate-bits must be <= 8 (LDE memory doubles per bit: lde_size = 2^(degree_bits + rate_bits) per committed polynomial), got %d" % bits)
        assert validate(pkg, cap_height=bits) == "--cap-height must be <= 8 (Merkle caps and recursive verifier-data allocations scale as 2^cap_height), got %d" % bits
    assert validate(pkg, rate_bits=8) is None and validate(pkg, cap_height=8) is None
    # rate_bits_below_quotient_degree_are_rejected
    for bits in (1, 2):
        assert validate(pkg, rate_bits=bits) == ("--rate-bits (%d) must be >= ceil(log2(max_quotient_degree_factor = 8)) = 3; plonky2's prover cannot compute quotient chunks of "
                                                 "degree higher than the FRI rate and asserts this only at proving time, after the full circuit build" % bits)
    assert "ceil(log2(max_quotient_degree_factor = 7)) = 3" in validate(pkg, rate_bits=2, max_quotient_degree_factor=7)
    assert validate(pkg, rate_bits=3) is None
    # the gate of the four security-affecting knobs
    assert validate(pkg, zk_mode="rowblinding") is None
    assert validate(pkg, zk_mode="disabled", num_query_rounds=20, security_bits=90, num_challenges=1) == (
        "the following flags can weaken security: --zk-mode disabled, --num-query-rounds, --security-bits, --num-challenges\npass --allow-weakening-security to acknowledge and proceed")
    assert validate(pkg, num_challenges=3) == "the following flags can weaken security: --num-challenges\npass --allow-weakening-security to acknowledge and proceed"
    assert validate(pkg, allow=True, zk_mode="disabled", num_query_rounds=20, security_bits=90, num_challenges=1) is None


def test_knob_policy_build(pkg):
    base = pkg.circuit_config("private_batch").as_dict()
    assert pkg.agg_config_build(pkg.agg_config_args()).as_dict() == base
    # rate_bits re-balances the query rounds: ceil(3 * 28 / v)
    assert [pkg.agg_config_build(pkg.agg_config_args(rate_bits=v)).num_query_rounds for v in range(3, 9)] == [28, 21, 17, 14, 12, 11]
    c = pkg.agg_config_build(pkg.agg_config_args(rate_bits=4, num_query_rounds=9, allow_weakening_security=True))
    assert (c.rate_bits, c.num_query_rounds) == (4, 9)              # an explicit num_query_rounds wins
    c = pkg.agg_config_build(pkg.agg_config_args(zk_mode="disabled", cap_height=2, num_wires=143, num_routed_wires=54, max_quotient_degree_factor=7, security_bits=90, num_challenges=3))
    assert c.as_dict() == dict(base, zero_knowledge=0, cap_height=2, num_wires=143, num_routed_wires=54, max_quotient_degree_factor=7, security_bits=90, num_challenges=3)
    assert pkg.agg_config_build(pkg.agg_config_args(zk_mode="rowblinding")).zero_knowledge == 1


def sweep_rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "memprof_sweep_grid.json")) as f:
        return json.load(f)["rows"]


def test_sweep_fixture(pkg):
    """Every recorded row parses; each yields a config the reference's validate_circuit_config accepts or is one of the three kinds
    this backend names as unrunnable (tools/agg_config_sweep.py prints those with the refusal's text)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("agg_config_sweep", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "agg_config_sweep.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = sweep_rows()
    assert len(rows) == 32 and {r["sweep"] for r in rows} >= {"baseline", "zk_mode", "num_routed_wires", "num_wires", "max_qdf", "rayon_threads", "combo_per_N"}
    kinds = {}
    for r in rows:
        plan = tool.plan_row(pkg, r)
        if plan["refusal"] is not None:
            kinds.setdefault(plan["kind"], []).append(r["label"])
            continue
        assert pkg.validate_circuit_config(plan["config"]) is None, r
        assert plan["num_leaf_proofs"] in (1, 2, 4, 8, 16)
    assert sorted(kinds) == ["max_quotient_degree_factor", "polyfri", "rayon_threads"]
    assert kinds["max_quotient_degree_factor"] == ["7"] and len(kinds["rayon_threads"]) == 4 and kinds["polyfri"] == ["polyfri (default)"]
    best = tool.plan_row(pkg, next(r for r in rows if r["label"] == "best_safe_combo"))
    assert (best["config"].num_routed_wires, best["config"].zero_knowledge, best["num_leaf_proofs"]) == (54, 1, 16)
