"""qpgpu_stage_plan_create without a device: the words are parsed and checked before the context and the oracle are looked at, so
every refusal of the header reads the same on a CPU-only machine. Both forms of the words (the full pack; the pack with its
constants/sigmas value block left out) are walked by length; a NULL context, a NULL plan pointer and truncated words fail
cleanly; the binding declares the five entries."""
import ctypes

import numpy as np
import pytest

HDR = 18      # magic + 17 header words


def create(pkg, words, n_words=None, out=True):
    lib = pkg.load_library()
    w = None if words is None else np.ascontiguousarray(words, dtype=np.uint64)
    plan = ctypes.c_void_p(0x1234)
    err = ctypes.create_string_buffer(pkg.binding.STAGE_ERR_CAP)
    rc = lib.qpgpu_stage_plan_create(None, None if w is None else w.ctypes.data, (0 if w is None else w.size) if n_words is None else n_words,
                                     None, ctypes.byref(plan) if out else None, err)
    if out:
        assert plan.value is None          # *out is NULL on every error
    return rc, err.value.decode()


@pytest.fixture(scope="module")
def packs(pkg):
    plain = pkg.synth_circuit(6, seed=63, num_wires=24, num_routed=16, num_public_inputs=3)[0]
    p2 = pkg.synth_circuit(7, seed=21, poseidon=True, base_sum=True, poseidon2=True)[0]
    hints = pkg.synth_circuit(7, seed=22, hints=True)[0]
    return plain, p2, hints


def test_binding_declares_the_stage_entries(pkg):
    lib = pkg.load_library()
    for name, nargs in (("qpgpu_stage_plan_create", 6), ("qpgpu_stage_plan_free", 1), ("qpgpu_stage_plan_info", 6),
                        ("qpgpu_stage_partial_products", 6), ("qpgpu_stage_quotient", 8)):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert name in pkg.binding.exported_symbols()
    assert callable(pkg.StagePlan) and callable(pkg.stage_header_words)
    lib.qpgpu_stage_plan_free(None)
    assert lib.qpgpu_stage_plan_info(None, None, None, None, None, None) == -1
    assert lib.qpgpu_stage_partial_products(None, None, 0, None, None, None) == -1
    assert lib.qpgpu_stage_quotient(None, None, None, None, None, None, None, None) == -1


def test_good_words_of_both_forms_reach_the_context_check(pkg, packs):
    """A header that passes is refused only for the missing context: the parse took the form the length says."""
    for pack in packs:
        short = pkg.stage_header_words(pack)
        h = pkg.pack_header(pack)
        ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
        assert short.size == pack.size - (ncs << h["degree_bits"])
        for words in (pack, short):
            assert create(pkg, words) == (-1, "stage_plan_create: null context")
    # the trailers are optional in the short form except where a gate needs one: the hint / PUBI1 trailers may simply be dropped
    plain, _, hints = packs
    for pack in (plain, hints):
        h = pkg.pack_header(pack)
        end = HDR + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
        assert create(pkg, pack[:end]) == (-1, "stage_plan_create: null context")


def test_null_pointers(pkg, packs):
    plain = packs[0]
    assert create(pkg, plain, out=False) == (-1, "stage_plan_create: null plan pointer")
    assert create(pkg, None) == (-1, "stage_plan_create: null words")
    lib = pkg.load_library()
    plan = ctypes.c_void_p()
    assert lib.qpgpu_stage_plan_create(None, plain.ctypes.data, plain.size, None, ctypes.byref(plan), None) == -1     # no err buffer either


def test_truncated_and_misfit_words(pkg, packs):
    plain, p2, _ = packs
    h = pkg.pack_header(plain)
    end = HDR + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    for n_words, why in ((0, "bad magic or truncated header"), (17, "bad magic or truncated header"),
                         (HDR + h["num_arity_rounds"] + 3, "truncated gate list"), (end - 1, "truncated k_is")):
        assert create(pkg, plain, n_words=n_words) == (-1, "stage_plan_create: " + why)
    # past the header, a length that is neither form
    for n_words in (end + 1, end + 7, plain.size - 1, plain.size - 64):
        rc, msg = create(pkg, plain, n_words=n_words)
        assert rc == -1 and "length fits neither" in msg, (n_words, msg)
    bad = plain.copy(); bad[0] ^= 1
    assert create(pkg, bad) == (-1, "stage_plan_create: bad magic or truncated header")


def test_header_rules_are_the_loaders(pkg, packs):
    """CircuitPack::validate() on either form: a type-14 gate without its layout trailer, a header field out of range, and a limit
    of the kernels (more than 16 chunks)."""
    plain, p2, _ = packs
    assert int(p2[-12]) == 0x000000314C473250 and int(p2[-11]) == 10
    why = "stage_plan_create: Poseidon2 gate (type 14) without a wire-layout trailer (P2GL1): the layout is not assumed"
    assert create(pkg, p2[:-12]) == (-1, why)
    assert create(pkg, pkg.stage_header_words(p2)[:-12]) == (-1, why)
    for words in (plain, pkg.stage_header_words(plain)):
        bad = words.copy(); bad[7] = 3                                 # quotient_degree_factor: not a power of two
        assert create(pkg, bad) == (-1, "stage_plan_create: quotient_degree_factor must be a power of two")
        bad = words.copy(); bad[10] = 9                                # rate_bits
        assert create(pkg, bad) == (-1, "stage_plan_create: header field out of range: rate_bits")
        bad = words.copy(); bad[7] = 1; bad[8] = 15                    # 16 routed wires in chunks of one: consistent, and within the limit
        assert create(pkg, bad) == (-1, "stage_plan_create: null context")


def test_stage_example_compiles_against_the_header(tmp_path):
    """examples/stage_prove_example.c uses only include/qpgpu.h; it must compile and link with plain gcc."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "qpgpu_stage_prove_example")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "stage_prove_example.c"),
                           "-L", os.path.join(root, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(root, "qp-zk-circuits_amd"), "-o", out])
    assert os.path.exists(out)
