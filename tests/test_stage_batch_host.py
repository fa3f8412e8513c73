"""The lockstep-batch entries of the stage-level C ABI (include/qpgpu.h: qpgpu_oracle_commit_batch .. qpgpu_fri_grind_batch), the part
that needs no device: qpgpu_stage_plan_create_batch refuses a max_batch outside 1..1024 together with the header, before the
context and the oracle are looked at; every new export resolves in the built library, has its prototype declared in the binding and
refuses NULL handles and pointers without touching anything. The entries themselves are tested on the device by
tests/test_stage_batch_gpu.py."""
import ctypes

import numpy as np
import pytest

NEW = {
    "qpgpu_oracle_commit_batch": 11, "qpgpu_oracle_batch": 1, "qpgpu_oracle_strides": 4, "qpgpu_oracle_eval_batch": 5,
    "qpgpu_oracle_open_batch": 5, "qpgpu_stage_plan_create_batch": 7, "qpgpu_stage_plan_max_batch": 1,
    "qpgpu_stage_partial_products_batch": 7, "qpgpu_stage_quotient_batch": 9, "qpgpu_fri_prove_batch": 12, "qpgpu_fri_begin_batch": 10,
    "qpgpu_fri_session_batch": 1, "qpgpu_fri_grind_batch": 5,
}


def create(pkg, words, max_batch, n_words=None):
    lib = pkg.load_library()
    w = np.ascontiguousarray(words, dtype=np.uint64)
    plan = ctypes.c_void_p(0x1234)
    err = ctypes.create_string_buffer(pkg.binding.STAGE_ERR_CAP)
    rc = lib.qpgpu_stage_plan_create_batch(None, w.ctypes.data, w.size if n_words is None else n_words, None, max_batch, ctypes.byref(plan), err)
    assert plan.value is None              # *out is NULL on every error
    return rc, err.value.decode()


@pytest.fixture(scope="module")
def pack(pkg):
    return pkg.synth_circuit(6, seed=63, num_wires=24, num_routed=16, num_public_inputs=3)[0]


def test_max_batch_is_checked_with_the_header_before_anything_else(pkg, pack):
    for words in (pack, pkg.stage_header_words(pack)):
        for bad in (0, 1025, 1 << 31):
            rc, msg = create(pkg, words, bad)
            assert rc == -1 and msg == "stage_plan_create: max_batch is %d, it must be 1..1024" % bad
        for good in (1, 3, 1024):
            assert create(pkg, words, good) == (-1, "stage_plan_create: null context")
    # a bad header still gives the loader's message first
    bad = pack.copy(); bad[10] = 9
    assert create(pkg, bad, 0) == (-1, "stage_plan_create: header field out of range: rate_bits")
    assert create(pkg, pack, 0, n_words=17) == (-1, "stage_plan_create: bad magic or truncated header")
    p2 = pkg.synth_circuit(7, seed=21, poseidon=True, base_sum=True, poseidon2=True)[0]
    rc, msg = create(pkg, p2[:-12], 1025)
    assert rc == -1 and "without a wire-layout trailer" in msg
    lib = pkg.load_library()
    assert lib.qpgpu_stage_plan_create_batch(None, pack.ctypes.data, pack.size, None, 0, None, None) == -1     # no plan pointer, no err buffer


def test_binding_declares_every_new_export(pkg):
    lib = pkg.load_library()
    names = pkg.binding.exported_symbols()
    for name, nargs in NEW.items():
        assert name in names, name + " is not declared in include/qpgpu.h"
        assert hasattr(lib, name), name + " declared but not exported"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    assert callable(pkg.PolyOracle.commit_batch) and callable(pkg.PolyOracle.strides)
    assert callable(pkg.StagePlan.partial_products_batch) and callable(pkg.StagePlan.quotient_batch)
    assert callable(pkg.fri_prove_batch) and callable(pkg.fri_grind_batch)
    import inspect
    assert "batch" in inspect.signature(pkg.FriSession.__init__).parameters
    assert "max_batch" in inspect.signature(pkg.StagePlan.__init__).parameters


def test_new_exports_refuse_null_handles_and_pointers(pkg):
    lib = pkg.load_library()
    fill = bytes([0xA5]) * 256
    buf = ctypes.create_string_buffer(fill, 256)
    buf2 = ctypes.create_string_buffer(fill, 256)
    a, a2 = ctypes.addressof(buf), ctypes.addressof(buf2)
    idx = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    ptrs = (ctypes.c_void_p * 2)(a, a2)
    handle = ctypes.c_void_p(0x1234)           # never dereferenced: the NULL context is refused first
    nonces = (ctypes.c_uint64 * 2)(77, 77)
    lens = (ctypes.c_size_t * 2)(77, 77)
    st = (pkg.binding.ChallengerState * 2)()
    before = bytes(st)
    assert lib.qpgpu_oracle_commit_batch(None, ptrs, 2, 3, 5, 3, 4, 0, 0, 0, ctypes.byref(handle)) == -1 and handle.value == 0x1234
    assert lib.qpgpu_oracle_commit_batch(None, None, 0, 0, 0, 0, 0, 0, 0, 0, None) == -1
    assert lib.qpgpu_oracle_batch(None) == 0
    assert lib.qpgpu_oracle_strides(None, idx, idx, idx) == -1 and lib.qpgpu_oracle_strides(None, None, None, None) == -1
    assert lib.qpgpu_oracle_eval_batch(None, idx, 0, 1, a) == -1 and lib.qpgpu_oracle_eval_batch(None, None, 0, 0, None) == -1
    assert lib.qpgpu_oracle_open_batch(None, idx, 2, a, a2) == -1 and lib.qpgpu_oracle_open_batch(None, None, 0, None, None) == -1
    assert lib.qpgpu_stage_plan_max_batch(None) == 0
    assert lib.qpgpu_stage_partial_products_batch(None, ptrs, 2, 0, idx, idx, a) == -1
    assert lib.qpgpu_stage_partial_products_batch(None, None, 0, 0, None, None, None) == -1
    assert lib.qpgpu_stage_quotient_batch(None, None, None, 2, idx, idx, idx, idx, a) == -1
    assert lib.qpgpu_stage_quotient_batch(None, None, None, 0, None, None, None, None, None) == -1
    assert lib.qpgpu_fri_prove_batch(None, None, 0, None, 0, idx, 2, None, ctypes.byref(st), ptrs, 256, lens) == -1
    assert lib.qpgpu_fri_prove_batch(None, None, 0, None, 0, None, 0, None, None, None, 0, None) == -1
    assert lib.qpgpu_fri_begin_batch(None, None, 0, None, 0, idx, 2, None, idx, ctypes.byref(handle)) == -1 and handle.value == 0x1234
    assert lib.qpgpu_fri_begin_batch(None, None, 0, None, 0, None, 0, None, None, None) == -1
    assert lib.qpgpu_fri_session_batch(None) == 0
    assert lib.qpgpu_fri_grind_batch(None, ctypes.byref(st), 2, 4, nonces) == -1 and lib.qpgpu_fri_grind_batch(None, None, 0, 0, None) == -1
    assert buf.raw == fill and buf2.raw == fill and list(idx) == [0, 1, 2, 3]
    assert list(nonces) == [77, 77] and list(lens) == [77, 77] and bytes(st) == before
