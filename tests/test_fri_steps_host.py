"""The FRI opening proof one step at a time (include/qpgpu.h: qpgpu_fri_session, qpgpu_fri_grind, qpgpu_oracle_open), the part that
needs no device: the call-order state machine of csrc/fri_steps.hpp as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tools/host_checks/fri_steps_check.cpp), every new export's refusal of NULL handles and pointers, and
the Python surface. The steps themselves are tested on the device by tests/test_fri_steps_gpu.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_order_state_machine_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "fri_steps_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "fri_steps_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fri steps: failures 0" in r.stdout and "runtime error" not in r.stderr


def test_new_exports_refuse_null_handles_and_pointers(pkg):
    lib = pkg.load_library()
    fill = bytes([0xA5]) * 256
    buf = ctypes.create_string_buffer(fill, 256)
    buf2 = ctypes.create_string_buffer(fill, 256)
    idx = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    two = (ctypes.c_uint64 * 2)(5, 6)
    n_out = ctypes.c_size_t(77)
    nonce = ctypes.c_uint64(77)
    session = ctypes.c_void_p(0x1234)          # never dereferenced: qpgpu_fri_begin refuses the NULL context first
    ch = pkg.Challenger()
    ch.observe([1, 2, 3])
    before = bytes(ch.state)
    a, a2 = ctypes.addressof(buf), ctypes.addressof(buf2)
    # a NULL handle with every other argument valid, and with every pointer NULL
    assert lib.qpgpu_oracle_open(None, idx, 4, a, a2) == -1 and lib.qpgpu_oracle_open(None, None, 0, None, None) == -1
    assert lib.qpgpu_oracle_leaf_width(None) == 0
    assert lib.qpgpu_fri_begin(None, None, 0, None, 0, None, two, ctypes.byref(session)) == -1 and session.value == 0x1234
    assert lib.qpgpu_fri_begin(None, None, 0, None, 0, None, None, None) == -1
    assert lib.qpgpu_fri_round_commit(None, a, 64) == -1 and lib.qpgpu_fri_round_commit(None, None, 0) == -1
    assert lib.qpgpu_fri_round_fold(None, two) == -1 and lib.qpgpu_fri_round_fold(None, None) == -1
    assert lib.qpgpu_fri_final_poly(None, a, 32, ctypes.byref(n_out)) == -1 and lib.qpgpu_fri_final_poly(None, None, 0, None) == -1
    assert lib.qpgpu_fri_query_size(None) == 0
    assert lib.qpgpu_fri_open(None, idx, 4, a, 256, ctypes.byref(n_out)) == -1 and lib.qpgpu_fri_open(None, None, 0, None, 0, None) == -1
    lib.qpgpu_fri_session_free(None)
    assert lib.qpgpu_fri_grind(None, ctypes.byref(ch.state), 4, ctypes.byref(nonce)) == -1
    assert lib.qpgpu_fri_grind(None, None, 0, None) == -1
    assert buf.raw == fill and buf2.raw == fill and list(idx) == [0, 1, 2, 3] and list(two) == [5, 6]
    assert n_out.value == 77 and nonce.value == 77 and bytes(ch.state) == before


def test_python_surface(pkg):
    for name in ("round_commit", "round_fold", "final_poly", "open", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.FriSession, name))
    assert callable(pkg.PolyOracle.open) and isinstance(pkg.PolyOracle.leaf_width, property)
    assert callable(pkg.fri_grind)
    names = pkg.binding.exported_symbols()
    for n in ("qpgpu_oracle_open", "qpgpu_oracle_leaf_width", "qpgpu_fri_begin", "qpgpu_fri_round_commit", "qpgpu_fri_round_fold",
              "qpgpu_fri_final_poly", "qpgpu_fri_query_size", "qpgpu_fri_open", "qpgpu_fri_session_free", "qpgpu_fri_grind"):
        assert n in names, n
