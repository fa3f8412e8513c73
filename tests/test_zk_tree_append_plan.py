"""The host side of the append-only device ZK tree (csrc/zk_tree.hpp: the reserved plan, the dirty range of an append, the checks behind
qpgpu_zk_tree_append and qpgpu_zk_tree_open_at) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tools/host_checks/zk_tree_append_check.cpp. No GPU; a few seconds. The kernels and the exports are tested on the device by
tests/test_zk_tree_append_gpu.py; what needs no device of the new exports (every refusal of a NULL handle) is here too."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reserved_plan_dirty_ranges_and_snapshot_checks_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "zk_tree_append_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "zk_tree_append_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "zk tree append: failures 0" in r.stdout and "runtime error" not in r.stderr


def test_append_exports_refuse_null_handles_and_contexts(pkg):
    lib = pkg.load_library()
    L = pkg.leaf
    out = ctypes.create_string_buffer(64)
    h = ctypes.c_void_p(0x1234)
    err = ctypes.create_string_buffer(160)
    assert lib.qpgpu_zk_tree_build_reserved(None, out, 1, 4, 0, 0, ctypes.byref(h), err) == -1 and h.value is None and b"null context" in err.value
    snap = L.ZkSnapshot()
    assert ctypes.sizeof(snap) == 528 and L.ZkSnapshot.last.offset == 16
    assert lib.qpgpu_zk_tree_capacity(None) == 0
    assert lib.qpgpu_zk_tree_append(None, out, 1, 0, ctypes.addressof(snap), err) == -1 and b"null tree" in err.value
    assert lib.qpgpu_zk_tree_append(None, out, 1, 0, None, None) == -1
    assert lib.qpgpu_zk_tree_snapshot(None, ctypes.addressof(snap)) == -1
    assert lib.qpgpu_zk_tree_open_at(None, ctypes.addressof(snap), out, 1, out, out) == -1
    assert bytes(snap) == bytes(528)
