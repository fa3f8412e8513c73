"""The host side of the device ZK tree (csrc/zk_tree.hpp: level sizes and offsets up to 2^24 leaves, the depth bounds, the range and
index checks behind qpgpu_zk_tree_read_level / qpgpu_zk_tree_open) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/host_checks/zk_tree_plan_check.cpp. No GPU; a second or two. The kernels and the exports are tested
on the device by tests/test_zk_tree_gpu.py; what needs no device of the exports (every refusal of a NULL handle) is here too."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_geometry_and_argument_checks_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "zk_tree_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "zk_tree_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "zk tree plan: failures 0" in r.stdout and "runtime error" not in r.stderr


def test_tree_exports_refuse_null_handles_and_contexts(pkg):
    lib = pkg.load_library()
    out = ctypes.create_string_buffer(32)
    h = ctypes.c_void_p(0x1234)
    err = ctypes.create_string_buffer(160)
    assert lib.qpgpu_zk_tree_build(None, out, 1, 0, 0, ctypes.byref(h), err) == -1 and h.value is None and b"null context" in err.value
    assert lib.qpgpu_zk_leaf_hash_batch(None, out, 1, out) == -1
    assert lib.qpgpu_zk_tree_depth(None) == 0 and lib.qpgpu_zk_tree_leaf_count(None) == 0
    assert lib.qpgpu_zk_tree_root(None, out) == -1 and lib.qpgpu_zk_tree_read_level(None, 0, 0, 1, out) == -1
    assert lib.qpgpu_zk_tree_open(None, out, 1, out, out) == -1
    lib.qpgpu_zk_tree_free(None)
    L = pkg.leaf
    assert L.ZK_LEAF_DTYPE.itemsize == 48 and L.ZK_LEAF_DTYPE.fields["transfer_count"][1] == 32 and L.ZK_LEAF_DTYPE.fields["input_amount"][1] == 44
