"""The host side of the device ZK tree at earlier counts and through reorgs (csrc/zk_tree.hpp: last_node, the checks behind
qpgpu_zk_tree_snapshots_at, _open_at_counts and _truncate) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/host_checks/zk_tree_reorg_check.cpp. No GPU; a few seconds. The kernels and the exports are tested
on the device by tests/test_zk_tree_reorg_gpu.py; what needs no device of the new exports (every refusal of a NULL handle, whatever
the other arguments) is here too."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_node_derivation_and_reorg_checks_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "zk_tree_reorg_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "zk_tree_reorg_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "zk tree reorg: failures 0" in r.stdout and "runtime error" not in r.stderr


def test_reorg_exports_refuse_null_handles_and_pointers(pkg):
    lib = pkg.load_library()
    L = pkg.leaf
    fill = bytes([0xA5]) * 528
    snaps = ctypes.create_string_buffer(fill, 528)
    out = ctypes.create_string_buffer(fill, 528)
    counts = (ctypes.c_uint64 * 2)(1, 1)
    idx = (ctypes.c_uint64 * 2)(0, 0)
    err = ctypes.create_string_buffer(160)
    snap = L.ZkSnapshot()
    snap.count, snap.depth = 1, 1
    # a NULL tree, with every other argument valid and with every pointer NULL
    assert lib.qpgpu_zk_tree_snapshots_at(None, counts, 1, snaps) == -1
    assert lib.qpgpu_zk_tree_snapshots_at(None, None, 1, None) == -1 and lib.qpgpu_zk_tree_snapshots_at(None, None, 0, None) == -1
    assert lib.qpgpu_zk_tree_snapshot_check(None, ctypes.addressof(snap)) == -1 and lib.qpgpu_zk_tree_snapshot_check(None, None) == -1
    assert lib.qpgpu_zk_tree_open_at_counts(None, counts, idx, 2, out, out, out) == -1
    assert lib.qpgpu_zk_tree_open_at_counts(None, None, None, 2, None, None, None) == -1
    assert lib.qpgpu_zk_tree_open_at_counts(None, None, None, 0, None, None, None) == -1
    assert lib.qpgpu_zk_tree_truncate(None, 1, snaps, err) == -1 and b"null tree" in err.value
    assert lib.qpgpu_zk_tree_truncate(None, 1, None, None) == -1 and lib.qpgpu_zk_tree_truncate(None, 0, None, None) == -1
    assert snaps.raw == fill and out.raw == fill and list(counts) == [1, 1] and list(idx) == [0, 0]
    assert (snap.count, snap.depth) == (1, 1) and bytes(snap)[16:] == bytes(512)
    # the Python surface the device tests go through
    for name in ("snapshots_at", "check", "truncate"):
        assert callable(getattr(L.ZkTree, name))
