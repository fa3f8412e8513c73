"""The workgroup placement of the quotient stage's one-pass kernel on the host (csrc/quotient_map.hpp, the code the kernel compiles):
tools/host_checks/quotient_map_check.cpp walks id -> (tile, proof) for batches 1..33 and 1..40 tiles as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer: a bijection onto the launch's (tile, proof) pairs, the ids of a tile equal modulo 8.
No GPU; a few seconds. The kernel is tested on the device by tests/test_quotient_fused_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workgroup_map_is_a_bijection_and_keeps_a_tile_on_one_xcd(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "quotient_map_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "quotient_map_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "quotient map: launches 2640, failures 0" in r.stdout and "runtime error" not in r.stderr
