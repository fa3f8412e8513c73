"""Host build (g++) of gl::mul_add (gl64.hpp: a b + c mod p, the 64-bit addend taken into the 128-bit product before its one
reduction) against unsigned __int128 arithmetic: a, b in {0, 1, 2^32 - 1, 2^32, p - 1} (and p, 2^64 - 1) x c in {0, 2^32 - 1,
2^64 - 1, ...}, 10^6 random triples, and the device form's 32-bit word schedule with its no-wrap claims checked step by step.
tools/host_checks/mul_add_check.cpp; seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mul_add_on_the_host(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "host_checks", "mul_add_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches 0") == 3, r.stdout
