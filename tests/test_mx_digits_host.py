"""Host build (g++) of the carry-free digit conversion of the matrix-pipe permutation (pmf::to_digits: the eight signed digits of v
sum to the integer v - DIGIT_BIAS, the tables' additive constants carry the bias): the digit sums at the byte edges and on 10^5
random words, the three upload-time table self-checks, and the integer emulation of the device schedule against
poseidon::permute on states built from the edge values. tools/host_checks/digits_check.cpp; seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carry_free_digits_on_the_host(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "host_checks", "digits_check.cpp"),
                           os.path.join(csrc, "poseidon_constants.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches 0") == 3, r.stdout
