"""The folded form of the hash gates' quotient terms on the host (csrc/quotient_fold.hpp: the backward walk over the linear layers, the
folded sum and the forward walk of the round-by-round kernel, the same GL_HD code the kernels compile) against the plain alpha-weighted sum over verify_math.hpp's constraints, as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tools/host_checks/quotient_fold_check.cpp. No GPU; a few
seconds. The kernels are tested on the device by tests/test_quotient_fold_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folded_sum_equals_the_plain_constraint_sum_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "quotient_fold_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "host_checks", "quotient_fold_check.cpp"), os.path.join(csrc, "poseidon_constants.cpp"),
                           "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "quotient fold: failures 0" in r.stdout and r.stdout.count("pairs compared") == 12 and "runtime error" not in r.stderr
