"""Host build (g++) of two pieces the matrix-pipe hashing kernels share with the host through GL_HD headers: the S-box input of a
partial round from the gemm's limbs and the running group's UNREDUCED terms with one reduction (pmf::recombine_wide,
pmf::reduce96_terms), and the MDS layer limited to the rows a caller reads (poseidon::mds_layer_rows), both against 128-bit
integer arithmetic mod p. tools/host_checks/partial_terms_check.cpp; seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_terms_and_row_limited_layer_on_the_host(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "host_checks", "partial_terms_check.cpp"),
                           os.path.join(csrc, "poseidon_constants.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches 0") == 2, r.stdout
