"""Host build (g++) of the limb join of the matrix-pipe permutation (pmf::recombine_wide: eight accumulator limbs up to
16 711 935 at 8-bit spacing, joined as four 32-bit shift-adds, two multiply-adds by 2^16 and one carry): the join against the
128-bit integer sum on the 5^8 grid of edge limbs and 10^6 random vectors, the worst-case limb of all three tables derived from
the table bytes, and the upload-time self-checks with the integer emulation of the device schedule against poseidon::permute.
tools/host_checks/recombine_check.cpp; seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_limb_join_and_limb_bound_on_the_host(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "host_checks", "recombine_check.cpp"),
                           os.path.join(csrc, "poseidon_constants.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches 0") == 3, r.stdout
