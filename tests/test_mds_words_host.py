"""Host build (g++) of two pieces the matrix-pipe hashing kernels share with the host through GL_HD headers: the MDS layer on whole
words (poseidon::mds_layer_rows_words: one wrapping 64-bit transform, one 32-bit transform of the top 23 bits) for the whole layer
and the row sets <0,4>, <8,4>, <7,1>, <0,12> against mds_layer_naive and 128-bit integers, and the same layer with the constants of
the following round folded in (poseidon::mds_layer_words_rc) against the reference layer and a modular addition.
tools/host_checks/mds_words_check.cpp; seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_form_layer_on_the_host(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", csrc, os.path.join(ROOT, "tools", "host_checks", "mds_words_check.cpp"),
                           os.path.join(csrc, "poseidon_constants.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("mismatches 0") == 2, r.stdout
