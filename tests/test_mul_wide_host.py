"""The word-level schedule of the device form of gl::mul64wide (csrc/gl64.hpp: one 64-bit low product, both cross terms through one
64-bit addend, the 65th bit from the multiply-add's carry-out) and the lazy product built on it, restated in plain uint32_t /
uint64_t C++ with every no-overflow claim as an assertion, held against unsigned __int128 on the vectors of
tests/field_vectors_wide.py plus 10^7 random pairs, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/host_checks/mul_wide_check.cpp. No GPU; a few seconds. The device code itself is tested by
tests/test_mul_wide_gpu.py."""
import os
import subprocess

import numpy as np

import field_vectors_wide as fw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_level_schedule_equals_the_128_bit_product_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mul_wide_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "host_checks", "mul_wide_check.cpp"), "-o", exe])
    vec = str(tmp_path / "pairs.bin")
    np.array(fw.pairs(), dtype="<u8").tofile(vec)
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "mul wide: failures 0" in r.stdout and "runtime error" not in r.stderr
    assert "halves: 2401 pairs compared" in r.stdout and "boundaries: 10 pairs compared, 6 carry" in r.stdout
    assert "file: %d pairs compared" % len(fw.pairs()) in r.stdout and "random: 10000000 pairs compared" in r.stdout
