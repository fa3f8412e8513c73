"""examples/sharded_commit_example.c: a commitment sharded over two contexts of device 0 from plain C, against the headers alone;
it compares its cap and openings with qpgpu_oracle_commit's itself, proves the openings and verifies the proof."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name):
    out = str(tmp_path / name)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sharded_commit_example.c"),
                           "-L", os.path.join(ROOT, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "qp-zk-circuits_amd"), "-o", out])
    return out


def test_sharded_example_compiles_against_the_headers(tmp_path):
    assert os.path.exists(build(tmp_path, "qpgpu_sharded_commit_example"))


@pytest.mark.gpu
def test_sharded_example_in_c(tmp_path):
    out = build(tmp_path, "qpgpu_sharded_commit_example_gpu")
    res = subprocess.run([out, "10"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for line in ("2 shards, cap == qpgpu_oracle_commit's", "shard 1: leaves [4096, 8192)", "openings == qpgpu_oracle_commit's",
                 "qpgpu_fri_verify: accepted", "a flipped proof byte: rejected", "sharded commitment: ok"):
        assert line in res.stdout, res.stdout
