"""examples/sharded_stage_prove_example.c: the stage flow from plain C against the headers alone, with all four commitments sharded
over two contexts of device 0 and the plan from qpgpu_stage_plan_create_sharded; it compares its bytes with qpgpu_prove's itself,
verifies them with qpgpu_verifier_verify and shows the refusal of a broken witness. 2^10 rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name):
    out = str(tmp_path / name)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sharded_stage_prove_example.c"),
                           "-L", os.path.join(ROOT, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "qp-zk-circuits_amd"), "-o", out])
    return out


def test_sharded_stage_example_compiles_against_the_headers(tmp_path):
    assert os.path.exists(build(tmp_path, "qpgpu_sharded_stage_prove_example"))


@pytest.mark.gpu
def test_sharded_stage_example_in_c(tmp_path):
    out = build(tmp_path, "qpgpu_sharded_stage_prove_example_gpu")
    res = subprocess.run([out, "10"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    for line in ("qpgpu_stage_plan_create refuses it: stage_plan_create: cs_oracle is sharded over 2 contexts",
                 "plan over 2 shards", "quotient on 2 shards: done", "sharded staged flow == qpgpu_prove:",
                 "qpgpu_verifier_verify: accepted", "refused: witness does not satisfy the circuit: gate constraints fail at row 20",
                 "sharded stage flow: ok"):
        assert line in res.stdout, res.stdout
