"""Small trees on the matrix-pipe hashing build (merkle_kernels_mx.hip) against the latency build (merkle_hash_impl.hpp), byte for
byte: 2^10 leaves at widths 5, 8, 9, 16, 17 and 135 (one block; a full last block; a ragged last block behind a full one; both
endings of a multi-block sponge; the wires shape), cap heights 0 and 4, one tree and nine trees in lockstep. Trees this small
take the lane-cooperative and the latency kernels by default, and the routing is read once per process, so two child processes
build the same trees: one with every hashing launch forced onto the matrix build (QPGPU_TPUT_BATCH=1: every batch counts as
throughput work, which takes the large-launch builds at every level), one with the matrix build off and every launch on the
thread-per-hash latency build. Compared: the leaf digests, every level and the cap (one tree: the digest array itself; nine trees:
the Merkle paths of all leaves, which hold every digest below the cap, and the caps)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "mx_forced_trees_child.py")
NEVER = str(1 << 62)
ROUTING = {
    "matrix": {"QPGPU_TPUT_BATCH": "1", "QPGPU_MX": "1"},
    "latency": {"QPGPU_TPUT_BATCH": "4000000000", "QPGPU_MX": "0", "QPGPU_TP_MIN_THREADS": NEVER, "QPGPU_COOP_MAX": "0", "QPGPU_TREE_TOP": "0"},
}
WIDTHS = (5, 8, 9, 16, 17, 135)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    out = {}
    for name, env in ROUTING.items():
        path = str(tmp_path_factory.mktemp("mx_small_trees") / (name + ".npz"))
        base = {k: v for k, v in os.environ.items() if not k.startswith("QPGPU_")}
        r = subprocess.run([sys.executable, CHILD, path], env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        with np.load(path) as z:
            out[name] = {k: z[k] for k in z.files}
    assert set(out["matrix"]) == set(out["latency"])
    return out


@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("cap_height", [0, 4])
@pytest.mark.parametrize("width", WIDTHS)
def test_small_tree_matrix_build_equals_latency_build(trees, width, cap_height, batch):
    prefix = "b%d_w%d_c%d_" % (batch, width, cap_height)
    keys = sorted(k for k in trees["matrix"] if k.startswith(prefix))
    assert len(keys) == (2 if batch == 1 else 3)
    for k in keys:
        got, want = trees["matrix"][k], trees["latency"][k]
        assert got.shape == want.shape and got.size > 0
        assert got.tobytes() == want.tobytes(), k
    if batch == 1:
        dig = trees["matrix"][prefix + "digests"]
        assert dig[: 1 << 10].any(axis=1).all(), "every leaf digest was written"
