"""The matrix-pipe hashing build with carry-free digits (poseidon_mfma.hpp: to_digits is one XOR, the digits sum to v - DIGIT_BIAS and
the tables' additive constants carry the bias) against the latency build and the host hash, byte for byte, at the smallest shapes:
trees of 2^10 leaves at widths 9, 17 and 135 (a ragged block behind a full one, both endings of a multi-block sponge, the wires
shape), one tree and three in lockstep. The columns mix the byte edges of the digit conversion (0, 1, 0x7F..7F, 0x80..80,
0x80..80 - 1, p - 1, and p and 2^64 - 1 reduced) with random elements, whole leaves of edge values included. Trees this small
take the latency kernels by default and the routing is read once per process, so two child processes (mx_digits_child.py) build
the same trees, as tests/test_mx_small_trees_gpu.py does: one with every hashing launch forced onto the matrix build, one with
the matrix build off. Each child also proves one 2^8-row circuit: the proof holds the nonce its proof-of-work launch found, and
both must be the CPU oracle's bytes. The host side of the digits is tests/test_mx_digits_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_digits_child as child
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "mx_digits_child.py")
NEVER = str(1 << 62)
ROUTING = {
    "matrix": {"QPGPU_TPUT_BATCH": "1", "QPGPU_MX": "1"},
    "latency": {"QPGPU_TPUT_BATCH": "4000000000", "QPGPU_MX": "0", "QPGPU_TP_MIN_THREADS": NEVER, "QPGPU_COOP_MAX": "0", "QPGPU_TREE_TOP": "0"},
}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = {}
    for name, env in ROUTING.items():
        path = str(tmp_path_factory.mktemp("mx_digits") / (name + ".npz"))
        base = {k: v for k, v in os.environ.items() if not k.startswith("QPGPU_")}
        r = subprocess.run([sys.executable, CHILD, path], env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        with np.load(path) as z:
            out[name] = {k: z[k] for k in z.files}
    assert set(out["matrix"]) == set(out["latency"])
    return out


def test_columns_hold_the_byte_edges():
    a = child.leaves_of(9)
    for v in child.EDGES:
        assert (a == np.uint64(v)).sum() > 100
    by = a.view(np.uint8)
    for b in (0x00, 0x7F, 0x80, 0xFF):
        assert (by == b).any()
    assert (a < np.uint64(child.P)).all()


@pytest.mark.parametrize("width", child.WIDTHS)
def test_one_tree_equals_latency_build_and_host_hash(built, orc, width):
    got, want = built["matrix"], built["latency"]
    dig_host, cap_host = orc.merkle(child.leaves_of(width)[0], child.CAP_HEIGHT)
    for k, host in (("b1_w%d_digests" % width, dig_host), ("b1_w%d_cap" % width, cap_host)):
        assert got[k].shape == want[k].shape == host.shape and got[k].size > 0
        assert got[k].tobytes() == want[k].tobytes() == host.tobytes(), k


@pytest.mark.parametrize("width", child.WIDTHS)
def test_three_trees_in_lockstep_equal_latency_build(built, width):
    keys = sorted(k for k in built["matrix"] if k.startswith("b3_w%d_" % width))
    assert len(keys) == 3
    for k in keys:
        got, want = built["matrix"][k], built["latency"][k]
        assert got.shape == want.shape and got.size > 0
        assert got.tobytes() == want.tobytes(), k


def test_proof_with_its_nonce_equals_the_oracle(built, pkg, orc):
    pack, wires, pis = pkg.synth_circuit(8, **child.PROOF_CIRCUIT)
    oc = OracleCircuit(orc, pack)
    try:
        want = oc.prove(wires, pis)
        assert built["matrix"]["proof"].tobytes() == built["latency"]["proof"].tobytes() == want
        assert oc.verify(want) == 0
    finally:
        oc.close()
