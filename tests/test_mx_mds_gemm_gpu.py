"""The matrix-pipe hashing build (poseidon_mfma.hpp: the limb join of the gemm outputs, pmf::recombine_wide, in its shift-add and
carry-chain form) against the CPU oracle's host hash, byte for byte, at the smallest shapes that can go wrong: trees of 2^10
leaves with cap height 4 at widths 8 (one block, digest ending), 9 (a ragged block behind a full one), 16 (two full blocks,
capacity-only ending), 17 (both endings) and 135 (the wires shape), and three 2^8-leaf trees in lockstep (768 leaf hashes: a
half-filled workgroup and clamped lanes above). The columns mix the edge values 0, 1, p - 1, 2^64 - 1 (reduced) and the byte edges
of the digit conversion with random elements, whole leaves of edge values included. Trees this small take the latency kernels by
default and the routing is read once per process, so two child processes (mx_mds_gemm_child.py) build the same trees: one with
every hashing launch forced onto the matrix build, one with the matrix build off; each is held against the oracle. Each child
also proves one 2^8-row circuit: the proof holds the nonce its proof-of-work launch found (the row-7 ending), and its bytes
must be the oracle's. The host side of the join is tests/test_mx_recombine_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mx_mds_gemm_child as child
from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "mx_mds_gemm_child.py")
NEVER = str(1 << 62)
ROUTING = {
    "matrix": {"QPGPU_TPUT_BATCH": "1", "QPGPU_MX": "1"},
    "latency": {"QPGPU_TPUT_BATCH": "4000000000", "QPGPU_MX": "0", "QPGPU_TP_MIN_THREADS": NEVER, "QPGPU_COOP_MAX": "0", "QPGPU_TREE_TOP": "0"},
}
BUILDS = tuple(ROUTING)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    out = {}
    for name, env in ROUTING.items():
        path = str(tmp_path_factory.mktemp("mx_mds_gemm") / (name + ".npz"))
        base = {k: v for k, v in os.environ.items() if not k.startswith("QPGPU_")}
        r = subprocess.run([sys.executable, CHILD, path], env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        with np.load(path) as z:
            out[name] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(scope="module")
def host_trees(orc):
    """the oracle's digests and cap of every single tree, computed once"""
    return {w: orc.merkle(child.leaves_of(w), child.CAP_HEIGHT) for w in child.WIDTHS}


def test_columns_hold_the_edge_values():
    a = child.leaves_of(9)
    for v in child.EDGES:
        assert (a == np.uint64(v)).sum() > 100
    for k, v in enumerate(child.EDGES):
        assert (a[1 + k] == np.uint64(v)).all()
    assert (a < np.uint64(child.P)).all()
    assert {0, 1, child.P - 1, (2**64 - 1) % child.P} <= set(child.EDGES)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("width", child.WIDTHS)
def test_one_tree_equals_the_host_hash(built, host_trees, width, build):
    dig_host, cap_host = host_trees[width]
    for k, host in (("w%d_digests" % width, dig_host), ("w%d_cap" % width, cap_host)):
        got = built[build][k]
        assert got.shape == host.shape and got.size > 0
        assert got.tobytes() == host.tobytes(), (build, k)


@pytest.fixture(scope="module")
def host_lockstep(built, orc):
    """per tree, the oracle's digest levels (leaf digests first, the cap last) over the leaf rows the matrix build opened"""
    rows = built["matrix"]["lock_rows"]
    trees = []
    for b in range(child.LOCK_BATCH):
        levels = [np.stack([orc.hash_or_noop(r) for r in rows[b]])]
        while len(levels[-1]) > (1 << child.CAP_HEIGHT):
            d = levels[-1]
            levels.append(np.stack([orc.two_to_one(d[2 * i], d[2 * i + 1]) for i in range(len(d) // 2)]))
        trees.append(levels)
    return trees


@pytest.mark.parametrize("build", BUILDS)
def test_three_trees_in_lockstep_equal_the_host_hash(built, host_lockstep, build):
    got = built[build]
    n, plen = 1 << child.LOCK_LOG_LEAVES, child.LOCK_LOG_LEAVES - child.CAP_HEIGHT
    assert got["lock_rows"].shape == (child.LOCK_BATCH, n, child.LOCK_WIDTH)
    assert got["lock_rows"].tobytes() == built["matrix"]["lock_rows"].tobytes()         # the same leaves under both routings
    assert got["lock_paths"].shape == (child.LOCK_BATCH, n, plen, 4)
    for b, levels in enumerate(host_lockstep):
        assert got["lock_cap"][b].tobytes() == levels[-1].tobytes(), (build, b)
        idx = np.arange(n)
        for lvl in range(plen):
            assert got["lock_paths"][b, :, lvl].tobytes() == levels[lvl][(idx >> lvl) ^ 1].tobytes(), (build, b, lvl)


@pytest.fixture(scope="module")
def host_proof(pkg, orc):
    pack, wires, pis = pkg.synth_circuit(8, **child.PROOF_CIRCUIT)
    oc = OracleCircuit(orc, pack)
    try:
        want = oc.prove(wires, pis)
        assert oc.verify(want) == 0
    finally:
        oc.close()
    return want


@pytest.mark.parametrize("build", BUILDS)
def test_proof_with_its_nonce_equals_the_oracle(built, host_proof, build):
    assert built[build]["proof"].tobytes() == host_proof
