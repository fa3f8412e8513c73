"""The column-resident coset LDE (csrc/ntt_lde_column.hip: 2^11..2^13 coefficients, rate_bits 1..3, leaf order, one launch)
against the CPU oracle word for word; the QPGPU_NTT_LDE_COLUMN=0 fallback in a fresh child process; shapes that stay on the
generic passes; and a lockstep batch, whose FRI opening-polynomial LDE runs through the kernel with one workspace per proof
(proof strides that are not the column sizes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import OracleCircuit
from test_ntt_gpu import MULT_GEN, P, bitrev_perm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_lde(orc, coeffs, log_n, rate_bits, shift=MULT_GEN):
    """coset_fft of the zero-padded columns, natural order; inputs are reduced first (the oracle takes canonical words)."""
    red = np.where(coeffs >= np.uint64(P), coeffs - np.uint64(P), coeffs)
    pad = np.zeros((coeffs.shape[0], 1 << (log_n + rate_bits)), dtype=np.uint64)
    pad[:, : 1 << log_n] = red
    return np.stack([np.asarray(orc.coset_fft(np.ascontiguousarray(c), log_n + rate_bits, shift), dtype=np.uint64) for c in pad])


def gpu_lde(gpu, coeffs, log_n, rate_bits, bitrev=True, shift=MULT_GEN):
    d_c = gpu.to_device(coeffs)
    d_o = gpu.alloc(coeffs.nbytes << rate_bits)
    gpu.lde_dev(d_c, d_o, log_n, rate_bits, coeffs.shape[0], coset_shift=shift, bitrev=bitrev)
    gpu.sync()
    out = d_o.download().reshape(coeffs.shape[0], -1)
    d_c.free(); d_o.free()
    return out


def edge_columns(log_n, batch, seed):
    """Random columns with the edge inputs in front: all zero, all p - 1, all 2^64 - 1 and p + i (non-canonical words)."""
    n = 1 << log_n
    a = np.random.default_rng(seed).integers(0, P, (batch, n), dtype=np.uint64)
    edges = [np.zeros(n, dtype=np.uint64), np.full(n, P - 1, dtype=np.uint64), np.full(n, 2**64 - 1, dtype=np.uint64),
             np.arange(n, dtype=np.uint64) + np.uint64(P)]
    for i, e in enumerate(edges[: max(0, batch - 1)]):     # a single column stays random
        a[i] = e
    return a


@pytest.mark.parametrize("rate_bits", [1, 2, 3])
@pytest.mark.parametrize("log_n", [11, 12, 13])
@pytest.mark.parametrize("batch", [1, 20, 135])
def test_lde_words_equal_the_oracle(gpu, orc, log_n, rate_bits, batch):
    a = edge_columns(log_n, batch, 500 + 10 * log_n + rate_bits)
    want = oracle_lde(orc, a, log_n, rate_bits)
    got = gpu_lde(gpu, a, log_n, rate_bits)
    assert int(got.max()) < P
    assert np.array_equal(got, want[:, bitrev_perm(log_n + rate_bits)])


@pytest.mark.parametrize("log_n", [11, 13])
def test_edge_inputs_alone(gpu, orc, log_n):
    """Every edge input as a whole batch of its own (five columns: the plain workgroup order, not a multiple of eight)."""
    n = 1 << log_n
    for name, col in (("zero", np.zeros(n, dtype=np.uint64)), ("p_minus_1", np.full(n, P - 1, dtype=np.uint64)),
                      ("all_ones", np.full(n, 2**64 - 1, dtype=np.uint64)), ("p_plus_i", np.arange(n, dtype=np.uint64) + np.uint64(P))):
        a = np.tile(col, (5, 1))
        got = gpu_lde(gpu, a, log_n, 3)
        assert np.array_equal(got, oracle_lde(orc, a, log_n, 3)[:, bitrev_perm(log_n + 3)]), name
    assert not gpu_lde(gpu, np.zeros((8, n), dtype=np.uint64), log_n, 3).any()


def test_other_coset_shift(gpu, orc):
    """The FRI layers use powers of the generator as shifts: the scale table is per shift."""
    shift = orc.pow(MULT_GEN, 16)
    a = edge_columns(12, 8, 77)
    assert np.array_equal(gpu_lde(gpu, a, 12, 3, shift=shift), oracle_lde(orc, a, 12, 3, shift)[:, bitrev_perm(15)])
    assert np.array_equal(gpu_lde(gpu, a, 12, 3), oracle_lde(orc, a, 12, 3)[:, bitrev_perm(15)])


@pytest.mark.parametrize("log_n,rate_bits,bitrev", [(14, 3, True), (13, 3, False), (12, 2, False), (10, 3, True), (13, 4, True)])
def test_shapes_outside_the_kernel_are_unchanged(gpu, orc, log_n, rate_bits, bitrev):
    """d = 14, d = 10, rate_bits = 4 and natural order stay on the generic passes and still equal the oracle."""
    a = edge_columns(log_n, 9, 600 + log_n)
    want = oracle_lde(orc, a, log_n, rate_bits)
    if bitrev:
        want = want[:, bitrev_perm(log_n + rate_bits)]
    assert np.array_equal(gpu_lde(gpu, a, log_n, rate_bits, bitrev=bitrev), want)


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as g
pkg = g.load_package()
a = np.load(sys.argv[2])
log_n, rate_bits = int(sys.argv[4]), int(sys.argv[5])
with pkg.QpGpu(0) as gpu:
    d_c = gpu.to_device(a)
    d_o = gpu.alloc(a.nbytes << rate_bits)
    gpu.lde_dev(d_c, d_o, log_n, rate_bits, a.shape[0], bitrev=True)
    gpu.sync()
    np.save(sys.argv[3], d_o.download().reshape(a.shape[0], -1))
"""


@pytest.mark.parametrize("log_n,rate_bits", [(13, 3), (11, 1)])
def test_fallback_switch_gives_the_same_words(gpu, orc, tmp_path, log_n, rate_bits):
    """QPGPU_NTT_LDE_COLUMN=0 is read once per process: a fresh child runs the generic passes on the same input."""
    a = edge_columns(log_n, 20, 700 + log_n)
    src, dst = str(tmp_path / "in.npy"), str(tmp_path / "out.npy")
    np.save(src, a)
    env = dict(os.environ, QPGPU_NTT_LDE_COLUMN="0")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst, str(log_n), str(rate_bits)], env=env, check=True, timeout=600)
    generic = np.load(dst)
    got = gpu_lde(gpu, a, log_n, rate_bits)
    assert np.array_equal(got, generic)
    assert np.array_equal(got, oracle_lde(orc, a, log_n, rate_bits)[:, bitrev_perm(log_n + rate_bits)])


def test_lockstep_batch_proofs_equal_the_oracle(pkg, gpu, orc):
    """Three proofs of a 2^11-row circuit in lockstep: the wires / Z / quotient LDEs carry the proofs as extra columns, the
    FRI opening polynomial's LDE carries them as proof strides of a per-proof workspace. Proof bytes against the oracle."""
    pack, wires, pis = pkg.synth_circuit(11, seed=31, poseidon=True)
    circ = pkg.Circuit(gpu, pack, max_batch=3); oc = OracleCircuit(orc, pack)
    try:
        mask = circ.witness_free_mask(*wires.shape)
        ws, ps = [], []
        for b in range(3):
            p_b = (pis + np.uint64(b)) % np.uint64(P)
            part = np.where(mask == 1, wires, 0).astype(np.uint64)
            ws.append(circ.generate_witness(part, p_b)); ps.append(p_b)
        d_w = gpu.to_device(np.stack(ws))
        got = circ.prove_batch_dev([d_w.ptr + b * wires.nbytes for b in range(3)], ps)
        d_w.free()
        for b in range(3):
            assert got[b] == oc.prove(ws[b], ps[b]), b
            assert oc.verify(got[b]) == 0
    finally:
        circ.close(); oc.close()
