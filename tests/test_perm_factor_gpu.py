"""The permutation factors of the quotient stage's one-pass kernel (csrc/quotient_kernels.hip: quotient_perm_gates_kernel forms
beta_k k_r x + (v + gamma_k) and beta_k sigma + (v + gamma_k) with v + gamma_k once and ONE reduction per factor, gl::mul_add)
against the two kernels it stands in for (quotient_perm_kernel + quotient_gates_kernel, which keep the reduced forms) and against
the CPU oracle. Synthetic circuits at degree_bits 8 (2^11 LDE points), two challenges: 80 routed wires (ten whole chunks of
eight) and 60 (a ragged last chunk of four, the wire-by-wire path), a single proof and a lockstep batch of three. The witnesses
carry 0, 1 and p - 1 on routed wires: in every NoopGate row (unconstrained, not copy-connected) each routed wire holds one of the
three, so each of them meets every k_r, and sigma sends them through the denominator's factors as well. Held equal, byte for
byte: the proofs of the same witnesses with the switch off and on (qpgpu_circuit_set_quotient_fused), the oracle's proofs, and
the quotient oracle's cap inside the proof against the cap of the oracle's `quotient_chunk_coeffs` trace committed through the
staged API, which pins the quotient coefficients themselves. Exact arithmetic: no tolerance anywhere. The host side of
gl::mul_add is tests/test_mul_add_host.py."""
import numpy as np
import pytest

from oracle_binding import OracleCircuit
from test_quotient_fold_gpu import prove_batch, quotient_cap_of_trace
from test_quotient_fused_gpu import off_and_on
from test_staged_gpu import parse_pack

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
D = 8
EDGE = np.array([0, 1, P - 1], dtype=np.uint64)


def edge_witnesses(pkg, num_routed, nb):
    """(pack, nb witnesses, public inputs): the synthetic circuit's satisfied witness with 0, 1, p - 1 written over the routed
    wires of its NoopGate rows (the last n / 16 rows), another rotation of the three per proof."""
    pack, wires, pis = pkg.synth_circuit(D, num_routed=num_routed, seed=50 + num_routed, base_sum=True)
    n = 1 << D
    noop = np.arange(n - n // 16, n)
    ws = []
    for b in range(nb):
        w = wires.copy()
        r, c = np.meshgrid(np.arange(num_routed), noop, indexing="ij")
        w[:num_routed, n - n // 16:] = EDGE[(r + c + b) % 3]
        ws.append(w)
    return pack, ws, [pis] * nb


@pytest.mark.parametrize("num_routed", [80, 60])
@pytest.mark.parametrize("nb", [1, 3])
def test_one_pass_kernel_equals_two_kernels_and_oracle(pkg, gpu, orc, num_routed, nb):
    pack, ws, ps = edge_witnesses(pkg, num_routed, nb)
    h = parse_pack(pack)
    assert h["degree_bits"] == D and h["rate_bits"] == 3 and h["num_challenges"] == 2
    for w in ws:
        for v in EDGE:
            assert (w[:num_routed] == v).sum() >= num_routed
    circ = pkg.Circuit(gpu, pack, max_batch=nb); oc = OracleCircuit(orc, pack)
    try:
        (off, on), sel = off_and_on(circ, lambda: prove_batch(gpu, circ, ws, ps))
        assert sel == [(False, False), (True, True)]
        cap_bytes = (1 << h["cap_height"]) * 32
        for b in range(nb):
            want = oc.prove(ws[b], ps[b])                     # fills the stage trace for this witness
            assert oc.verify(want) == 0                       # the edited witness still satisfies the circuit
            qcap = quotient_cap_of_trace(pkg, gpu, oc, h)
            assert on[b][2 * cap_bytes:3 * cap_bytes] == off[b][2 * cap_bytes:3 * cap_bytes] == qcap, (num_routed, b)
            assert on[b] == off[b] == want, (num_routed, b)
        assert len(set(on)) == nb
    finally:
        circ.close(); oc.close()
