"""The Goldilocks device arithmetic, primitive by primitive, at its rare carry and borrow paths: qpgpu_field_probe runs each
function of gl64.hpp (and the NTT's mul_pow2_dyn, dif_regs and dif_sparse) on the device, one thread per index, on the vectors of
tests/field_vectors.py — the edge set E and its products, operand pairs built to force each class of the branch census, full-range
("loose") random words — and every result word is compared with Python integers modulo p: right iff r % p == want, and < p where
the operation is documented canonical. No tolerance, no case left out.

The register transforms are compared with a direct O(4^K) DFT in the convention read off dif_level: root w = 2^(192 / 2^K), the
inverse direction uses w^-1 and carries no 1/N factor, output slot j holds X[bitrev_K(j)]; dif_sparse computes the same transform
for inputs that are zero from index 2^LV on (tests/test_field_probe.py pins the convention and the vectors without a GPU)."""
import pytest

import field_vectors as fv
from test_field_probe import SCALAR_OPS

pytestmark = pytest.mark.gpu


def run_dev(gpu, case):
    case.check(gpu.field_probe(case.op, case.a, case.b, case.param))


@pytest.mark.parametrize("op", SCALAR_OPS)
def test_scalar_operation(gpu, op):
    cases = [c for c in fv.scalar_cases() if c.op == op]
    assert len(cases) == 1
    run_dev(gpu, cases[0])


@pytest.mark.parametrize("op", ["mul_pow2", "mul_pow2_dyn"])
def test_shifts(gpu, op):
    """every arm of mul_pow2<S>, S in 0..191, and of the NTT's own copy mul_pow2_dyn, s in 0..95 (constant shift, as its call
    sites have it)"""
    cases = [c for c in fv.shift_cases() if c.op == op]
    assert [c.param for c in cases] == list(range(192 if op == "mul_pow2" else 96))
    for c in cases:
        run_dev(gpu, c)


@pytest.mark.parametrize("terms", fv.ACC_TERMS)
def test_accumulator(gpu, terms):
    """acc_zero, `terms` x acc_mul, acc_reduce: final top word 0, 1 and >= 2 (the census of test_field_probe.py)"""
    run_dev(gpu, [c for c in fv.acc_cases() if c.param == terms][0])


@pytest.mark.parametrize("n", fv.GROUP_THREADS)
@pytest.mark.parametrize("N", fv.GROUP_SIZES)
def test_mul_group_wave_patterns(gpu, N, n):
    """mul_group<N>'s one branch per wave: no lane rare, one lane in one element, all, disjoint lanes in different elements, rare
    next to common across a wave boundary and next to the lanes the tail guard retired"""
    cases = [c for c, _ in fv.group_cases() if c.param == N and c.tag.startswith("N%d n%d " % (N, n))]
    assert len(cases) == len(fv.GROUP_PATTERNS)
    for c in cases:
        run_dev(gpu, c)


@pytest.mark.parametrize("k", range(1, 7))
def test_dif_regs(gpu, k):
    cases = [c for c in fv.dif_cases() if c.op == "dif_regs" and (c.param & 0xFF) == k]
    assert sorted(c.param >> 8 for c in cases) == [0, 1]
    for c in cases:
        run_dev(gpu, c)


@pytest.mark.parametrize("inst", fv.DIF_SPARSE_INSTANCES, ids=lambda t: "K%d_INV%d_LV%d" % t)
def test_dif_sparse(gpu, inst):
    k, inv, lv = inst
    cases = [c for c in fv.dif_cases() if c.op == "dif_sparse" and c.param == (k | inv << 8 | lv << 16)]
    assert len(cases) == 1
    run_dev(gpu, cases[0])


def test_device_and_host_paths_agree_mod_p(gpu, pkg):
    """the two texts behind `#if`: same values modulo p on every scalar case (representatives may differ)"""
    for c in fv.scalar_cases():
        d = gpu.field_probe(c.op, c.a, c.b, c.param)
        h = pkg.field_probe_host(c.op, c.a, c.b, c.param)
        assert [int(x) % fv.P for x in d] == [int(x) % fv.P for x in h], c.name


def test_bad_arguments_on_device(gpu, pkg):
    import numpy as np
    with pytest.raises(pkg.QpGpuError):
        gpu.field_probe("dif_regs", np.zeros(128, dtype=np.uint64), param=7)             # K above 6
    with pytest.raises(pkg.QpGpuError):
        gpu.field_probe("mul_pow2", np.zeros(4, dtype=np.uint64), param=192)
    with pytest.raises(pkg.QpGpuError):
        gpu.field_probe("dif_sparse", np.zeros(16, dtype=np.uint64), param=4 | 2 << 16)     # not an instance the kernels use
    with pytest.raises(pkg.QpGpuError):
        gpu.field_probe("dif_sparse", np.zeros(16, dtype=np.uint64), param=4 | 1 << 8 | 1 << 16)
