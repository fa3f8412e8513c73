"""The device form of the 64 x 64 -> 128 product (gl::mul64wide: both cross terms through one 64-bit addend, the 65th bit taken from
the multiply-add's own carry-out) through everything that is built on it, on the vectors of tests/field_vectors_wide.py: all
combinations of extreme 32-bit halves, the boundaries of the cross-term sum (2^64 - 2 .. 2^64 + 1, a = b = 2^64 - 1, operands
swapped), 2^16 random pairs, and pairs built to take mul_lazy's rare borrow on either side of the carry. Every result word is
compared with Python integers modulo p: no tolerance, no case left out. tests/test_mul_wide.py holds the census of the vectors."""
import pytest

import field_vectors_wide as fw

pytestmark = pytest.mark.gpu


def run_dev(gpu, case):
    case.check(gpu.field_probe(case.op, case.a, case.b, case.param))


@pytest.mark.parametrize("op", ["mul", "sqr", "e2_mul", "pow"])
def test_scalar_operation(gpu, op):
    cases = [c for c in fw.host_cases() if c.op == op]
    assert len(cases) == 1
    run_dev(gpu, cases[0])


@pytest.mark.parametrize("N", fw.GROUP_SIZES)
def test_mul_group(gpu, N):
    """all pairs, N to a thread; then the carry pairs in one lane of each wave, in all lanes, and next to lanes without a carry
    across a wave boundary"""
    cases = [c for c in fw.host_cases() if c.op == "mul_group" and c.param == N]
    assert len(cases) == 1 + len(fw.GROUP_PATTERNS)
    for c in cases:
        run_dev(gpu, c)


@pytest.mark.parametrize("terms", fw.ACC_TERMS)
def test_accumulator(gpu, terms):
    """acc_mul chains of 1, 3 and 4096 products: the top word stays 0, reaches 1, and runs up to 4095"""
    cases = [c for c in fw.host_cases() if c.op == "acc" and c.param == terms]
    assert len(cases) == 1
    run_dev(gpu, cases[0])


@pytest.mark.parametrize("k", range(1, 7))
def test_dif_regs_on_boundary_operands(gpu, k):
    cases = fw.all_dif_cases()[k]
    assert sorted(c.param >> 8 for c in cases) == [0, 1]
    for c in cases:
        run_dev(gpu, c)
