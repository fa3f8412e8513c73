"""The vectors of tests/field_vectors_wide.py themselves (no GPU): the census of the cross-term carry of the 64 x 64 -> 128 product
(gl::mul64wide's device form: M = a1 b0 + (a0 b1 + hi32(a0 b0)) with the carry-out cM of that multiply-add), and the same vectors
through the host versions of the field primitives. tests/test_mul_wide_gpu.py runs them on the device.

Every class of (cM in {0, 1}) x (high word of M in {0, 0xFFFFFFFF, other}) x (mul_lazy's rare borrow taken / not taken) that
exists keeps at least one pair. Two of the twelve do not exist, and the test says why: the cross-term sum is at most
2^65 - 3 2^32, so with cM = 1 the high word of M is at most 0xFFFFFFFD. Everything is computed from the operand values alone."""
import collections

import pytest

import field_vectors as fv
import field_vectors_wide as fw


def test_pair_sets():
    assert len(fw.half_pairs()) == 2401 == len(set(fw.half_pairs()))
    for s, a, b in fw.BOUNDARY:
        assert fw.cross_sum(a, b) == s == fw.cross_sum(b, a)
    assert [s - fv.T64 for s, _, _ in fw.BOUNDARY] == [-2, -1, 0, 1]
    bp = fw.boundary_pairs()
    assert (fv.M64, fv.M64) in bp and all((b, a) in bp for a, b in bp) and len(bp) == 10
    assert len(fw.random_pairs()) == 1 << 16 and fw.random_pairs() == fw.random_pairs()          # seeded
    assert len(fw.pairs()) == 2401 + 10 + (1 << 16) + 4 * len(fw.RARE_SUMS)
    for (a, b), s in zip(fw.rare_pairs(), [s for s in fw.RARE_SUMS for _ in range(4)]):
        assert fw.cross_sum(a, b) == s and fv.is_rare_pair(a, b)


def test_census_of_the_cross_term_carry():
    cen = collections.Counter(fw.classes())
    for cl in fw.REQUIRED_CLASSES:
        assert cen[cl] >= 1, (cl, dict(cen))
    # the two classes that cannot exist: the largest cross-term sum, at a = b = 2^64 - 1, has M's high word at 0xFFFFFFFD
    assert fw.cross_sum(fv.M64, fv.M64) == fw.S_MAX == (1 << 65) - 3 * fv.W
    assert (fw.S_MAX - fv.T64) >> 32 == 0xFFFFFFFD
    assert set(fw.REQUIRED_CLASSES) | set(fw.UNREACHABLE_CLASSES) == set(fw.ALL_CLASSES) and len(fw.ALL_CLASSES) == 12
    assert not any(cen[cl] for cl in fw.UNREACHABLE_CLASSES)


def test_share_of_random_pairs_that_carry():
    """7.25 % of full-range random pairs set cM; a generator that has lost the carry path leaves the 5 % .. 10 % band"""
    share = sum(1 for a, b in fw.random_pairs() if fw.cross_sum(a, b) >= fv.T64) / fw.N_RANDOM
    assert 0.05 < share < 0.10, share


def test_group_patterns_place_the_carry_pairs():
    for N in fw.GROUP_SIZES:
        for pat in fw.GROUP_PATTERNS:
            case, mask = fw.group_pattern_case(N, pat)
            n = fw.GROUP_THREADS
            got = [[fw.cross_sum(int(case.a[i * N + k]), int(case.b[i * N + k])) >= fv.T64 for k in range(N)] for i in range(n)]
            assert got == mask
            lanes = [any(r) for r in mask]
            if pat == "all lanes":
                assert all(lanes)
            elif pat == "one lane":
                assert [sum(lanes[w:w + 64]) for w in range(0, n, 64)] == [1, 1, 1]
            else:
                assert lanes[63] and not lanes[64] and not lanes[127] and lanes[128] and lanes[n - 1] and n > 128


def test_accumulator_rows_reach_the_top_word():
    assert fw.ACC_TERMS == (1, 3, 4096)
    by_terms = {c.param: c for c in fw.host_cases() if c.op == "acc"}
    assert set(by_terms[4096].labels) >= {"top = 0", "top >= 2"} and "top = 1" in by_terms[3].labels
    assert fv.acc_class([fv.M64] * 4096, [fv.M64] * 4096) == "top >= 2" and (4096 * fv.M64 * fv.M64) >> 128 == 4095


def test_host_case_names():
    assert tuple(c.name for c in fw.host_cases()) == fw.HOST_CASE_NAMES


@pytest.mark.parametrize("name", fw.HOST_CASE_NAMES)
def test_host_path(pkg, name):
    case = [c for c in fw.host_cases() if c.name == name]
    assert len(case) == 1
    case[0].check(pkg.field_probe_host(case[0].op, case[0].a, case[0].b, case[0].param))
