"""The field probe through the HOST versions of gl64.hpp (qpgpu_field_probe with on_device = 0; no GPU): every operation the host
path has, on the vectors of tests/field_vectors.py, against Python integers modulo p — plus the checks on the vectors
themselves: the branch census (every rare carry / borrow class keeps at least 16 cases), the mul_group wave patterns, and the
DFT convention of the register transforms' reference. tests/test_field_probe_gpu.py runs the same vectors on the device."""
import os
import re

import numpy as np
import pytest

import field_vectors as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR_OPS = ("canon", "neg", "sqr", "mul7", "inv", "mul_eps", "add", "sub", "mul", "reduce128", "reduce96", "add_canonical", "pow",
              "e2_add", "e2_sub", "e2_mul", "e2_scale", "e2_inv", "e2_pow")


def test_operation_numbers_match_the_header(pkg):
    text = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    names = re.findall(r"QPGPU_FP_([A-Z0-9_]+)\b", re.search(r"enum \{\s*QPGPU_FP_CANON = 0(.*?)\};", text, re.S).group(0))
    assert names[-1] == "OP_COUNT"
    assert tuple(n.lower() for n in names[:-1]) == fv.FP_OPS == pkg.FP_OPS
    assert set(SCALAR_OPS) | {"mul_pow2", "mul_pow2_dyn", "mul_group", "acc", "dif_regs", "dif_sparse"} == set(fv.FP_OPS)


def test_edge_set():
    P, W, T = fv.P, fv.W, fv.T64
    need = [0, 1, 2, 7, 2**31, W - 2, W - 1, W, W + 1, 2**33 - 1, 2**63 - 1, 2**63, 2**63 + 1, P - W, P - 2, P - 1, P, P + 1, P + W - 2,
            T - W + 1, T - W + 2, T - W - 1, T - 2, T - 1]
    need += [m * W + lo for m in (1, 2**16, 2**31, W - 2, W - 1) for lo in (0, W - 1)]
    assert set(need) <= set(fv.E) and len(set(fv.E)) == len(fv.E) and 45 <= len(fv.E) <= 60
    assert sum(1 for e in fv.E if e >= P) >= 8            # loose values are the point


def test_branch_census():
    """Every rare class of every operation keeps at least 16 cases; computed from the operand values alone."""
    cen = fv.census(fv.scalar_cases() + fv.acc_cases())
    for op, classes in fv.REQUIRED_CLASSES.items():
        for cl in classes:
            assert cen[op][cl] >= fv.MIN_PER_CLASS, (op, cl, dict(cen[op]))
    # the length-1024 chain: all maximal operands, and (2^64 - 1, 2^64 - 1) repeated reaches top >= 2
    long_chain = [c for c in fv.acc_cases() if c.param == 1024][0]
    assert set(int(x) for x in long_chain.a[:1024]) == {fv.M64} and set(int(x) for x in long_chain.b[:1024]) == {fv.M64}
    assert set(long_chain.labels) == {"top >= 2"} and int(long_chain.a.min()) >= fv.M64 - 3
    assert fv.acc_class([fv.M64] * 3, [fv.M64] * 3) == "top >= 2" and fv.acc_class([fv.M64] * 2, [fv.M64] * 2) == "top = 1"
    assert tuple(c.param for c in fv.acc_cases()) == (1, 2, 3, 257, 1024) and max(len(c.labels) for c in fv.acc_cases()) <= 256


def test_mul_group_wave_patterns():
    """The rare products sit where the pattern says (and nowhere else): checked on the operand pairs in Python."""
    seen = set()
    for case, mask in fv.group_cases():
        N, n = case.param, len(mask)
        pat = case.tag.split(" ", 2)[2]
        seen.add((N, n, pat))
        rare = np.array([fv.is_rare_pair(int(x), int(y)) for x, y in zip(case.a, case.b)]).reshape(n, N)
        assert np.array_equal(rare, np.array(mask))
        waves = [rare[w:w + 64] for w in range(0, n, 64)]
        if pat == "none":
            assert not rare.any()
        elif pat == "all":
            assert rare.all()
        elif pat == "one lane one element":
            assert all(w.sum() == 1 for w in waves)
            if n == 1000:
                assert len({int(np.argwhere(w)[0][0]) for w in waves}) > 4 and (N == 1 or len({int(np.argwhere(w)[0][1]) for w in waves}) > 1)
        elif pat == "disjoint lanes":
            assert (rare.sum(axis=1) <= 1).all() and rare[0::2].any(axis=1).all() and not rare[1::2].any()
            if N > 1 and n >= 4:
                assert rare.any(axis=0).sum() == min(N, (n + 1) // 2)       # different elements in different lanes
        else:
            assert rare[n - 1].all()
            for kb in range(1, (n + 63) // 64):
                below, above = rare[64 * kb - 1].all(), rare[64 * kb].all()
                assert below != above or 64 * kb == n - 1 or 64 * kb - 1 == n - 1
    assert seen == {(N, n, p) for N in (1, 2, 12) for n in (1, 63, 64, 65, 1000) for p in fv.GROUP_PATTERNS}


def test_dif_reference_convention():
    """dif_reference (direct DFT: w = 2^(192 / 2^K), inverse w^-1 without 1/N, slot j = X[bitrev_K(j)]) equals dif_level's
    butterfly network transcribed into Python integers, for every K and both directions; forward then inverse gives N x."""
    for k in range(1, 7):
        rows = fv.dif_rows(k, 77)[:20]
        for inv in (0, 1):
            for r in rows:
                assert fv.dif_reference(r, k, inv) == fv.dif_network(r, k, inv)
        r = rows[-1]
        f = fv.dif_reference(r, k, 0)
        nat = [f[fv.bitrev(j, k)] for j in range(1 << k)]
        back = fv.dif_reference(nat, k, 1)
        assert [back[fv.bitrev(j, k)] for j in range(1 << k)] == [(x << k) % fv.P for x in r]
    for k, inv, lv in fv.DIF_SPARSE_INSTANCES:
        assert all(not any(r[1 << lv:]) for r in fv.dif_rows(k, 1, live=1 << lv))


def run_host(pkg, case):
    case.check(pkg.field_probe_host(case.op, case.a, case.b, case.param))


@pytest.mark.parametrize("op", SCALAR_OPS)
def test_host_scalar_operation(pkg, op):
    cases = [c for c in fv.scalar_cases() if c.op == op]
    assert len(cases) == 1
    run_host(pkg, cases[0])


@pytest.mark.parametrize("op", ["mul_pow2", "mul_pow2_dyn"])
def test_host_shifts(pkg, op):
    cases = [c for c in fv.shift_cases() if c.op == op]
    assert [c.param for c in cases] == list(range(192 if op == "mul_pow2" else 96))
    for c in cases:
        run_host(pkg, c)


@pytest.mark.parametrize("terms", fv.ACC_TERMS)
def test_host_accumulator(pkg, terms):
    run_host(pkg, [c for c in fv.acc_cases() if c.param == terms][0])


@pytest.mark.parametrize("N", fv.GROUP_SIZES)
def test_host_mul_group_fallback(pkg, N):
    for case, _ in fv.group_cases():
        if case.param == N:
            run_host(pkg, case)


def test_host_probe_detects_a_wrong_word(pkg):
    """the comparison itself: one flipped bit, or a loose word where a canonical one is due, fails the case"""
    c = [c for c in fv.scalar_cases() if c.op == "canon"][0]
    got = pkg.field_probe_host(c.op, c.a)
    c.check(got)
    bad = got.copy(); bad[5] ^= np.uint64(1)
    with pytest.raises(AssertionError):
        c.check(bad)
    loose = got.copy(); loose[0] = np.uint64(fv.P)          # = 0 mod p, but not canonical
    assert int(got[0]) == 0
    with pytest.raises(AssertionError):
        c.check(loose)


def test_bad_arguments(pkg):
    lib, FP = pkg.load_library(), pkg.FP
    a = np.arange(1, 25, dtype=np.uint64); out = np.zeros(64, dtype=np.uint64)
    pa, po = a.ctypes.data, out.ctypes.data
    call = lambda op, param, a_, b_, n, o_, ow, dev=0: lib.qpgpu_field_probe(None, op, param, a_, b_, n, o_, ow, dev)
    assert call(FP["add"], 0, pa, pa, 8, po, 8) == 0
    assert call(len(pkg.FP_OPS), 0, pa, pa, 8, po, 8) == -1                 # bad op
    assert call(FP["add"], 0, None, pa, 8, po, 8) == -1 and call(FP["add"], 0, pa, None, 8, po, 8) == -1
    assert call(FP["add"], 0, pa, pa, 8, None, 8) == -1
    assert call(FP["add"], 0, pa, pa, 8, po, 7) == -1                       # short out
    assert call(FP["add"], 0, pa, pa, 0, po, 8) == -1
    assert call(FP["neg"], 0, pa, None, 8, po, 8) == 0                      # b is not read
    assert call(FP["mul_pow2"], 192, pa, None, 8, po, 8) == -1 and call(FP["mul_pow2"], 191, pa, None, 8, po, 8) == 0
    assert call(FP["mul_pow2_dyn"], 96, pa, None, 8, po, 8) == -1 and call(FP["mul_pow2_dyn"], 95, pa, None, 8, po, 8) == 0
    assert call(FP["mul_group"], 3, pa, pa, 2, po, 64) == -1 and call(FP["mul_group"], 12, pa, pa, 2, po, 23) == -1
    assert call(FP["mul_group"], 12, pa, pa, 2, po, 24) == 0
    assert call(FP["acc"], 0, pa, pa, 2, po, 64) == -1 and call(FP["acc"], 4097, pa, pa, 2, po, 64) == -1
    assert call(FP["e2_mul"], 0, pa, pa, 4, po, 7) == -1 and call(FP["e2_mul"], 0, pa, pa, 4, po, 8) == 0
    big = np.array([1 << 32, fv.P], dtype=np.uint64)
    assert call(FP["reduce96"], 0, pa, big.ctypes.data, 1, po, 8) == -1      # hi is a 32-bit word
    assert call(FP["mul_eps"], 0, big.ctypes.data, None, 1, po, 8) == -1
    assert call(FP["add_canonical"], 0, pa, big.ctypes.data, 2, po, 8) == -1   # b = p is not canonical
    # the register transforms are device code: the host path refuses them; the device path needs a context
    assert call(FP["dif_regs"], 3, pa, None, 1, po, 8) == -1 and call(FP["dif_sparse"], 4 | 1 << 16, pa, None, 1, po, 64) == -1
    assert call(FP["add"], 0, pa, pa, 8, po, 8, dev=1) == -1
    with pytest.raises(pkg.QpGpuError):
        pkg.field_probe_host("dif_regs", a[:8], param=3)
    with pytest.raises(ValueError):
        pkg.field_probe_host("e2_mul", a[:3], a[:3])
