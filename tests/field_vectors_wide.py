"""Operand pairs for the 64 x 64 -> 128 product of gl64.hpp (mul64wide) at the carry of its cross-term sum, and their expected
results in Python integers modulo p. Shared by tests/test_mul_wide.py (census, host path), tests/test_mul_wide_gpu.py (the device
code) and tests/test_mul_wide_host.py (the word-level schedule restated in plain C++, under sanitizers).

With a = a0 + a1 2^32 and b = b0 + b1 2^32 the device code forms

    S = a1 b0 + a0 b1 + hi32(a0 b0)         (up to 2^65 - 3 2^32)

as ONE multiply-add with a 64-bit addend: M = S mod 2^64, cM = S >> 64 is that instruction's carry-out. The pairs:
  (a) every combination of 32-bit halves from HALVES: 7^4 = 2 401 pairs;
  (b) the boundaries S = 2^64 - 2, 2^64 - 1, 2^64, 2^64 + 1, a = b = 2^64 - 1, and each of these with its operands swapped;
  (c) 2^16 seeded full-range random pairs;
  (d) pairs BUILT to take mul_lazy's rare borrow (lo64 of the product below its top word) at a chosen S = k 2^32: the classes of
      the census that (a)-(c) do not reach (a rare borrow needs lo32(S) = 0, which random pairs see once in 2^32).

The census class of a pair is (cM, high word of M in {0, 0xFFFFFFFF, other}, rare borrow taken or not), from the operand values
alone. Two of the twelve combinations do not exist: S <= 2 (2^32 - 1)^2 + 2^32 - 2 = 2^65 - 3 2^32, so with cM = 1 the high word
of M is at most 0xFFFFFFFD (UNREACHABLE_CLASSES; tests/test_mul_wide.py asserts the bound)."""
import math

import numpy as np

import field_vectors as fv

P, W, T64, M64 = fv.P, fv.W, fv.T64, fv.M64
HALVES = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
BOUNDARY = ((T64 - 2, 0xFFFFFFFFAAAAAAAA, 0x2FFFFFFFF),
            (T64 - 1, 0xFFFFFFFF49249249, 0x6FFFFFFFF),
            (T64, 0xFFFFFFFF80000000, 0x3FFFFFFFF),
            (T64 + 1, 0xFFFFFFFFAAAAAAAB, 0x2FFFFFFFF))
N_RANDOM = 1 << 16
S_MAX = 2 * (W - 1) ** 2 + W - 2

MH_CLASSES = ("0", "0xFFFFFFFF", "other")
ALL_CLASSES = tuple((c, h, r) for c in (0, 1) for h in MH_CLASSES for r in (False, True))
UNREACHABLE_CLASSES = ((1, "0xFFFFFFFF", False), (1, "0xFFFFFFFF", True))
REQUIRED_CLASSES = tuple(c for c in ALL_CLASSES if c not in UNREACHABLE_CLASSES)


def cross_sum(a, b):
    a0, a1, b0, b1 = a & fv.EPS, a >> 32, b & fv.EPS, b >> 32
    return a1 * b0 + a0 * b1 + ((a0 * b0) >> 32)


def wide_class(a, b):
    s = cross_sum(a, b)
    mh = (s % T64) >> 32
    return (s >> 64, "0" if mh == 0 else "0xFFFFFFFF" if mh == fv.EPS else "other", fv.is_rare_pair(a, b))


def half_pairs():
    return [((a1 << 32) | a0, (b1 << 32) | b0) for a0 in HALVES for a1 in HALVES for b0 in HALVES for b1 in HALVES]


def boundary_pairs():
    ps = [(a, b) for _, a, b in BOUNDARY] + [(M64, M64)]
    return ps + [(b, a) for a, b in ps]


def random_pairs():
    rng = np.random.default_rng(20260)
    a, b = fv.rand64(rng, N_RANDOM), fv.rand64(rng, N_RANDOM)
    return list(zip(a, b))


def rare_pair_at(s, rng):
    """a pair with cross_sum = s (a multiple of 2^32) that takes the rare borrow: b0 odd and a0 near the top at random, b1 from
    s - hi32(a0 b0) = a0 b1 (mod b0), a1 the exact quotient; kept if a1 is a 32-bit word and lo32(a0 b0) is below the top word"""
    assert s % W == 0 and s <= S_MAX
    while True:
        b0 = int(rng.integers(1 << 23, 1 << 25)) | 1
        a0 = W - 1 - int(rng.integers(0, 1 << 18))
        if math.gcd(a0, b0) != 1:
            continue
        h00 = (a0 * b0) >> 32
        b1 = (s - h00) * pow(a0, -1, b0) % b0
        b1 += (W - 1 - b1) // b0 * b0
        r = s - a0 * b1 - h00
        if r < 0 or r % b0 or r // b0 >= W:
            continue
        a, b = ((r // b0) << 32) | a0, (b1 << 32) | b0
        assert cross_sum(a, b) == s
        if fv.is_rare_pair(a, b):
            return a, b


RARE_SUMS = (T64 - W, T64, T64 - 2 * W, T64 - 5 * W, T64 + W, T64 + 3 * W, T64 - (1 << 48), T64 + (1 << 48))


def rare_pairs():
    rng = np.random.default_rng(20261)
    return [rare_pair_at(s, rng) for s in RARE_SUMS for _ in range(4)]


_cache = {}


def pairs():
    """(a) + (b) + (c) + (d), in this order"""
    if "pairs" not in _cache:
        _cache["pairs"] = half_pairs() + boundary_pairs() + random_pairs() + rare_pairs()
    return _cache["pairs"]


def classes():
    if "classes" not in _cache:
        _cache["classes"] = [wide_class(a, b) for a, b in pairs()]
    return _cache["classes"]


def carry_pairs():
    """the pairs with cM = 1 / cM = 0 among (b), (c), (d), none of them rare unless built so"""
    if "carry" not in _cache:
        ps = boundary_pairs() + random_pairs()
        _cache["carry"] = ([p for p in ps if cross_sum(*p) >= T64], [p for p in ps if cross_sum(*p) < T64])
    return _cache["carry"]


def _labels():
    return ["cM %d, M high %s, %s" % (c, h, "rare" if r else "common") for c, h, r in classes()]


# ---- the launches ----
GROUP_SIZES = (1, 2, 12)
GROUP_PATTERNS = ("one lane", "all lanes", "wave boundary")
GROUP_THREADS = 130           # three waves, the last one partial
ACC_TERMS = (1, 3, 4096)


def mul_case():
    a, b = zip(*pairs())
    return fv.Case("mul", a, b, want=[x * y % P for x, y in pairs()], labels=_labels(), tag="wide")


def sqr_case():
    u = [x for p in pairs() for x in p]
    return fv.Case("sqr", u, want=[x * x % P for x in u], tag="wide")


def group_all_case(N):
    """all pairs, N per thread (the tail padded with the first pairs)"""
    ps = pairs()
    ps = ps + ps[:(-len(ps)) % N]
    a, b = zip(*ps)
    return fv.Case("mul_group", a, b, N, [x * y % P for x, y in ps], tag="wide N%d all pairs" % N)


def group_carry_mask(pattern, n, N):
    """[n][N] booleans: which (thread, element) products carry (cM = 1)"""
    m = [[False] * N for _ in range(n)]
    if pattern == "all lanes":
        m = [[True] * N for _ in range(n)]
    elif pattern == "one lane":
        for w in range((n + 63) // 64):
            m[64 * w + (11 * w + 5) % min(64, n - 64 * w)] = [True] * N
    else:
        m[63] = [True] * N                      # the last lane of wave 0; lane 0 of wave 1 does not carry
        m[128] = [True] * N                     # lane 0 of wave 2; the last lane of wave 1 does not carry
        m[n - 1] = [True] * N
    return m


def group_pattern_case(N, pattern):
    carry, plain = carry_pairs()
    mask = group_carry_mask(pattern, GROUP_THREADS, N)
    a, b, ic, ip = [], [], 0, 0
    for i in range(GROUP_THREADS):
        for k in range(N):
            if mask[i][k]:
                x, y = carry[ic % len(carry)]; ic += 1
            else:
                x, y = plain[ip % len(plain)]; ip += 1
            a.append(x); b.append(y)
    want = [x * y % P for x, y in zip(a, b)]
    return fv.Case("mul_group", a, b, N, want, ["carry" if any(r) else "plain" for r in mask], "wide N%d %s" % (N, pattern)), mask


def acc_case(terms):
    """rows of `terms` products: the pairs in order; then rows of one boundary pair repeated (all carries; (2^64 - 1)^2 repeated
    drives the top word as far as it goes: 4096 terms reach top = 4095)"""
    ps = pairs()
    rows = [ps[i:i + terms] for i in range(0, len(ps) - terms + 1, terms)]
    rows += [[p] * terms for p in boundary_pairs()]
    want = [sum(x * y for x, y in r) % P for r in rows]
    labels = [fv.acc_class([x for x, _ in r], [y for _, y in r]) for r in rows]
    return fv.Case("acc", [x for r in rows for x, _ in r], [y for r in rows for _, y in r], terms, want, labels, "wide T%d" % terms)


def e2_mul_case():
    ps = pairs()
    ps = ps + ps[:len(ps) % 2]
    X = [(ps[i][0], ps[i + 1][0]) for i in range(0, len(ps), 2)]
    Y = [(ps[i][1], ps[i + 1][1]) for i in range(0, len(ps), 2)]
    # and the boundary operands against themselves in both slots: (a + a x)(b + b x)
    X += [(a, a) for a, _ in boundary_pairs()]
    Y += [(b, b) for _, b in boundary_pairs()]
    return fv.Case("e2_mul", fv._flat(X), fv._flat(Y), want=fv._flat([fv.e2_mul_ref(x, y) for x, y in zip(X, Y)]), tag="wide")


def pow_case():
    """base a, exponent b: (a) and (b), the rare pairs, and the first 4096 random pairs (64 squarings and up to 64 products each)"""
    ps = half_pairs() + boundary_pairs() + rare_pairs() + random_pairs()[:4096]
    a, b = zip(*ps)
    return fv.Case("pow", a, b, want=[pow(x % P, y, P) for x, y in ps], tag="wide")


def dif_cases(k):
    """dif_regs<K> in both directions on rows whose entries are the boundary operands (and the extremes of the halves)"""
    ops = [x for p in boundary_pairs() for x in p] + [(h1 << 32) | h0 for h0 in HALVES for h1 in HALVES]
    n = 1 << k
    rows = [[ops[(r * 7 + j * (2 * r + 1)) % len(ops)] for j in range(n)] for r in range(16)]
    rows += [[v] * n for v in ops[:10]]
    return [fv.Case("dif_regs", fv._flat(rows), param=k | inv << 8, want=fv._flat([fv.dif_reference(r, k, inv) for r in rows]),
                    tag="wide K%d %s" % (k, "inverse" if inv else "forward")) for inv in (0, 1)]


def host_cases():
    """every launch the host path has (the register transforms are device code)"""
    if "host" not in _cache:
        cs = [mul_case(), sqr_case(), e2_mul_case(), pow_case()]
        cs += [group_all_case(N) for N in GROUP_SIZES]
        cs += [group_pattern_case(N, pat)[0] for N in GROUP_SIZES for pat in GROUP_PATTERNS]
        cs += [acc_case(t) for t in ACC_TERMS]
        _cache["host"] = cs
    return _cache["host"]


HOST_CASE_NAMES = tuple(["mul[wide]", "sqr[wide]", "e2_mul[wide]", "pow[wide]"] + ["mul_group[wide N%d all pairs]" % N for N in GROUP_SIZES]
                        + ["mul_group[wide N%d %s]" % (N, pat) for N in GROUP_SIZES for pat in GROUP_PATTERNS]
                        + ["acc[wide T%d]" % t for t in ACC_TERMS])


def all_dif_cases():
    if "dif" not in _cache:
        _cache["dif"] = {k: dif_cases(k) for k in range(1, 7)}
    return _cache["dif"]
