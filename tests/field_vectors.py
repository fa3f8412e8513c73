"""Operands for the field probe (qpgpu_field_probe) and their expected results in plain Python integers modulo p.

Shared by tests/test_field_probe.py (host versions of the primitives) and tests/test_field_probe_gpu.py (the device code).
Every case carries, per index, the CENSUS class of its operands: which rare carry / borrow the operands trigger, computed here
from the operand values alone (never from what the code under test returns). The tests assert that every class keeps at least
MIN_PER_CLASS cases, so that an edit of the vectors cannot silently lose a branch.

A result word r is right iff int(r) % P == want; operations documented to return canonical values must also be < P."""
import collections

import numpy as np

P = 0xFFFFFFFF00000001
W = 1 << 32
EPS = W - 1
T64 = 1 << 64
M64 = T64 - 1
MIN_PER_CLASS = 16

FP_OPS = ("canon", "add", "sub", "neg", "mul", "sqr", "reduce128", "reduce96", "mul_eps", "add_canonical", "mul7", "inv", "pow",
          "mul_pow2", "mul_pow2_dyn", "mul_group", "acc", "e2_add", "e2_sub", "e2_mul", "e2_scale", "e2_inv", "e2_pow", "dif_regs",
          "dif_sparse")
CANONICAL_OPS = ("canon", "inv", "pow", "e2_inv", "e2_pow")
DEVICE_ONLY_OPS = ("dif_regs", "dif_sparse")


def _dedup(xs):
    seen, out = set(), []
    for x in xs:
        assert 0 <= x < T64
        if x not in seen:
            seen.add(x); out.append(x)
    return out


# the edge set E: small values, the 2^32 and 2^63 neighbourhoods, both sides of p, the top of the u64 range ("loose" values
# in [p, 2^64) are the point), and words with an extreme high half over a zero or an all-ones low half
E = _dedup([0, 1, 2, 7, 1 << 31, W - 2, W - 1, W, W + 1, 2 * W - 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1,
            P - W, P - 2, P - 1, P, P + 1, P + W - 2,
            T64 - W + 1, T64 - W + 2, T64 - W - 1, T64 - 2, T64 - 1]
           + [m * W + lo for m in (1, 1 << 16, 1 << 31, W - 2, W - 1) for lo in (0, EPS)]
           + [3, 8, 1 << 16, 1 << 33, 1 << 48, 1 << 62, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, W + (1 << 31), 3 * W,
              P - 7, P + 7, P + (1 << 31), T64 - 2 * W + 1, T64 - (1 << 31), (1 << 63) + W, (1 << 63) - W, 0x0123456789ABCDEF,
              4, 6, (1 << 16) - 1, (1 << 48) - 1, P - (1 << 31), T64 - 3, (1 << 63) + EPS, 0xFFFFFFFE00000001])
E32 = [e for e in E if e < W]
E_CANON = [e for e in E if e < P]
EXTREMES = [0, 1, W - 1, W, P - 1, P, T64 - 1]


def _rng(seed):
    return np.random.default_rng(seed)


def rand64(rng, n):
    return [int(x) for x in rng.integers(0, M64, size=n, dtype=np.uint64, endpoint=True)]


def rand32(rng, n):
    return [int(x) for x in rng.integers(0, W, size=n, dtype=np.uint64)]


def u64(xs):
    return np.array(xs, dtype=np.uint64)


# ---- census: which rare branch the operands of one index take (operand values only) ----
def add_class(a, b):
    s = a + b
    if s < T64:
        return "no carry"
    return "two carries" if (s - T64) + EPS >= T64 else "one carry"


def sub_class(a, b):
    if a >= b:
        return "no borrow"
    return "two borrows" if (a - b + T64) < EPS else "one borrow"


def reduce128_class(lo, hi):
    hh, hl = hi >> 32, hi & EPS
    borrow = lo < hh
    t = (lo - hh - (EPS if borrow else 0)) % T64
    carry = hl * EPS + t >= T64
    return ("borrow" if borrow else "no borrow") + ", " + ("carry" if carry else "no carry")


def mul_class(a, b):
    m = a * b
    return reduce128_class(m & M64, m >> 64)


def is_rare_pair(a, b):
    """the 128-bit product has lo < hi >> 32: the borrow mul_group folds behind its wave-uniform branch"""
    m = a * b
    return (m & M64) < (m >> 96)


def reduce96_class(lo, hi):
    return "carry" if hi * EPS + lo >= T64 else "no carry"


def acc_class(a_row, b_row):
    top = sum(x * y for x, y in zip(a_row, b_row)) >> 128
    return "top = 0" if top == 0 else "top = 1" if top == 1 else "top >= 2"


REQUIRED_CLASSES = {
    "add": ("no carry", "one carry", "two carries"),
    "sub": ("no borrow", "one borrow", "two borrows"),
    "reduce128": ("borrow, carry", "borrow, no carry", "no borrow, carry", "no borrow, no carry"),
    "mul": ("borrow, carry", "borrow, no carry", "no borrow, carry", "no borrow, no carry"),
    "reduce96": ("carry", "no carry"),
    "acc": ("top = 0", "top = 1", "top >= 2"),
}


class Case:
    """one launch of the probe: flat operand words, expected values (flat, one per output word), a census label per index"""

    def __init__(self, op, a, b=None, param=0, want=None, labels=None, tag=""):
        self.op, self.param, self.tag = op, param, tag
        self.a = u64(a)
        self.b = None if b is None else u64(b)
        self.want = want
        self.labels = labels
        self.canonical = op in CANONICAL_OPS
        self.device_only = op in DEVICE_ONLY_OPS

    @property
    def name(self):
        return self.op + (("[%s]" % self.tag) if self.tag else "")

    def check(self, got):
        """got: the probe's raw output words. Raises with the first mismatches (operand index, census class)."""
        got = [int(x) for x in np.asarray(got).ravel()]
        assert len(got) == len(self.want), (self.name, len(got), len(self.want))
        wo = len(got) // max(1, len(self.labels)) if self.labels else 1
        bad = [i for i, (g, w) in enumerate(zip(got, self.want)) if g % P != w or (self.canonical and g >= P)]
        if bad:
            lines = []
            for i in bad[:8]:
                lab = self.labels[i // wo] if self.labels else ""
                lines.append("  out[%d] = %#x (mod p %#x), want %#x %s" % (i, got[i], got[i] % P, self.want[i], lab))
            raise AssertionError("%s param %d: %d of %d result words wrong\n%s" % (self.name, self.param, len(bad), len(got), "\n".join(lines)))


def _pairs(xs, ys):
    return [x for x in xs for _ in ys], [y for _ in xs for y in ys]


def _binary_operands(seed, extra=()):
    """E x E, constructive extras, 4096 random full-range pairs"""
    a, b = _pairs(E, E)
    for x, y in extra:
        a.append(x); b.append(y)
    rng = _rng(seed)
    return a + rand64(rng, 4096), b + rand64(rng, 4096)


def _unary_operands(seed):
    return E + rand64(_rng(seed), 1024)


def _constructive_add(rng):
    # two carries: a + b >= 2^65 - 2^32 + 1, both operands within 2^31 of the top
    hi = [T64 - 1 - int(x) for x in rng.integers(0, 1 << 31, size=128, dtype=np.uint64)]
    return list(zip(hi[:64], hi[64:]))


def _constructive_sub(rng):
    # two borrows: a < b and a - b + 2^64 < 2^32 - 1: a tiny, b within 2^31 of the top
    lo = [int(x) for x in rng.integers(0, 1 << 30, size=64, dtype=np.uint64)]
    hi = [T64 - 1 - int(x) for x in rng.integers(0, 1 << 30, size=64, dtype=np.uint64)]
    return list(zip(lo, hi))


def rare_pair(rng, with_carry=None):
    """(m 2^32, k 2^32) with m k >= 2^32: the product is m k 2^64, a zero low half under a top word: the reduce128 borrow. The
    carry of the multiply-add behind it follows the low word of m k: 0 or 1 -> none, above -> one."""
    while True:
        if with_carry is False:
            m, k = (int(x) << 16 for x in rng.integers(1 << 8, 1 << 16, size=2))       # m k = 0 mod 2^32
        else:
            m, k = (int(x) for x in rng.integers(1 << 16, W, size=2))
        a, b = m * W, k * W
        if not is_rare_pair(a, b):
            continue
        if with_carry is None or ("no carry" not in mul_class(a, b)) == with_carry:
            return a, b


def common_pair(rng):
    while True:
        a, b = rand64(rng, 2)
        if not is_rare_pair(a, b):
            return a, b


def _constructive_mul(rng):
    out = [rare_pair(rng, True) for _ in range(48)] + [rare_pair(rng, False) for _ in range(48)]
    # no borrow and no carry: small products
    out += [(int(x), int(y)) for x, y in rng.integers(0, W, size=(32, 2), dtype=np.uint64)]
    return out


def _constructive_reduce128(rng):
    out = []
    for _ in range(32):
        hh, hl = (int(x) for x in rng.integers(1, W, size=2))
        out.append((int(rng.integers(0, hh)), (hh << 32) | hl))               # lo < hi_hi: borrow
        out.append((int(rng.integers(0, hh)), (hh << 32) | int(rng.integers(0, 2))))   # borrow, hi_lo in {0, 1}: no carry
    return out


# ---- extension field F[x]/(x^2 - 7) on word pairs ----
def e2_mul_ref(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def e2_pow_ref(x, e):
    r, x = (1, 0), (x[0] % P, x[1] % P)
    while e:
        if e & 1:
            r = e2_mul_ref(r, x)
        x = e2_mul_ref(x, x)
        e >>= 1
    return r


def e2_inv_ref(x):
    a, b = x[0] % P, x[1] % P
    ni = pow((a * a - 7 * b * b) % P, P - 2, P)          # 0 for the zero element, as the device's a^(p-2) gives
    return (a * ni % P, (P - b) * ni % P)


def _flat(pairs):
    return [w for p in pairs for w in p]


# ---- the register transforms ----
def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def dif_reference(row, k, inverse):
    """Direct O(4^K) DFT in Python integers, in the convention read off dif_level (ntt_kernel_impl.hpp): root w = 2^(192 / 2^K)
    (2^192 = 1 mod p), the inverse direction uses w^-1 = 2^(192 - 192 / 2^K) and carries NO 1/N factor, and output slot j holds
    X[bitrev_K(j)]."""
    n = 1 << k
    step = 192 // n
    w = pow(2, (192 - step) % 192 if inverse else step, P)
    pw = [pow(w, i, P) for i in range(n)]
    xs = [sum(row[j] * pw[(j * kk) % n] for j in range(n)) % P for kk in range(n)]
    return [xs[bitrev(j, k)] for j in range(n)]


def dif_network(row, k, inverse):
    """dif_level transcribed butterfly by butterfly (Python integers mod p): pins dif_reference's convention without a GPU."""
    n = 1 << k
    x = [v % P for v in row]
    ln = n
    while ln >= 2:
        half, step = ln // 2, 192 // ln
        for b in range(0, n, ln):
            for j in range(half):
                u, v = x[b + j], x[b + j + half]
                s = (((ln - j) % ln) if inverse else j) * step
                x[b + j] = (u + v) % P
                x[b + j + half] = (u - v) * pow(2, s, P) % P
        ln = half
    return x


DIF_SPARSE_INSTANCES = ((4, 0, 1), (5, 0, 2))      # (K, INV, LV) of the LDE pass kernels (lde_sparse_lv)


def dif_rows(k, seed, live=None):
    """input rows of 2^K words: rows cycling through E, all-equal rows of each extreme, random full-range rows; with `live`,
    the words from index `live` on are zero (dif_sparse's contract)"""
    n = 1 << k
    rows = [[E[(r * 5 + j * (2 * r + 1)) % len(E)] for j in range(n)] for r in range(10)]
    rows += [[v] * n for v in EXTREMES]
    rng = _rng(seed)
    rows += [rand64(rng, n) for _ in range(48)]
    if live is not None:
        rows = [r[:live] + [0] * (n - live) for r in rows]
    return rows


# ---- mul_group wave patterns ----
GROUP_SIZES = (1, 2, 12)
GROUP_THREADS = (1, 63, 64, 65, 1000)
GROUP_PATTERNS = ("none", "one lane one element", "all", "disjoint lanes", "wave boundary")


def group_rare_mask(pattern, n, N):
    """[n][N] booleans: which (thread, element) products are rare"""
    m = [[False] * N for _ in range(n)]
    if pattern == "all":
        m = [[True] * N for _ in range(n)]
    elif pattern == "one lane one element":
        for w in range((n + 63) // 64):
            lanes = min(64, n - 64 * w)
            m[64 * w + (7 * w + 3) % lanes][(5 * w + 1) % N] = True
    elif pattern == "disjoint lanes":
        for i in range(0, n, 2):
            m[i][(i // 2) % N] = True                   # even lanes, each in an element of its own
    elif pattern == "wave boundary":
        for kb in range(1, (n + 63) // 64):
            m[64 * kb - (1 if kb % 2 == 0 else 0)] = [True] * N      # even boundary: the last lane below; odd: the first above
        m[n - 1] = [True] * N                            # and the last live lane, next to the lanes the tail guard retired
    return m


def group_case(N, n, pattern, seed):
    rng = _rng(seed)
    mask = group_rare_mask(pattern, n, N)
    a, b = [], []
    for i in range(n):
        for k in range(N):
            x, y = rare_pair(rng) if mask[i][k] else common_pair(rng)
            assert is_rare_pair(x, y) == mask[i][k]
            a.append(x); b.append(y)
    want = [x * y % P for x, y in zip(a, b)]
    labels = ["rare" if any(r) else "common" for r in mask]
    return Case("mul_group", a, b, N, want, labels, "N%d n%d %s" % (N, n, pattern)), mask


# ---- accumulator chains ----
ACC_TERMS = (1, 2, 3, 257, 1024)


def acc_case(terms, seed):
    rng = _rng(seed)
    if terms == 1024:
        # all (near-)maximal operands; row 0 is (2^64 - 1, 2^64 - 1) throughout
        rows = [([M64 - (r % 4)] * terms, [M64 - ((r // 4) % 4)] * terms) for r in range(32)]
    else:
        rows = [([x] * terms, [y] * terms) for x in (M64, P - 1, P, EPS * W, 1 << 63, 0, 1) for y in (M64, P - 1, 1 << 63, EPS)]
        rows += [([E[(r + 3 * t) % len(E)] for t in range(terms)], [E[(5 * r + 7 * t + 1) % len(E)] for t in range(terms)]) for r in range(24)]
        rows += [(rand64(rng, terms), rand64(rng, terms)) for _ in range(24)]
        rows += [([M64 - v for v in rand32(rng, terms)], [M64 - v for v in rand32(rng, terms)]) for _ in range(24)]
        rows += [(rand32(rng, terms), rand64(rng, terms)) for _ in range(20)]
    assert len(rows) <= 256
    want = [sum(x * y for x, y in zip(ra, rb)) % P for ra, rb in rows]
    labels = [acc_class(ra, rb) for ra, rb in rows]
    return Case("acc", _flat([ra for ra, _ in rows]), _flat([rb for _, rb in rows]), terms, want, labels, "T%d" % terms)


# ---- the whole table ----
_cache = {}


def scalar_cases():
    """basic operations, pow, inv, the extension field: one case per operation"""
    if "scalar" in _cache:
        return _cache["scalar"]
    cs = []
    u = _unary_operands(1)
    cs.append(Case("canon", u, want=[x % P for x in u]))
    cs.append(Case("neg", u, want=[-x % P for x in u]))
    cs.append(Case("sqr", u, want=[x * x % P for x in u], labels=[mul_class(x, x) for x in u]))
    cs.append(Case("mul7", u, want=[7 * x % P for x in u]))
    cs.append(Case("inv", u, want=[pow(x % P, P - 2, P) for x in u]))
    u32 = E32 + rand32(_rng(2), 1024)
    cs.append(Case("mul_eps", u32, want=[x * EPS % P for x in u32]))

    a, b = _binary_operands(3, _constructive_add(_rng(103)))
    cs.append(Case("add", a, b, want=[(x + y) % P for x, y in zip(a, b)], labels=[add_class(x, y) for x, y in zip(a, b)]))
    a, b = _binary_operands(4, _constructive_sub(_rng(104)))
    cs.append(Case("sub", a, b, want=[(x - y) % P for x, y in zip(a, b)], labels=[sub_class(x, y) for x, y in zip(a, b)]))
    a, b = _binary_operands(5, _constructive_mul(_rng(105)))
    cs.append(Case("mul", a, b, want=[x * y % P for x, y in zip(a, b)], labels=[mul_class(x, y) for x, y in zip(a, b)]))
    a, b = _binary_operands(6, _constructive_reduce128(_rng(106)))          # (lo, hi), hi unrestricted
    cs.append(Case("reduce128", a, b, want=[(x + y * T64) % P for x, y in zip(a, b)], labels=[reduce128_class(x, y) for x, y in zip(a, b)]))
    a, b = _pairs(E, E32)
    rng = _rng(7)
    a, b = a + rand64(rng, 4096), b + rand32(rng, 4096)
    cs.append(Case("reduce96", a, b, want=[(x + y * T64) % P for x, y in zip(a, b)], labels=[reduce96_class(x, y) for x, y in zip(a, b)]))
    a, b = _pairs(E, E_CANON)
    rng = _rng(8)
    a, b = a + rand64(rng, 4096), b + [x % P for x in rand64(rng, 4096)]
    cs.append(Case("add_canonical", a, b, want=[(x + y) % P for x, y in zip(a, b)], labels=[add_class(x, y) for x, y in zip(a, b)]))
    a, b = _binary_operands(9)
    cs.append(Case("pow", a, b, want=[pow(x % P, y, P) for x, y in zip(a, b)]))

    # extension elements: every (E, E) word pair against a scrambled partner, all pairs of the extreme elements, random ones
    L = len(E)
    xs = [(E[i], E[j]) for i in range(L) for j in range(L)]
    ys = [(E[(3 * i + j + 1) % L], E[(i + 5 * j + 2) % L]) for i in range(L) for j in range(L)]
    ext = [(p, q) for p in EXTREMES for q in EXTREMES]
    px, py = _pairs(ext, ext)
    rng = _rng(10)
    rx = [tuple(rand64(rng, 2)) for _ in range(4096)]
    ry = [tuple(rand64(rng, 2)) for _ in range(4096)]
    X, Y = xs + px + rx, ys + py + ry
    cs.append(Case("e2_add", _flat(X), _flat(Y), want=_flat([((x[0] + y[0]) % P, (x[1] + y[1]) % P) for x, y in zip(X, Y)])))
    cs.append(Case("e2_sub", _flat(X), _flat(Y), want=_flat([((x[0] - y[0]) % P, (x[1] - y[1]) % P) for x, y in zip(X, Y)])))
    cs.append(Case("e2_mul", _flat(X), _flat(Y), want=_flat([e2_mul_ref(x, y) for x, y in zip(X, Y)])))
    S = [y[0] for y in Y]
    cs.append(Case("e2_scale", _flat(X), S, want=_flat([(x[0] * s % P, x[1] * s % P) for x, s in zip(X, S)])))
    U = xs + rx[:1024]
    cs.append(Case("e2_inv", _flat(U), want=_flat([e2_inv_ref(x) for x in U])))
    pxs, pes = _pairs([(E[i], E[(7 * i + 3) % L]) for i in range(L)], E)
    pxs, pes = pxs + rx[:1024], pes + rand64(rng, 1024)
    cs.append(Case("e2_pow", _flat(pxs), pes, want=_flat([e2_pow_ref(x, e) for x, e in zip(pxs, pes)])))
    _cache["scalar"] = cs
    return cs


def shift_cases():
    """mul_pow2<S> for every S in 0..191 and the NTT's mul_pow2_dyn for s in 0..95, each on E plus 1024 random words"""
    if "shift" in _cache:
        return _cache["shift"]
    u = _unary_operands(11)
    cs = [Case("mul_pow2", u, param=s, want=[x * pow(2, s, P) % P for x in u], tag="S%d" % s) for s in range(192)]
    cs += [Case("mul_pow2_dyn", u, param=s, want=[x * pow(2, s, P) % P for x in u], tag="s%d" % s) for s in range(96)]
    _cache["shift"] = cs
    return cs


def acc_cases():
    if "acc" not in _cache:
        _cache["acc"] = [acc_case(t, 20 + t) for t in ACC_TERMS]
    return _cache["acc"]


def group_cases():
    """[(Case, rare mask)] for every N, thread count and wave pattern"""
    if "group" not in _cache:
        _cache["group"] = [group_case(N, n, pat, 1000 * N + 10 * n + pi) for N in GROUP_SIZES for n in GROUP_THREADS
                           for pi, pat in enumerate(GROUP_PATTERNS)]
    return _cache["group"]


def dif_cases():
    """dif_regs<K, INV> for K in 1..6, both directions, and the dif_sparse instances of the LDE kernels (device only)"""
    if "dif" in _cache:
        return _cache["dif"]
    cs = []
    for k in range(1, 7):
        rows = dif_rows(k, 30 + k)
        for inv in (0, 1):
            cs.append(Case("dif_regs", _flat(rows), param=k | inv << 8, want=_flat([dif_reference(r, k, inv) for r in rows]),
                           tag="K%d %s" % (k, "inverse" if inv else "forward")))
    for k, inv, lv in DIF_SPARSE_INSTANCES:
        rows = dif_rows(k, 40 + k, live=1 << lv)
        cs.append(Case("dif_sparse", _flat(rows), param=k | inv << 8 | lv << 16, want=_flat([dif_reference(r, k, inv) for r in rows]),
                       tag="K%d LV%d" % (k, lv)))
    _cache["dif"] = cs
    return cs


def census(cases):
    """op -> Counter of census classes over the given cases"""
    out = collections.defaultdict(collections.Counter)
    for c in cases:
        if c.labels:
            out[c.op].update(c.labels)
    return out
