"""FRI reduction schedules away from ConstantArityBits(4, 5): the case table the schedule tests share, a pack rewriter that
takes an arbitrary list of rounds, plonky2's ConstantArityBits rule restated, and a Python-integer replay of the FRI commit phase
of a proof (plain Lagrange interpolation over F_p[x]/(x^2 - 7)). A helper module, no tests; tests/REFERENCE_TESTS.md ("FRI
schedules") says what each row of the table is for."""
import ctypes

import numpy as np

P = 0xFFFFFFFF00000001
MULT_GEN = 14293326489335486720                # plonky2 GoldilocksField::MULTIPLICATIVE_GROUP_GENERATOR (the coset shift)
POWER_OF_TWO_GENERATOR = 7277203076849721926   # GoldilocksField::POWER_OF_TWO_GENERATOR = MULT_GEN^((p - 1) / 2^32)
W = 7                                          # the quadratic extension is F_p[x] / (x^2 - 7)

SCHEDULES = [
    dict(label="ones", degree_bits=8, rate_bits=3, cap_height=4, arity_bits=[1] * 7),       # no-hash leaves; last round path length 0
    dict(label="twos", degree_bits=8, rate_bits=3, cap_height=4, arity_bits=[2, 2, 2]),
    dict(label="threes", degree_bits=8, rate_bits=3, cap_height=4, arity_bits=[3, 3]),
    dict(label="falling", degree_bits=8, rate_bits=3, cap_height=2, arity_bits=[4, 3, 1]),  # 1-coefficient final polynomial, 2-coefficient LDE
    dict(label="rising", degree_bits=9, rate_bits=3, cap_height=4, arity_bits=[1, 2, 3]),
    dict(label="one_round_3", degree_bits=6, rate_bits=3, cap_height=4, arity_bits=[3]),
    dict(label="none_long_final", degree_bits=7, rate_bits=3, cap_height=4, arity_bits=[]),  # final polynomial of 128 coefficients
    dict(label="flat_cap", degree_bits=7, rate_bits=3, cap_height=0, arity_bits=[2, 4, 1]),   # cap of one digest; longest paths
]
BY_LABEL = {s["label"]: s for s in SCHEDULES}
LABELS = [s["label"] for s in SCHEDULES]


def with_schedule(pack, arity_bits, cap_height=None, rate_bits=None, num_queries=None, pow_bits=None):
    """A copy of a circuit pack with the FRI reduction schedule replaced (header word 17 and the list from word 18 on) and,
    where given, rate_bits / cap_height / proof_of_work_bits / num_query_rounds (words 10..13)."""
    pack = np.array(pack, dtype=np.uint64)
    head, rest = pack[:18].copy(), pack[18 + int(pack[17]):]
    if rate_bits is not None: head[10] = rate_bits
    if cap_height is not None: head[11] = cap_height
    if pow_bits is not None: head[12] = pow_bits
    if num_queries is not None: head[13] = num_queries
    head[17] = len(arity_bits)
    return np.concatenate([head, np.array(list(arity_bits), dtype=np.uint64), rest])


def constant_arity(degree_bits, rate_bits, cap_height, arity_bits, final_poly_bits):
    """FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) (plonky2 fri/reduction_strategies.rs): reduce by
    arity_bits while the polynomial is longer than 2^final_poly_bits and the tree of the reduced layer still holds the cap."""
    out, d = [], degree_bits
    while d > final_poly_bits and d + rate_bits - arity_bits >= cap_height and d >= arity_bits:
        out.append(arity_bits)
        d -= arity_bits
    return out


def synth_case(pkg, row, seed, **kw):
    """(pack, wires, public inputs) of the small 24-wire synthetic circuit (or of `kw`'s) under a row of SCHEDULES."""
    kw = kw or dict(num_wires=24, num_routed=16, num_public_inputs=3)
    pack, wires, pis = pkg.synth_circuit(row["degree_bits"], seed=seed, **kw)
    return with_schedule(pack, row["arity_bits"], cap_height=row["cap_height"], rate_bits=row["rate_bits"]), wires, pis


# ---- F_p[x]/(x^2 - 7) in Python integers ----

def e_add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def e_sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def e_mul(a, b): return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def root_of_unity(bits):
    return pow(POWER_OF_TWO_GENERATOR, 1 << (32 - bits), P)


def lagrange_at(xs, ys, z):
    """The value at z (extension) of the polynomial through (xs[i], ys[i]); xs in the base field, ys in the extension."""
    acc = (0, 0)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = (1, 0), 1
        for j, xj in enumerate(xs):
            if j != i:
                num = e_mul(num, e_sub(z, (xj, 0)))
                den = den * (xi - xj) % P
        di = pow(den, P - 2, P)
        acc = e_add(acc, e_mul(yi, (num[0] * di % P, num[1] * di % P)))
    return acc


class FriLayout:
    """Byte layout of a FriProof (caps, query rounds, final polynomial, proof-of-work witness) for `leaf_widths` initial
    oracles, restated from plonky2's write_fri_proof rather than read from the library."""

    def __init__(self, degree_bits, rate_bits, cap_height, arity_bits, num_queries, leaf_widths):
        self.degree_bits, self.rate_bits, self.cap_height = degree_bits, rate_bits, cap_height
        self.arity_bits, self.num_queries = list(arity_bits), num_queries
        L = degree_bits + rate_bits
        self.cap_bytes = 32 << cap_height
        self.queries_pos = len(self.arity_bits) * self.cap_bytes
        off = 0
        for w in leaf_widths:
            off += 8 * w + 1 + 32 * (L - cap_height)
        self.rounds = []            # (row offset in a query round, path length)
        lvl = L
        for ab in self.arity_bits:
            lvl -= ab
            assert lvl >= cap_height
            self.rounds.append((off, lvl - cap_height))
            off += (16 << ab) + 1 + 32 * (lvl - cap_height)
        self.q_bytes = off
        self.final_pos = self.queries_pos + num_queries * off
        self.final_n = 1 << (degree_bits - sum(self.arity_bits))
        self.pow_pos = self.final_pos + 16 * self.final_n
        self.total = self.pow_pos + 8


def _words(b, pos, n):
    return [int(x) for x in np.frombuffer(b, dtype="<u8", count=n, offset=pos)]


def replay_transcript(challenger, fri, lay):
    """Feed `challenger` (a pkg.Challenger in the state the prover's had when FRI began) what the FRI prover feeds its own, in
    the prover's order: the alpha draw, every round's cap then the beta draw, the final polynomial, the proof-of-work witness and
    its response, then one draw per query taken mod the LDE size. Returns (betas, query indices)."""
    challenger.get_n(2)                                             # fri_alpha
    betas = []
    cap_words = 4 << lay.cap_height
    for r in range(len(lay.arity_bits)):
        challenger.observe(np.array(_words(fri, r * lay.cap_bytes, cap_words), dtype=np.uint64))
        betas.append(tuple(challenger.get_n(2)))
    challenger.observe(np.array(_words(fri, lay.final_pos, 2 * lay.final_n), dtype=np.uint64))
    challenger.observe(np.array(_words(fri, lay.pow_pos, 1), dtype=np.uint64))
    challenger.get()                                                # the proof-of-work response
    lde = 1 << (lay.degree_bits + lay.rate_bits)
    return betas, [challenger.get() % lde for _ in range(lay.num_queries)]


def python_fri_check(fri, lay, betas, indices):
    """Replay the FRI commit phase of the FriProof bytes `fri` in Python integers. For every query and every round: the 2^ab
    opened extension values sit at the coset points start * g^i as evals[bitrev(i)]; their Lagrange interpolant, evaluated at
    the round's beta, must be the next round's value at position x_index & (arity - 1); after the last round it must be the
    final polynomial's Horner value at subgroup_x. Returns the list of failures as (query, round or "final", got, want); empty
    when every query passes. The sibling counts are compared with the layout as well."""
    assert len(fri) == lay.total, (len(fri), lay.total)
    L = lay.degree_bits + lay.rate_bits
    final = [tuple(_words(fri, lay.final_pos + 16 * i, 2)) for i in range(lay.final_n)]
    bad = []
    for q, x_index in enumerate(indices):
        base = lay.queries_pos + q * lay.q_bytes
        x = MULT_GEN * pow(root_of_unity(L), bitrev(x_index, L), P) % P
        carried = None
        for r, ab in enumerate(lay.arity_bits):
            off, plen = lay.rounds[r]
            arity = 1 << ab
            row = _words(fri, base + off, 2 * arity)
            if fri[base + off + 16 * arity] != plen:
                bad.append((q, r, "sibling count %d" % fri[base + off + 16 * arity], plen))
            evals = [(row[2 * i], row[2 * i + 1]) for i in range(arity)]
            within = x_index & (arity - 1)
            if carried is not None and evals[within] != carried:
                bad.append((q, r, evals[within], carried))
            g = root_of_unity(ab)
            start = x * pow(g, arity - bitrev(within, ab), P) % P      # the coset's first point: x / g^bitrev(within)
            xs = [start * pow(g, i, P) % P for i in range(arity)]
            ys = [evals[bitrev(i, ab)] for i in range(arity)]
            assert xs[bitrev(within, ab)] == x
            carried = lagrange_at(xs, ys, betas[r])
            x = pow(x, arity, P)
            x_index >>= ab
        if carried is not None:
            acc = (0, 0)
            for c in reversed(final):
                acc = e_add(e_mul(acc, (x, 0)), c)
            if acc != carried:
                bad.append((q, "final", acc, carried))
    return bad


def copy_challenger(pkg, ch):
    """A second pkg.Challenger in the same state (the struct is plain data)."""
    other = pkg.Challenger(ch.gpu)
    ctypes.memmove(ctypes.byref(other.state), ctypes.byref(ch.state), ctypes.sizeof(ch.state))
    return other


def fri_of_proof(pkg, pack, proof, pi_hash):
    """(challenger as it stands when FRI begins, FriProof bytes, FriLayout) of a whole proof of `pack`: the transcript of
    plonky2's prove() up to the openings, replayed over the proof's own caps and openings. pi_hash: the hash of the public inputs."""
    h = pkg.pack_header(pack)
    nch, n_pis = h["num_challenges"], h["num_public_inputs"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    nw, npp, nq = h["num_wires"], nch * h["num_partial_products"], nch * h["quotient_degree_factor"]
    salt = 4 if h["zero_knowledge"] else 0
    at = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"]
    capw = 4 << h["cap_height"]
    n_open = ncs + nw + 2 * nch + npp + nq
    w = np.frombuffer(proof, dtype="<u8", count=3 * capw + 2 * n_open)
    ch = pkg.Challenger()
    ch.observe(pack[at:at + 4]); ch.observe(pi_hash); ch.observe(w[:capw])
    ch.get_n(2 * nch)                                               # betas, gammas
    ch.observe(w[capw:2 * capw]); ch.get_n(nch)                     # alphas
    ch.observe(w[2 * capw:3 * capw]); ch.get_n(2)                   # zeta
    o = 3 * capw
    cs_w, o = w[o:o + 2 * (ncs + nw)], o + 2 * (ncs + nw)
    zs, o = w[o:o + 2 * nch], o + 2 * nch
    zs_next, o = w[o:o + 2 * nch], o + 2 * nch
    rest = w[o:o + 2 * (npp + nq)]
    ch.observe(np.concatenate([cs_w, zs, rest])); ch.observe(zs_next)
    fri = bytes(proof[8 * (3 * capw + 2 * n_open):len(proof) - 8 * n_pis])
    arity = [int(x) for x in pack[18:18 + h["num_arity_rounds"]]]
    lay = FriLayout(h["degree_bits"], h["rate_bits"], h["cap_height"], arity, h["num_query_rounds"],
                    [ncs, nw + salt, nch + npp + salt, nq + salt])
    return ch, fri, lay
