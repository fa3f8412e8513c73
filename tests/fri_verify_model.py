"""plonky2's fri::verifier::verify_fri_proof in Python integers, for any FRI instance (oracles of any width, blinded or not, any
list of opening batches, any reduction schedule): GF(p) and GF(p^2) with W = 7 from tests/fri_schedules.py, Merkle hashing through
the oracle binding's permutation (hash_or_noop, two_to_one: whichever hasher the oracle has selected). The second, independent
statement qpgpu_fri_verify and qpgpu_fri_verify_many_device are held to, next to the whole-proof host verifier. The commit phase (continuation from round to round, interpolation at beta, final polynomial) is fs.python_fri_check's; this module
adds the Merkle paths, the combination of the initial openings and the order of checks. A helper module, no tests. A verdict is the triple the library names in its reason: (kind, query, oracle or round), see KINDS; None = accepted."""
import re

import numpy as np

import fri_schedules as fs

P, W = fs.P, fs.W
e_add, e_sub, e_mul = fs.e_add, fs.e_sub, fs.e_mul

# kind -> the library's text (csrc/fri_verify.cpp: query_reason, prepare); {q} the query round, {at} the oracle or round
KINDS = {
    "oracle_plen": "query {q}: Merkle path length of oracle {at} out of range",
    "oracle_path": "query {q}: Merkle path of initial oracle {at} does not lead to its cap",
    "round_plen": "query {q}: Merkle path length of FRI round {at} out of range",
    "round_cont": "query {q}: FRI round {at} does not continue the previous evaluation",
    "round_path": "query {q}: Merkle path of FRI round {at} does not lead to its cap",
    "final": "query {q}: the final polynomial does not match the last FRI round",
    "noncanonical": "proof holds a non-canonical field element",
    "pow": "proof-of-work response has fewer than {at} leading zero bits",
}


def reason_of(verdict):
    """The library's reason text for a model verdict ("" for None)."""
    if verdict is None:
        return ""
    kind, q, at = verdict
    return KINDS[kind].format(q=q, at=at)


def verdict_of(reason):
    """The (kind, query, oracle-or-round) a reason text of the library names; None for ""."""
    if not reason:
        return None
    for kind, text in KINDS.items():
        m = re.fullmatch(re.escape(text).replace(r"\{q\}", r"(?P<q>\d+)").replace(r"\{at\}", r"(?P<at>\d+)"), reason)
        if m:
            g = m.groupdict()
            return (kind, int(g["q"]) if "q" in g else None, int(g["at"]) if "at" in g else None)
    raise AssertionError("not a verdict of the FRI verifier: %r" % reason)


def e_inv(a):
    n = pow((a[0] * a[0] - W * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, (P - a[1]) * n % P)


def e_pow(a, k):
    r = (1, 0)
    while k:
        if k & 1:
            r = e_mul(r, a)
        a = e_mul(a, a); k >>= 1
    return r


class Instance:
    """oracles: [(num_polys, blinded)]; batches: one list of (oracle, first, count) per opening point."""

    def __init__(self, degree_bits, rate_bits, cap_height, arity_bits, num_queries, oracles, batches, pow_bits=0):
        self.degree_bits, self.rate_bits, self.cap_height, self.pow_bits = degree_bits, rate_bits, cap_height, pow_bits
        self.arity_bits, self.num_queries = list(arity_bits), num_queries
        self.oracles, self.batches = [(int(n), bool(b)) for n, b in oracles], [list(b) for b in batches]
        self.widths = [n + (4 if b else 0) for n, b in self.oracles]
        self.lay = fs.FriLayout(degree_bits, rate_bits, cap_height, arity_bits, num_queries, self.widths)
        L = degree_bits + rate_bits
        self.rows, off = [], 0                      # (row offset in a query round, width, path length) per initial oracle
        for w in self.widths:
            self.rows.append((off, w, L - cap_height))
            off += 8 * w + 1 + 32 * (L - cap_height)
        self.num_openings = sum(c for b in self.batches for _, _, c in b)

    def regions(self):
        """Every region of a FriProof a tamper can land in: [(name, byte offset, bytes)] — each round cap; per query and per oracle
        or round the row (evaluations), the salt, the path-length byte, every path node; each final coefficient; the nonce."""
        lay, out = self.lay, []
        for r in range(len(self.arity_bits)):
            out.append(("cap%d" % r, r * lay.cap_bytes, lay.cap_bytes))
        for q in range(self.num_queries):
            base = lay.queries_pos + q * lay.q_bytes
            for o, (off, w, plen) in enumerate(self.rows):
                n = self.oracles[o][0]
                out.append(("q%d.o%d.row" % (q, o), base + off, 8 * n))
                if w > n:
                    out.append(("q%d.o%d.salt" % (q, o), base + off + 8 * n, 32))
                out.append(("q%d.o%d.plen" % (q, o), base + off + 8 * w, 1))
                for k in range(plen):
                    out.append(("q%d.o%d.node%d" % (q, o, k), base + off + 8 * w + 1 + 32 * k, 32))
            for r, ab in enumerate(self.arity_bits):
                off, plen = lay.rounds[r]
                out.append(("q%d.r%d.row" % (q, r), base + off, 16 << ab))
                out.append(("q%d.r%d.plen" % (q, r), base + off + (16 << ab), 1))
                for k in range(plen):
                    out.append(("q%d.r%d.node%d" % (q, r, k), base + off + (16 << ab) + 1 + 32 * k, 32))
        for i in range(lay.final_n):
            out.append(("final%d" % i, lay.final_pos + 16 * i, 16))
        out.append(("nonce", lay.pow_pos, 8))
        return out


def _words(b, pos, n):
    return [int(x) for x in np.frombuffer(b, dtype="<u8", count=n, offset=pos)] if n else []


def _path_ok(orc, row, index, nodes, cap):
    cur = [int(x) for x in orc.hash_or_noop(np.array(row, dtype=np.uint64))] if len(row) > 4 else list(row) + [0] * (4 - len(row))
    for sib in nodes:
        cur = [int(x) for x in (orc.two_to_one(sib, cur) if index & 1 else orc.two_to_one(cur, sib))]
        index >>= 1
    return cur == [int(x) for x in np.asarray(cap, dtype=np.uint64).reshape(-1, 4)[index]]


def noncanonical(inst, proof):
    """True when a field element of the FriProof (caps, rows, path nodes, final polynomial, nonce) is not below p."""
    spans = [(pos, n // 8) for name, pos, n in inst.regions() if n >= 8]
    return any(x >= P for pos, n in spans for x in _words(proof, pos, n))


def verify(orc, inst, caps, points, openings, alpha, betas, pow_response, indices, proof):
    """The verdict on a FriProof of the right length (None = accepted), checks in the library's order: canonical elements, proof
    of work, then per query: per oracle path length and path; per round path length, continuation, path; the final polynomial.
    caps: per oracle [2^cap_height, 4]; points: per batch (a, b); openings: [(a, b)] batch by batch, range by range."""
    lay = inst.lay
    assert len(proof) == lay.total
    if noncanonical(inst, proof):
        return ("noncanonical", None, None)
    if inst.pow_bits and pow_response >> (64 - inst.pow_bits):
        return ("pow", None, inst.pow_bits)
    L = inst.degree_bits + inst.rate_bits
    alpha = (int(alpha[0]), int(alpha[1]))
    reduced, at = [], 0                                 # PrecomputedReducedOpenings
    for b in inst.batches:
        n = sum(c for _, _, c in b)
        red = (0, 0)
        for v in reversed(openings[at:at + n]):
            red = e_add(e_mul(red, alpha), (int(v[0]), int(v[1])))
        reduced.append(red); at += n
    cap_words = 4 << inst.cap_height
    round_caps = [_words(proof, r * lay.cap_bytes, cap_words) for r in range(len(inst.arity_bits))]
    final = [tuple(_words(proof, lay.final_pos + 16 * i, 2)) for i in range(lay.final_n)]
    commit_bad = {(f[0], f[1]) for f in fs.python_fri_check(proof, lay, [(int(b[0]), int(b[1])) for b in betas], [int(i) for i in indices])
                  if not isinstance(f[2], str)}              # the sibling counts are checked below, in the verifier's order

    def final_at(x):
        acc = (0, 0)
        for c in reversed(final):
            acc = e_add(e_mul(acc, (x, 0)), c)
        return acc

    for q, x_index in enumerate(indices):
        x_index = int(x_index)
        base = lay.queries_pos + q * lay.q_bytes
        rows = []
        for o, (off, w, plen) in enumerate(inst.rows):
            row = _words(proof, base + off, w)
            rows.append(row)
            got = proof[base + off + 8 * w]
            if got > 60:
                return ("oracle_plen", q, o)
            nodes = [_words(proof, base + off + 8 * w + 1 + 32 * k, 4) for k in range(plen)]
            if got != plen or not _path_ok(orc, row, x_index, nodes, caps[o]):
                return ("oracle_path", q, o)
        x = fs.MULT_GEN * pow(fs.root_of_unity(L), fs.bitrev(x_index, L), P) % P
        total = (0, 0)                                  # fri_combine_initial
        for b, ranges in enumerate(inst.batches):
            evals = [rows[o][f + j] for o, f, c in ranges for j in range(c)]
            e = (0, 0)
            for v in reversed(evals):
                e = e_add(e_mul(e, alpha), (v, 0))
            pt = (int(points[b][0]), int(points[b][1]))
            term = e_mul(e_sub(e, reduced[b]), e_inv(e_sub((x, 0), pt)))
            total = e_add(e_mul(total, e_pow(alpha, len(evals))), term)
        # the commit phase is fs.python_fri_check's: which rounds fail to continue the one before, which queries miss the final
        # polynomial. What it does not know is what round 0 continues (the combined initial openings), nor the order of checks.
        if inst.arity_bits:
            if total != tuple(_words(proof, base + lay.rounds[0][0] + 16 * (x_index & ((1 << inst.arity_bits[0]) - 1)), 2)):
                commit_bad.add((q, 0))
        elif total != final_at(x):
            commit_bad.add((q, "final"))
        for r, ab in enumerate(inst.arity_bits):
            off, plen = lay.rounds[r]
            arity = 1 << ab
            row = _words(proof, base + off, 2 * arity)
            got = proof[base + off + 16 * arity]
            if got > 60:
                return ("round_plen", q, r)
            if (q, r) in commit_bad:
                return ("round_cont", q, r)
            nodes = [_words(proof, base + off + 16 * arity + 1 + 32 * k, 4) for k in range(plen)]
            if got != plen or not _path_ok(orc, row, x_index >> ab, nodes, round_caps[r]):
                return ("round_path", q, r)
            x_index >>= ab
        if (q, "final") in commit_bad:
            return ("final", q, None)
    return None


def plonk_view(pkg, pack, proof, pi_hash, cs_cap):
    """The FRI part of a whole proof of `pack` as a 4-oracle, 2-batch instance (fs.fri_of_proof with what a FRI verifier needs
    besides the bytes): dict(oracles, batches, caps, points, openings, challenger (as FRI begins), fri, lay, base (offset of the
    FriProof in the proof), header)."""
    h = pkg.pack_header(pack)
    nch = h["num_challenges"]
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    nw, npp, nq = h["num_wires"], nch * h["num_partial_products"], nch * h["quotient_degree_factor"]
    zk = bool(h["zero_knowledge"])
    at = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"]
    capw = 4 << h["cap_height"]
    n_open = ncs + nw + 2 * nch + npp + nq
    w = np.frombuffer(proof, dtype="<u8", count=3 * capw + 2 * n_open)
    ch = pkg.Challenger()
    ch.observe(pack[at:at + 4]); ch.observe(pi_hash); ch.observe(w[:capw])
    ch.get_n(2 * nch)
    ch.observe(w[capw:2 * capw]); ch.get_n(nch)
    ch.observe(w[2 * capw:3 * capw])
    zeta = tuple(ch.get_n(2))
    o = 3 * capw
    cs_w, o = w[o:o + 2 * (ncs + nw)], o + 2 * (ncs + nw)
    zs, o = w[o:o + 2 * nch], o + 2 * nch
    zs_next, o = w[o:o + 2 * nch], o + 2 * nch
    rest = w[o:o + 2 * (npp + nq)]
    ch.observe(np.concatenate([cs_w, zs, rest])); ch.observe(zs_next)
    _, fri, lay = fs.fri_of_proof(pkg, pack, proof, pi_hash)
    g = fs.root_of_unity(h["degree_bits"])
    return dict(
        oracles=[(ncs, False), (nw, zk), (nch + npp, zk), (nq, zk)],
        batches=[[(0, 0, ncs), (1, 0, nw), (2, 0, nch + npp), (3, 0, nq)], [(2, 0, nch)]],
        caps=[np.array(cs_cap, dtype=np.uint64).reshape(-1, 4)] + [w[k * capw:(k + 1) * capw].reshape(-1, 4).copy() for k in range(3)],
        points=[zeta, (zeta[0] * g % P, zeta[1] * g % P)],
        openings=np.concatenate([cs_w, zs, rest, zs_next]).reshape(-1, 2).copy(),
        challenger=ch, fri=fri, lay=lay, base=8 * (3 * capw + 2 * n_open), header=h)
