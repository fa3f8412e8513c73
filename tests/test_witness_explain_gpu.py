"""qpgpu_circuit_explain_witness on the device (include/qpgpu.h, csrc/explain_api.cpp, explain_kernels.hip): an unsatisfied witness
explained as (row, gate, constraint, value) and (cell, source cell, both values) findings.

Independent yardstick: the CPU oracle's per-constraint evaluator of one row, orc_eval_gates_ext (oracle/prove.c), called through
ctypes with the base values embedded as (x, 0): a row's expected GATE findings are exactly {k : acc[k] != 0} with value == acc[k],
every imaginary part 0. Rows, gates and copy classes are read from the pack's selector and sigma columns here, as
tools/pack_dump.py reads them, never from the library.

Shapes: two 128-row synthetic circuits (the one of test_other_challenge_counts, and one with Poseidon2-gate rows), all 15 gate types
between them, 123 gate constraints, num_challenges 2 (and 1, 3, 4 by pack[6]): 62 expansion passes, the last with a single live
column. Every case is a handful of launches on 128 rows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import OracleCircuit

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE, COPY = 1, 2
NOOP, POSEIDON, POSEIDON2 = 0, 4, 14


class Case:
    """A pack read the way tools/pack_dump.py reads it, its satisfied witness, and the oracle's view of one row."""

    def __init__(self, pkg, orc, pack, wires, pis):
        self.pack, self.wires, self.pis = pack, wires, pis
        h = pkg.pack_header(pack)
        self.n, self.NW, self.R = 1 << h["degree_bits"], h["num_wires"], h["num_routed_wires"]
        self.nsel, self.ncon, self.C = h["num_selectors"], h["num_constants"], h["num_gate_constraints"]
        at = 18 + h["num_arity_rounds"]
        self.gates = [tuple(int(x) for x in pack[at + 8 * i:at + 8 * i + 8]) for i in range(h["num_gates"])]     # type, p0, p1, selector, g0, g1, constraints, p2
        at += 8 * h["num_gates"]
        self.k_is = [int(x) for x in pack[at:at + self.R]]
        at += self.R + 4
        self.ncs = self.nsel + self.ncon + self.R
        self.cs_at = at
        self.cs =np.array(pack[at:at + self.ncs * self.n], dtype=np.uint64).reshape(self.ncs, self.n)
        self.gate_of_row = []
        for r in range(self.n):
            sel = [int(self.cs[s, r]) for s in range(self.nsel)]
            self.gate_of_row.append(next(x for x in sel if x != 0xFFFFFFFF))
        self.orc = orc
        self.oc = OracleCircuit(orc, pack)
        f = orc.lib.orc_eval_gates_ext
        f.restype = None
        f.argtypes = [ctypes.c_void_p] * 5
        self.pih = np.ascontiguousarray(orc.hash_n_to_m(pis, 4), dtype=np.uint64)

    def close(self):
        self.oc.close()

    def type_of_row(self, r):
        return self.gates[self.gate_of_row[r]][0]

    def rows_of_type(self, t):
        return [r for r in range(self.n) if self.type_of_row(r) == t]

    def expected(self, wires, r):
        """{constraint: filter * constraint} of row r from the oracle, non-zero entries only."""
        cs_row = np.zeros((self.ncs, 2), dtype=np.uint64); cs_row[:, 0] = self.cs[:, r]
        w = np.zeros((self.NW, 2), dtype=np.uint64); w[:, 0] = wires[:, r] % np.uint64(P)
        acc = np.zeros((256, 2), dtype=np.uint64)
        self.orc.lib.orc_eval_gates_ext(self.oc.h, cs_row.ctypes.data, w.ctypes.data, self.pih.ctypes.data, acc.ctypes.data)
        assert not acc[:, 1].any(), "a base-field row gave an imaginary part"
        assert not acc[self.C:, 0].any()
        return {k: int(acc[k, 0]) for k in range(self.C) if int(acc[k, 0]) != 0}

    def corrupt(self, r, routed=None, value=None):
        """A copy of the witness with one cell of row r changed so that the oracle sees a failing constraint there: a non-routed wire
        where the row's gate reads one, otherwise a routed one (routed=True/False forces the kind). Returns (wires, wire) or None."""
        kinds = [routed] if routed is not None else [False, True]
        for want_routed in kinds:
            for wire in (range(self.R) if want_routed else range(self.R, self.NW)):
                w = self.wires.copy()
                w[wire, r] = (int(w[wire, r]) + 1) % P if value is None else value
                if int(w[wire, r]) != int(self.wires[wire, r]) and self.expected(w, r):
                    return w, wire
        return None

    def copy_classes(self):
        """The cycles of the sigma permutation, as sorted lists of (row, wire); singletons omitted."""
        wn = pow(7277203076849721926, 1 << (32 - (self.n.bit_length() - 1)), P)
        where = {}
        for c in range(self.R):
            a = self.k_is[c]
            for r in range(self.n):
                where[a] = (r, c); a = a * wn % P
        sig0 = self.nsel + self.ncon
        nxt = {(r, c): where[int(self.cs[sig0 + c, r])] for c in range(self.R) for r in range(self.n)}
        seen, classes = set(), []
        for cell in sorted(nxt):
            cyc, x = [], cell
            while x not in seen:
                seen.add(x); cyc.append(x); x = nxt[x]
            if len(cyc) > 1:
                classes.append(sorted(cyc))
        return classes


def gate_findings(found, row=None):
    return [f for f in found if f.kind == GATE and (row is None or f.row == row)]


def check_row(case, found, wires, r):
    got = gate_findings(found, r)
    want = case.expected(wires, r)
    assert {f.constraint: f.value for f in got} == want, (r, case.type_of_row(r))
    assert [f.constraint for f in got] == sorted(want)
    assert all(f.gate == case.gate_of_row[r] for f in got)


@pytest.fixture(scope="module")
def A(pkg, orc):
    c = Case(pkg, orc, *pkg.synth_circuit(7, seed=95, poseidon=True, base_sum=True, ext_arith=True, recursion=True))
    yield c
    c.close()


@pytest.fixture(scope="module")
def B(pkg, orc):
    c = Case(pkg, orc, *pkg.synth_circuit(7, seed=4, poseidon=True, base_sum=True, ext_arith=True, recursion=True, poseidon2=True))
    yield c
    c.close()


@pytest.fixture(scope="module")
def circA(pkg, gpu, A):
    c = pkg.Circuit(gpu, A.pack)
    yield c
    c.close()


@pytest.fixture(scope="module")
def circB(pkg, gpu, B):
    c = pkg.Circuit(gpu, B.pack)
    yield c
    c.close()


def test_satisfied_witness_has_no_findings(A, B, circA, circB):
    for case, circ in ((A, circA), (B, circB)):
        assert case.n == 128 and case.C == 123
        assert all(not case.expected(case.wires, r) for r in (0, 1, case.n - 1))
        assert circ.explain_witness(case.wires, case.pis) == ([], 0, 0)


def test_one_corrupted_cell_per_gate_type(A, B, circA, circB):
    types = {name: set(g[0] for g in case.gates) for name, case in (("A", A), ("B", B))}
    assert types["A"] | types["B"] == set(range(15)) and POSEIDON2 in types["B"]
    seen = set()
    for case, circ in ((A, circA), (B, circB)):
        for t in sorted(set(case.type_of_row(r) for r in range(case.n))):
            r = case.rows_of_type(t)[len(case.rows_of_type(t)) // 2]
            if t == NOOP:           # no constraints: a changed non-routed cell of a Noop row is nobody's business
                w = case.wires.copy(); w[case.NW - 1, r] = (int(w[case.NW - 1, r]) + 1) % P
                assert circ.explain_witness(w, case.pis) == ([], 0, 0)
                seen.add(t)
                continue
            w, wire = case.corrupt(r)
            found, rows, copies = circ.explain_witness(w, case.pis)
            assert rows == 1 and gate_findings(found) == gate_findings(found, r) != []
            check_row(case, found, w, r)
            if wire >= case.R:
                assert copies == 0 and all(f.kind == GATE for f in found)
            else:
                assert all((f.row, f.wire) == (r, wire) or (f.row_b, f.wire_b) == (r, wire) for f in found if f.kind == COPY)
            seen.add(t)
    assert seen == set(range(15))


def test_hash_gate_first_and_last_constraint(A, B, circA, circB):
    """PoseidonGate and the Poseidon2 gate (default layout: swap wire 24, outputs 12..23): constraint 0 is the swap boolean, constraint
    122 the last output. 123 constraints in passes of two: the last pass has one live column."""
    for case, circ, t in ((A, circA, POSEIDON), (B, circB, POSEIDON), (B, circB, POSEIDON2)):
        r = case.rows_of_type(t)[0]
        assert case.gates[case.gate_of_row[r]][6] == 123
        w = case.wires.copy(); w[24, r] = 2
        found, rows, _ = circ.explain_witness(w, case.pis)
        check_row(case, found, w, r)
        assert rows == 1 and gate_findings(found, r)[0].constraint == 0 and gate_findings(found, r)[0].value == case.expected(w, r)[0]
        w = case.wires.copy(); w[23, r] = (int(w[23, r]) + 5) % P
        found, rows, _ = circ.explain_witness(w, case.pis)
        check_row(case, found, w, r)
        assert rows == 1 and [f.constraint for f in gate_findings(found, r)] == [122]


def test_first_and_last_row(pkg, gpu, orc, A):
    """Row 0 (the PublicInputGate row) and row n - 1. The synthetic circuits end in Noop rows, which cannot fail, so the pack's selector
    columns are rewritten here to put the ConstantGate on the last row; the oracle loads the same pack."""
    pack = A.pack.copy()
    last = A.n - 1
    gi = next(i for i, g in enumerate(A.gates) if g[0] == 1)
    for s in range(A.nsel):
        pack[A.cs_at + s * A.n + last] = gi if s == A.gates[gi][3] else 0xFFFFFFFF
    E = Case(pkg, orc, pack, A.wires, A.pis)
    circ = pkg.Circuit(gpu, pack)
    try:
        assert E.type_of_row(0) == 2 and E.type_of_row(last) == 1
        w = A.wires
        for r in (0, last):
            w, _ = _corrupt_on(E, w, r)
        found, rows, _ = circ.explain_witness(w, A.pis)
        failing = sorted(r for r in range(E.n) if E.expected(w, r))
        assert rows == len(failing) and failing[0] == 0 and failing[-1] == last
        assert sorted(set(f.row for f in gate_findings(found))) == failing[:8]
        for r in failing[:8]:
            check_row(E, found, w, r)
        assert [(f.row, f.constraint) for f in gate_findings(found)] == sorted((f.row, f.constraint) for f in gate_findings(found))
    finally:
        circ.close(); E.close()


def _corrupt_on(case, wires, r, routed=None):
    """case.corrupt on top of an already changed witness."""
    keep = case.wires
    case.wires = wires
    try:
        got = case.corrupt(r, routed=routed)
    finally:
        case.wires = keep
    assert got is not None, r
    return got


@pytest.mark.parametrize("nch", [1, 3, 4])
def test_other_challenge_counts(pkg, gpu, orc, A, nch):
    """123 % 4 != 0: the last pass of four columns has three live ones; the findings do not depend on the number of challenges."""
    pack = A.pack.copy(); pack[6] = nch
    circ = pkg.Circuit(gpu, pack)
    try:
        w = A.wires
        rows_used = []
        for t in (POSEIDON, 3, 13):                      # PoseidonGate, ArithmeticGate, CosetInterpolationGate rows
            r = A.rows_of_type(t)[0]
            w, _ = _corrupt_on(A, w, r)
            rows_used.append(r)
        found, rows, _ = circ.explain_witness(w, A.pis)
        assert rows == 3
        for r in rows_used:
            check_row(A, found, w, r)                    # A's oracle: the pack at two challenges
    finally:
        circ.close()


def test_copy_constraints(A, circA):
    """Every member of a copy class of three or more cells corrupted in turn: the class's source cell (whichever the plan chose) is
    reported once per other member, any other member once, against the source, with both values."""
    cls = min((c for c in A.copy_classes() if len(c) >= 3), key=len)
    reports = {}
    for (r, c) in cls:
        w = A.wires.copy(); w[c, r] = (int(w[c, r]) + 1) % P
        found, _, copies = circA.explain_witness(w, A.pis)
        cf = [f for f in found if f.kind == COPY]
        assert copies == len(cf) >= 1
        assert [(f.row, f.wire) for f in cf] == sorted((f.row, f.wire) for f in cf)
        for f in cf:
            assert (f.row, f.wire) in cls and (f.row_b, f.wire_b) in cls and (f.row, f.wire) != (f.row_b, f.wire_b)
            assert f.value == int(w[f.wire, f.row]) % P and f.value_b == int(w[f.wire_b, f.row_b]) % P and f.value != f.value_b
        reports[(r, c)] = cf
    sources = [cell for cell, cf in reports.items() if len(cf) == len(cls) - 1]      # (a class of three or more: never 1)
    assert len(sources) == 1
    src = sources[0]
    assert sorted((f.row, f.wire) for f in reports[src]) == [c for c in cls if c != src]
    assert all((f.row_b, f.wire_b) == src for f in reports[src])
    for cell in cls:
        if cell != src:
            assert len(reports[cell]) == 1 and (reports[cell][0].row, reports[cell][0].wire) == cell and (reports[cell][0].row_b, reports[cell][0].wire_b) == src


def test_truncation_by_max_rows_and_cap(A, circA):
    rows5 = [A.rows_of_type(t)[-1] for t in (POSEIDON, 1, 5, 10, 12)]           # Poseidon, Constant, BaseSum, RandomAccess, PoseidonMds rows
    assert len(set(rows5)) == 5
    w = A.wires
    for r in rows5:
        w, _ = _corrupt_on(A, w, r)
    five, rows, copies5 = circA.explain_witness(w, A.pis, max_rows=8)
    two, rows2, copies2 = circA.explain_witness(w, A.pis, max_rows=2)
    assert rows == rows2 == 5 and copies2 == copies5
    assert sorted(set(f.row for f in gate_findings(five))) == sorted(rows5)
    assert sorted(set(f.row for f in gate_findings(two))) == sorted(rows5)[:2]
    assert two == [f for f in five if f.kind == COPY or f.row in sorted(rows5)[:2]]
    for r in sorted(rows5)[:2]:
        check_row(A, two, w, r)
    # cap: two cells of one copy class changed as well (at least one of them is not its source), so that COPY findings follow
    cls = min((c for c in A.copy_classes() if len(c) >= 3 and not set(r for r, _ in c) & set(rows5)), key=len)
    w = w.copy()
    for (r, c) in cls[:2]:
        w[c, r] = (int(w[c, r]) + 1 + c) % P
    full, rows, copies = circA.explain_witness(w, A.pis, max_rows=8)
    assert rows >= 5 and copies >= 1
    kinds = [f.kind for f in full]
    assert kinds == sorted(kinds) and COPY in kinds      # GATE findings first, then COPY
    G = kinds.count(GATE)
    for cap in (0, 1, G - 1, G, G + 1, len(full)):
        got, r_, c_ = circA.explain_witness(w, A.pis, max_rows=8, cap=cap)
        assert got == full[:cap] and (r_, c_) == (rows, copies), cap


def test_entry_variants(pkg, gpu, A, circA):
    r = A.rows_of_type(POSEIDON)[1]
    w, _ = A.corrupt(r)
    host = circA.explain_witness(w, A.pis)
    d = gpu.to_device(w)
    try:
        assert circA.explain_witness(d, A.pis) == host and host[1] == 1
        assert np.array_equal(d.download().reshape(w.shape), w)            # the caller's buffer is left as it was
    finally:
        d.free(scrub=True)
    for bad in (0, 1025):
        with pytest.raises(pkg.QpGpuError) as e:
            circA.explain_witness(w, A.pis, max_rows=bad)
        assert e.value.code == -1 and "max_rows" in str(e.value)
    assert len(circA.explain_witness(w, A.pis, max_rows=1)[0]) == len(host[0])
    assert len(circA.explain_witness(w, A.pis, max_rows=1024)[0]) == len(host[0])


def test_no_residue_of_the_witness(pkg, A):
    """A needle planted in the corrupted cell (and so in the uploaded witness, the compact trace and a COPY finding's values) is in no
    buffer of the library's after the call; with an audit open, the call's buffers are scanned right before they are freed."""
    needle = 0xC0FFEE0123456789
    assert 1 << 32 <= needle < P
    g = pkg.QpGpu(0)
    circ = pkg.Circuit(g, A.pack)
    try:
        cls = min((c for c in A.copy_classes() if len(c) >= 3), key=len)
        r, c = cls[0]
        w = A.wires.copy(); w[c, r] = needle
        w[A.NW - 1, A.rows_of_type(POSEIDON)[0]] = needle
        found, rows, copies = circ.explain_witness(w, A.pis)
        assert rows >= 1 and copies >= 1 and any(needle in (f.value, f.value_b) for f in found if f.kind == COPY)
        hits, first, nbytes = g.residue_scan([needle])
        assert hits == 0 and nbytes > 0, first
        with g.residue_audit([needle]) as a:
            assert circ.explain_witness(w, A.pis) == (found, rows, copies)
        assert a.hits == 0 and a.buffers_released >= 10, (a.hits, a.buffers_released, a.first_hits)
        assert g.residue_scan([needle])[0] == 0
    finally:
        circ.close(); g.close()


def test_existing_behaviour_is_untouched(pkg, A, circA):
    before = circA.prove(A.wires, A.pis)
    r = A.rows_of_type(5)[0]
    w, _ = A.corrupt(r, routed=False) or A.corrupt(r)
    assert circA.explain_witness(w, A.pis)[1] == 1
    assert circA.prove(A.wires, A.pis) == before
    circA.set_witness_check(True)
    try:
        with pytest.raises(pkg.QpGpuError) as e:
            circA.prove(w, A.pis)
        assert e.value.code == -4 and str(e.value) == "qpgpu error -4: witness does not satisfy the circuit: gate constraints fail at row %d" % r
        assert circA.explain_witness(w, A.pis)[1] == 1                     # usable with the check on as well
        assert circA.prove(A.wires, A.pis) == before
    finally:
        circA.set_witness_check(False)


def test_c_example_runs(tmp_path):
    out = str(tmp_path / "qpgpu_explain_example_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "explain_witness_example.c"),
                           "-L", os.path.join(ROOT, "qp-zk-circuits_amd"), "-lqpgpu",
                           "-Wl,-rpath," + os.path.join(ROOT, "qp-zk-circuits_amd"), "-o", out])
    res = subprocess.run([out, "7"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    lines = res.stdout.split("\n")
    assert lines[0].startswith("prove: witness does not satisfy the circuit: gate constraints fail at row ")
    assert "(Poseidon), constraint" in lines[1] and lines[-2].startswith("ok degree_bits=7")


def test_command_line_tool(A, tmp_path):
    r = A.rows_of_type(POSEIDON)[0]
    w, _ = A.corrupt(r)
    for name, arr in (("pack.bin", A.pack), ("wires.bin", w), ("pis.bin", A.pis)):
        np.ascontiguousarray(arr, dtype="<u8").tofile(str(tmp_path / name))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "explain_witness.py")] + [str(tmp_path / f) for f in ("pack.bin", "wires.bin", "pis.bin")],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 1, res.stdout[-1500:] + res.stderr[-1500:]
    assert ("gate constraint fails at row %d: gate %d (Poseidon), constraint" % (r, A.gate_of_row[r])) in res.stdout
    assert res.stdout.rstrip().endswith("1 row(s) with failing gate constraints (1 expanded), 0 copy mismatch(es) (0 shown)")
