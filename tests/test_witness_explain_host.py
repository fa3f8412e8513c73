"""qpgpu_circuit_explain_witness (include/qpgpu.h), the parts that need no device: the text qpgpu_witness_finding_format writes for
hand-made findings against the golden pack (exact lines, truncation at cap, findings that do not fit the pack are refused without a
read), the finding structure's layout, the new entries' refusal of a NULL handle; and two stand-alone programs under
AddressSanitizer and UndefinedBehaviorSanitizer: the ordered selection from a bitmap (csrc/explain_select.hpp,
tests/native/explain_select_main.cpp) and the exactness of the hash gates' folded form under one-hot weights
(tools/host_checks/explain_one_hot_check.cpp), which is what lets the expansion pass read single constraints out of the kernels that
judge the witness. The call itself is tested on the device by tests/test_witness_explain_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC]


@pytest.fixture(scope="module")
def pack():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "pack_small.bin"), dtype="<u8")


def test_format_exact_text(pkg, pack):
    B = pkg.binding
    g = B.WitnessFinding(kind=B.FINDING_GATE, gate=13, constraint=40, row=63, value=0xFFFFFFFF00000000)
    assert B.format_finding(pack, g) == "gate constraint fails at row 63: gate 13 (Poseidon2), constraint 40 of 123, filtered value 18446744069414584320"
    g = B.WitnessFinding(kind=B.FINDING_GATE, gate=8, constraint=0, row=0, value=1)
    assert B.format_finding(pack, g) == "gate constraint fails at row 0: gate 8 (Arithmetic), constraint 0 of 20, filtered value 1"
    c = B.WitnessFinding(kind=B.FINDING_COPY, wire=79, row=5, value=7, wire_b=0, row_b=63, value_b=1 << 63)
    assert B.format_finding(pack, c) == ("copy constraint violated: wire 79 of row 5 holds 7, the source of its copy class, wire 0 of row 63, "
                                         "holds 9223372036854775808")
    # the gate names are tools/pack_dump.py's, for every gate of the pack
    import importlib.util
    spec = importlib.util.spec_from_file_location("pack_dump", os.path.join(ROOT, "tools", "pack_dump.py"))
    pd = importlib.util.module_from_spec(spec); spec.loader.exec_module(pd)
    h = pkg.pack_header(pack)
    at = 18 + int(pack[17])
    for gi in range(int(h["num_gates"])):
        t, nc = int(pack[at + 8 * gi]), int(pack[at + 8 * gi + 6])
        if nc == 0:
            continue
        line = B.format_finding(pack, B.WitnessFinding(kind=B.FINDING_GATE, gate=gi, constraint=nc - 1, row=1, value=2))
        assert "gate %d (%s), constraint %d of %d" % (gi, pd.GATE_NAMES[t], nc - 1, nc) in line
    # the header form of the pack (no constants/sigmas values) serves as well
    assert B.format_finding(pkg.stage_header_words(pack), c).startswith("copy constraint violated: wire 79 of row 5")


def test_format_truncates_at_cap(pkg, pack):
    lib = pkg.load_library()
    B = pkg.binding
    f = B.WitnessFinding(kind=B.FINDING_GATE, gate=13, constraint=40, row=63, value=5)._c()
    full = B.format_finding(pack, B.WitnessFinding(kind=B.FINDING_GATE, gate=13, constraint=40, row=63, value=5))
    for cap in (1, 2, 17, len(full), len(full) + 1):
        buf = ctypes.create_string_buffer(b"\xAA" * (cap + 8), cap + 8)
        rc = lib.qpgpu_witness_finding_format(pack.ctypes.data, pack.size, ctypes.byref(f), buf, cap)
        assert rc == (0 if cap > len(full) else -5), cap
        k = min(cap - 1, len(full))
        assert buf.raw[:k + 1] == full.encode()[:k] + b"\0"
        assert buf.raw[k + 1:] == b"\xAA" * (cap + 8 - k - 1)         # nothing past the NUL, let alone past cap
    with pytest.raises(pkg.QpGpuError) as e:
        B.format_finding(pack, B.WitnessFinding(kind=B.FINDING_GATE, gate=13, constraint=40, row=63, value=5), cap=20)
    assert e.value.code == -5


def test_format_refuses_what_does_not_fit_the_pack(pkg, pack):
    lib = pkg.load_library()
    B = pkg.binding
    bad = [B.WitnessFinding(kind=B.FINDING_GATE, gate=15, constraint=0, row=0),              # the pack has gates 0..14
           B.WitnessFinding(kind=B.FINDING_GATE, gate=0xFFFFFFFF, constraint=0, row=0),
           B.WitnessFinding(kind=B.FINDING_GATE, gate=8, constraint=20, row=0),              # Arithmetic has 20 constraints
           B.WitnessFinding(kind=B.FINDING_GATE, gate=0, constraint=0, row=0),               # Noop has none
           B.WitnessFinding(kind=B.FINDING_GATE, gate=8, constraint=0, row=64),              # 2^6 rows
           B.WitnessFinding(kind=B.FINDING_COPY, wire=80, row=0, wire_b=0, row_b=0),         # 80 routed wires
           B.WitnessFinding(kind=B.FINDING_COPY, wire=0, row=0, wire_b=0, row_b=1 << 40),
           B.WitnessFinding(kind=0), B.WitnessFinding(kind=3)]
    for f in bad:
        cf = f._c()
        buf = ctypes.create_string_buffer(b"x" * 64, 64)
        assert lib.qpgpu_witness_finding_format(pack.ctypes.data, pack.size, ctypes.byref(cf), buf, 64) == -1, f
        assert buf.raw[0] == 0
        with pytest.raises(pkg.QpGpuError):
            B.format_finding(pack, f)
    ok = B.WitnessFinding(kind=B.FINDING_GATE, gate=8, constraint=0, row=0)._c()
    buf = ctypes.create_string_buffer(64)
    assert lib.qpgpu_witness_finding_format(pack.ctypes.data, 10, ctypes.byref(ok), buf, 64) == -1          # a cut pack
    assert lib.qpgpu_witness_finding_format(None, 0, ctypes.byref(ok), buf, 64) == -1
    assert lib.qpgpu_witness_finding_format(pack.ctypes.data, pack.size, None, buf, 64) == -1
    assert lib.qpgpu_witness_finding_format(pack.ctypes.data, pack.size, ctypes.byref(ok), None, 64) == -1
    assert lib.qpgpu_witness_finding_format(pack.ctypes.data, pack.size, ctypes.byref(ok), buf, 0) == -1


def test_finding_layout_and_null_handle(pkg):
    B = pkg.binding
    F = B._WitnessFinding
    assert ctypes.sizeof(F) == 56
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == [
        ("kind", 0, 4), ("gate", 4, 4), ("constraint", 8, 4), ("wire", 12, 4), ("wire_b", 16, 4), ("reserved", 20, 4),
        ("row", 24, 8), ("row_b", 32, 8), ("value", 40, 8), ("value_b", 48, 8)]
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    assert "enum { QPGPU_FINDING_GATE = 1, QPGPU_FINDING_COPY = 2 };" in hdr and (B.FINDING_GATE, B.FINDING_COPY) == (1, 2)
    lib = pkg.load_library()
    n, rows, copies = ctypes.c_size_t(77), ctypes.c_uint64(77), ctypes.c_uint64(77)
    out = (F * 2)()
    w = np.zeros(4, dtype=np.uint64)
    assert lib.qpgpu_circuit_explain_witness(None, w.ctypes.data, 0, w.ctypes.data, 8, 0, out, 2, ctypes.byref(n), ctypes.byref(rows), ctypes.byref(copies)) == -1
    assert (n.value, rows.value, copies.value) == (77, 77, 77)
    names = B.exported_symbols()
    assert "qpgpu_circuit_explain_witness" in names and "qpgpu_witness_finding_format" in names
    assert callable(pkg.Circuit.explain_witness) and callable(pkg.leaf.LeafCircuit.describe) and callable(pkg.format_finding)


def test_leaf_describe_names_the_logical_targets(pkg):
    """LeafCircuit.describe: a COPY finding's two cells looked up in target_map (a reverse lookup, nothing more)."""
    B = pkg.binding
    lc = pkg.leaf.LeafCircuit()
    nw, R = int(lc.pack[2]), int(lc.pack[3])
    routed = [(i, int(c)) for i, c in enumerate(lc.target_map) if int(c) % nw < R]
    i0, cell = routed[0]
    same = [i for i, c in routed if c == cell]
    other = next(c for i, c in routed if c != cell)
    f = B.WitnessFinding(kind=B.FINDING_COPY, wire=cell % nw, row=cell // nw, value=3, wire_b=other % nw, row_b=other // nw, value_b=4)
    line = lc.describe(f)
    assert line.startswith(B.format_finding(lc.pack, f) + "; cell = logical target")
    assert ", ".join(str(i) for i in same) in line.split("; cell = ")[1].split(";")[0]
    assert "; source = logical target" in line
    g = B.WitnessFinding(kind=B.FINDING_GATE, gate=1, constraint=0, row=0, value=1)
    assert lc.describe(g) == B.format_finding(lc.pack, g)


def test_select_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "explain_select")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tests", "native", "explain_select_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == ["select ok", "edges ok", "constants ok", "explain select: ok"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_one_hot_fold_is_exact_under_sanitizers(tmp_path):
    exe = str(tmp_path / "explain_one_hot_check")
    subprocess.check_call(SAN + [os.path.join(ROOT, "tools", "host_checks", "explain_one_hot_check.cpp"), os.path.join(CSRC, "poseidon_constants.cpp"),
                                 "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "explain one-hot fold: failures 0" in r.stdout and r.stdout.count("one-hot folds compared") == 6 and "runtime error" not in r.stderr
