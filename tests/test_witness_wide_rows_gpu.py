"""The thread-per-row generators of the two hash gates (witness_hash_rows_wide_kernel, csrc/witness_kernels.hip) against the
lane-cooperative ones: QPGPU_WITNESS_WIDE_ROWS=1 sends every separately launched dependency level's PoseidonGate and Poseidon2 gate
rows to the wide kernel, =0 none; a circuit loaded under either must leave the same wire matrix cell for cell, and the oracle's.
Shapes: the dense leaf with all its Poseidon2 rows in one level (hash hints) and spread over the chains (no hints), the second
Poseidon2 wire layout (no swap wires), PoseidonGate rows with the swap wire set and unset (the wrapper's Merkle paths), and hash
rows fed with the field's edge values, loose representatives included."""
import numpy as np
import pytest

import field_vectors as fv
import leaf_cases as lc
from test_poseidon2_gate import KW

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
KNOB = "QPGPU_WITNESS_WIDE_ROWS"


@pytest.fixture(scope="module")
def L(pkg):
    return pkg.leaf


def both_knobs(pkg, gpu, monkeypatch, pack, run):
    """run(circ) on a circuit loaded freshly under the knob at 0 and at 1 (it is read at load); returns the two results. Runs of narrow
    levels keep the cooperative generators whatever the knob says, so they are switched off: every level is a launch of its own."""
    monkeypatch.setenv("QPGPU_WITNESS_FUSE", "0")
    out = []
    for knob in ("0", "1"):
        monkeypatch.setenv(KNOB, knob)
        circ = pkg.Circuit(gpu, pack, max_batch=2)
        try:
            out.append(run(circ))
        finally:
            circ.close()
    monkeypatch.delenv(KNOB)
    return out


@pytest.mark.parametrize("hints", [True, False], ids=["hinted", "plain"])
def test_dense_leaf(pkg, gpu, orc, L, monkeypatch, hints):
    dense = L.LeafCircuit(copies=3)
    sets = [[lc.dummy_inputs(L), lc.test_inputs(L, 0), lc.real_inputs(L, depth=16, seed=9)],
            [lc.real_inputs(L, depth=3), lc.real_inputs(L, depth=11, seed=4), lc.test_inputs(L, 1)]]
    com = [dense.commit(s, hash_hints=hints) for s in sets]
    nw, n = 135, 1 << dense.info["degree_bits"]

    def run(circ):
        d = gpu.alloc(2 * nw * n * 8)
        st = circ.generate_witness_partial_batch_dev(com[0][0], np.stack([c[1] for c in com]), np.stack([c[2] for c in com]), d)
        got = d.download().reshape(2, nw, n)
        d.free(scrub=True)
        return st, got, circ.witness_info()

    (st0, w0, info0), (st1, w1, info1) = both_knobs(pkg, gpu, monkeypatch, dense.pack, run)
    assert st0 == st1 == [0, 0] and info0 == info1
    assert np.array_equal(w0, w1)
    for b in range(2):
        plain = dense.commit(sets[b])
        rc, want, _ = orc.generate_witness(dense.pack, plain[0], plain[1], plain[2])
        assert rc == orc.WIT_OK and np.array_equal(w1[b], want), b
    one = pkg.Circuit(gpu, L.LeafCircuit().pack)
    x = sets[0][2]
    c1 = L.LeafCircuit().commit(x, hash_hints=hints)
    d1 = gpu.alloc(nw * 256 * 8)
    one.generate_witness_partial_dev(c1[0], c1[1], c1[2], d1)
    levels_of_one_copy = one.witness_info()[1]
    one.close(); d1.free(scrub=True)
    # the copies' rows share their levels: as deep as ONE copy (14 levels hinted, where every Poseidon2 row of the circuit, 183 of them,
    # is a generator of one level; 120 along the hash chains without hints)
    assert info1[1] == levels_of_one_copy == (14 if hints else 120), (info1, levels_of_one_copy)


def test_a_wrong_hint_fails_its_witness_alone_under_the_wide_kernel(pkg, gpu, L, monkeypatch):
    dense = L.LeafCircuit(copies=3)
    xs = [lc.dummy_inputs(L), lc.test_inputs(L, 0), lc.real_inputs(L, depth=5, seed=6)]
    cells, values, pis = dense.commit(xs, hash_hints=True)
    vals = np.stack([values, values]); vals[1, 3 * 299 - 16 + 796 + 77] ^= np.uint64(1)       # a sponge state of copy 1
    monkeypatch.setenv(KNOB, "1")
    circ = pkg.Circuit(gpu, dense.pack, max_batch=2)
    nw, n = 135, 1 << dense.info["degree_bits"]
    d = gpu.alloc(2 * nw * n * 8)
    try:
        assert circ.generate_witness_partial_batch_dev(cells, vals, np.stack([pis, pis]), d) == [0, -4]
        assert "witness 1" in gpu.last_error() and "set twice with different values" in gpu.last_error()
    finally:
        circ.close(); d.free(scrub=True)


def synth_run(gpu, part, pis, shape):
    def run(circ):
        d_w = gpu.to_device(np.stack([part, part]))
        circ.generate_witness_dev(d_w, np.stack([pis, pis]), batch=2)
        out = d_w.download().reshape(2, *shape)
        d_w.free(scrub=True)
        return out
    return run


@pytest.mark.parametrize("alt", [True, False], ids=["layout-without-swap-wires", "default-layout"])
def test_poseidon2_layouts_and_poseidon_rows_of_a_synthetic_circuit(pkg, gpu, monkeypatch, alt):
    """PoseidonGate and Poseidon2 rows in the same levels; the second layout has no swap / delta wires and other columns throughout."""
    pack, wires, pis = pkg.synth_circuit(8, seed=25, ext_arith=True, recursion=True, hints=True, p2_alt_layout=alt, **KW)
    lay = pkg.pack_p2_layout(pack)
    if alt:
        assert lay["w_swap"] == 0xFFFFFFFF and lay["w_input"] == 12 and lay["w_output"] == 0 and lay["w_full0"] == 94, lay
    else:
        assert lay["w_swap"] == 24 and lay["w_delta"] == 25 and lay["w_input"] == 0 and lay["w_full0"] == 29, lay
    assert lay["first_round_wires"] == 0          # (no layout with first-round wires fits 135 wires: 12 + 12 + 48 + 22 + 48 = 142)
    monkeypatch.setenv(KNOB, "0")
    c0 = pkg.Circuit(gpu, pack)
    mask = c0.witness_free_mask(*wires.shape)
    c0.close()
    part = np.where(mask == 1, wires, 0).astype(np.uint64)
    w0, w1 = both_knobs(pkg, gpu, monkeypatch, pack, synth_run(gpu, part, pis, wires.shape))
    assert np.array_equal(w0, w1) and np.array_equal(w1[0], wires) and np.array_equal(w1[1], wires)


@pytest.mark.parametrize("loose", [False, True], ids=["canonical-edges", "loose-representatives"])
def test_edge_values_as_row_inputs(pkg, gpu, monkeypatch, loose):
    """The free input cells of every Poseidon2 site take tests/field_vectors.py's edge set (values at the carry and borrow boundaries
    of the field arithmetic; with `loose` also representatives at and above p), so the rare paths run inside the wide kernel."""
    d = 8
    pack, wires, pis = pkg.synth_circuit(d, seed=23, **KW)
    monkeypatch.setenv(KNOB, "0")
    c0 = pkg.Circuit(gpu, pack)
    mask = c0.witness_free_mask(*wires.shape)
    c0.close()
    part = np.where(mask == 1, wires, 0).astype(np.uint64)
    edges = list(fv.E if loose else fv.E_CANON)
    free = [(c, r) for site in pkg.synth_p2_sites(d, 21, poseidon2=True) for c, r in pkg.p2_site_cells(pack, site)[0] if mask[c, r]]
    assert len(free) >= 32
    for off in range(0, len(edges), len(free)):                  # as many fills as it takes for every edge value to feed a row
        for k, (c, r) in enumerate(free):
            part[c, r] = np.uint64(edges[(off + k) % len(edges)])
        w0, w1 = both_knobs(pkg, gpu, monkeypatch, pack, synth_run(gpu, part, pis, wires.shape))
        assert np.array_equal(w0, w1), off
        assert not np.array_equal(w1[0], wires) and int(w1[0][mask == 0].max()) < P        # everything generated is canonical


@pytest.mark.parametrize("loose", [False, True], ids=["canonical-edges", "loose-representatives"])
def test_edge_values_as_poseidon_gate_row_inputs(pkg, gpu, monkeypatch, loose):
    """The same for the PoseidonGate body of the wide kernel (its MDS layer is the multiplication-free one, the cooperative body's the
    96-bit fold): the free input wires 0..11 of every PoseidonGate row take the edge set."""
    pack, wires, pis = pkg.synth_circuit(8, seed=72, poseidon=True, base_sum=True)
    monkeypatch.setenv(KNOB, "0")
    c0 = pkg.Circuit(gpu, pack)
    mask = c0.witness_free_mask(*wires.shape)
    rows = c0.gate_rows(4)
    c0.close()
    part = np.where(mask == 1, wires, 0).astype(np.uint64)
    free = [(c, int(r)) for r in rows for c in range(12) if mask[c, int(r)]]
    assert len(free) >= 12, len(free)
    edges = list(fv.E if loose else fv.E_CANON)
    for off in range(0, len(edges), len(free)):
        for k, (c, r) in enumerate(free):
            part[c, r] = np.uint64(edges[(off + k) % len(edges)])
        w0, w1 = both_knobs(pkg, gpu, monkeypatch, pack, synth_run(gpu, part, pis, wires.shape))
        assert np.array_equal(w0, w1), off
        assert not np.array_equal(w1[0], wires) and int(w1[0][mask == 0].max()) < P


def test_poseidon_rows_with_the_swap_wire_set_and_unset(pkg, gpu, orc, L, monkeypatch):
    """The two-leaf wrapper: 4 032 PoseidonGate rows, the Merkle paths' rows with swap = the index bit."""
    leaf = L.LeafCircuit()
    lp = L.LeafProver(pkg, gpu, leaf)
    proofs = [lp.prove(x)[0] for x in (lc.real_inputs(L, depth=5, seed=3), lc.test_inputs(L, 1))]
    ver = pkg.Verifier(leaf.pack, circuit=lp.circ)
    w = pkg.recursion.WrapperCircuit(leaf.pack, ver, 2)
    cells, vals, pis = w.commit(proofs)
    nw, n = 135, 1 << w.info["degree_bits"]

    def run(circ):
        d = gpu.alloc(nw * n * 8)
        circ.generate_witness_partial_dev(cells, vals, pis, d)
        got = d.download().reshape(nw, n)
        rows = circ.gate_rows(4)
        d.free(scrub=True)
        return got, rows

    (w0, rows), (w1, _) = both_knobs(pkg, gpu, monkeypatch, w.pack, run)
    swaps = w1[24, rows.astype(np.int64)]
    assert (swaps == 1).any() and (swaps == 0).any()
    assert np.array_equal(w0, w1)
    rc, want, _ = orc.generate_witness(w.pack, cells, vals, pis)
    assert rc == orc.WIT_OK and np.array_equal(w1, want)
    ver.close(); lp.close()
