"""Coset LDEs at every valid rate_bits (3..8): the shapes the pruned full-size plan cannot take run as 2^r independent 2^d-point
coset transforms with the cosets on the grid (csrc/ntt_plan.cpp lde_coset_run; the ntt_pass_coset kernels; the column-resident
kernel at rate_bits above 3). Words against the CPU oracle's coset_fft of the zero-padded column, in leaf and in natural order.

Before the decomposition, qpgpu_lde_batch_dev answered QPGPU_EINVAL for (d, r) = (3, 8), (4, 7), (5, 8), (6, 8) ("input shorter
than one pass-1 row"), and for (13, 8), (14, 7), (19, 4) ("the input must be at least 1/8 of the output"); qpgpu_oracle_commit_batch
refused (14, 7) as well ("rate_bits <= 3 above 2^20"). (11, 5) and the route pins ran before and still give the same words."""
import ctypes

import numpy as np
import pytest

from test_ntt_gpu import MULT_GEN, P, bitrev_perm
from test_ntt_lde_column_gpu import gpu_lde, oracle_lde

pytestmark = pytest.mark.gpu


def edge_columns(log_n, batch, seed):
    """Random columns; with more than one, the edge inputs in front: zeros, p - 1, the first and the last coefficient alone."""
    n = 1 << log_n
    a = np.random.default_rng(seed).integers(0, P, (batch, n), dtype=np.uint64)
    first = np.zeros(n, dtype=np.uint64); first[0] = 1
    last = np.zeros(n, dtype=np.uint64); last[-1] = P - 2
    edges = [np.zeros(n, dtype=np.uint64), np.full(n, P - 1, dtype=np.uint64), first, last]
    for i, e in enumerate(edges[: max(0, batch - 1)]):     # a single column stays random
        a[i] = e
    return a


# (d, r, columns): the table of the routes. Single pass with cosets, d <= 10; the column kernel at high rate (8 columns: the
# XCD-aware workgroup order; 3: the plain one); two passes with cosets, d >= 14.
SHAPES = [(3, 8, 1), (3, 8, 5), (4, 7, 1), (4, 7, 5), (5, 8, 1), (5, 8, 5), (6, 8, 1), (6, 8, 5),
          (11, 5, 8), (13, 8, 3), (14, 7, 2), (19, 4, 1)]
# shapes that worked before and keep their route
PINS = [(13, 3, 1), (14, 3, 1), (12, 8, 1), (10, 3, 1), (20, 3, 1)]

_cache = {}


def case(orc, d, r, cols):
    """(coefficients, the oracle's LDE in natural order), computed once per shape and never written to."""
    key = (d, r, cols)
    if key not in _cache:
        a = edge_columns(d, cols, 9000 + 100 * d + 10 * r + cols)
        want = oracle_lde(orc, a, d, r)
        a.setflags(write=False); want.setflags(write=False)
        _cache[key] = (a, want)
    return _cache[key]


@pytest.mark.parametrize("d,r,cols", SHAPES + PINS)
def test_lde_words_equal_the_oracle_in_both_orders(gpu, orc, d, r, cols):
    a, want = case(orc, d, r, cols)
    leaf = gpu_lde(gpu, a, d, r, bitrev=True)
    assert int(leaf.max()) < P
    assert np.array_equal(leaf, want[:, bitrev_perm(d + r)])
    nat = gpu_lde(gpu, a, d, r, bitrev=False)
    assert np.array_equal(nat, want)


def test_block_k_of_the_lde_is_the_transform_on_shift_g_w_k(gpu, orc):
    """The identity the decomposition rests on, against the oracle alone and then the device: points k + 2^r t of the natural-order
    LDE are the 2^d-point coset transform with shift g w_(d+r)^k."""
    d, r = 3, 8
    a, want = case(orc, d, r, 1)
    w = orc.pow(7277203076849721926, 1 << (32 - d - r))     # POWER_OF_TWO_GENERATOR^(2^(32 - (d + r))): the primitive 2^(d+r)-th root
    nat = gpu_lde(gpu, a, d, r, bitrev=False)
    for k in (0, 1, 77, 255):
        shift = MULT_GEN * orc.pow(w, k) % P
        sub = np.asarray(orc.coset_fft(np.ascontiguousarray(a[0]), d, shift), dtype=np.uint64)
        assert np.array_equal(want[0, k::1 << r], sub), k
        assert np.array_equal(nat[0, k::1 << r], sub), k


def test_other_coset_shift(gpu, orc):
    """FRI's folded layers use powers of the generator as shifts: the per-coset scale tables are per shift."""
    shift = orc.pow(MULT_GEN, 16)
    for d, r in ((5, 8), (14, 7)):
        a = edge_columns(d, 2, 31 + d)
        want = oracle_lde(orc, a, d, r, shift)
        assert np.array_equal(gpu_lde(gpu, a, d, r, shift=shift), want[:, bitrev_perm(d + r)])
        assert np.array_equal(gpu_lde(gpu, a, d, r, bitrev=False, shift=shift), want)


def resident_lde(pkg, gpu, o, batch):
    """The oracle's resident LDE, per proof: [batch][num_polys][2^(d + r)] read through qpgpu_oracle_device_ptrs / _strides."""
    d_lde = ctypes.c_void_p()
    gpu._check(gpu.lib.qpgpu_oracle_device_ptrs(o.h, None, ctypes.byref(d_lde), None))
    stride = o.strides()[1]
    words = o.num_polys << (o.degree_bits + o.rate_bits)
    assert stride >= words
    out = np.empty((batch, words), dtype=np.uint64)
    for b in range(batch):
        gpu._check(gpu.lib.qpgpu_memcpy_d2h(gpu.ctx, out[b].ctypes.data, ctypes.c_void_p(d_lde.value + 8 * b * stride), out[b].nbytes))
    return out.reshape(batch, o.num_polys, -1)


@pytest.mark.parametrize("d,r,cols", [(5, 8, 5), (14, 7, 2)])
@pytest.mark.parametrize("form", ["back_to_back", "gathered"])
def test_lockstep_commit_batch_lde_per_proof(pkg, gpu, orc, d, r, cols, form):
    """Three proofs' coefficient matrices through qpgpu_oracle_commit_batch, back to back in one allocation (used in place) and as
    separate allocations (gathered): each proof's resident LDE equals the oracle's words in leaf order."""
    batch = 3
    a0, want0 = case(orc, d, r, cols)
    mats = [a0] + [edge_columns(d, cols, 40 + 7 * b + d) for b in range(1, batch)]
    wants = [want0] + [oracle_lde(orc, m, d, r) for m in mats[1:]]
    bufs = []
    if form == "back_to_back":
        whole = gpu.to_device(np.ascontiguousarray(np.stack(mats)))
        bufs.append(whole)
        polys = [(whole.ptr + b * mats[0].nbytes, cols, 1 << d) for b in range(batch)]
    else:
        for m in mats:
            bufs.append(gpu.to_device(np.ascontiguousarray(m)))
        polys = [(x.ptr, cols, 1 << d) for x in bufs]
    o = pkg.PolyOracle.commit_batch(gpu, polys, rate_bits=r, cap_height=4, coeffs=True)
    try:
        got = resident_lde(pkg, gpu, o, batch)
        perm = bitrev_perm(d + r)
        for b in range(batch):
            assert np.array_equal(got[b], wants[b][:, perm]), b
    finally:
        o.close()
        for x in bufs:
            x.free()
