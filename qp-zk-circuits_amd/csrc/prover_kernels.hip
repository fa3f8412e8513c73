// prover_kernels.hip — stages s5 and s7..s11 of plonky2's prove() as gfx950 kernels (s6, the quotient: quotient_kernels.hip).
//
// Replaces, inside qp-plonky2 1.5.5 `plonk::prover::prove` (reference call site
// wormhole/prover/src/lib.rs:171-175):
//   s5  all_wires_permutation_partial_products   -> pp_rows_kernel, pp_scan_kernel, pp_finish_kernel
//   s6  compute_quotient_polys                   -> quotient_kernels.hip
//   s7  OpeningSet::new (poly evaluation at zeta) -> poly_eval_kernel
//   s8  prove_openings (batch reduce, /(X - z))  -> reduce_polys_kernel, divide_linear_kernel
//   s9  fri_committed_trees (fold)               -> fri_fold_kernel, interleave_ext_kernel
//   s10 fri_proof_of_work                        -> pow_kernel
//   s11 fri_prover_query_rounds (gathers)        -> gather kernels
// Layout: polynomial batches column-major; LDEs in leaf order (slot j = point bitrev(j)), so every
// per-point kernel reads one slot of every column with unit-stride across the wave.
#include <hip/hip_runtime.h>
#include "gl64.hpp"
#include "poseidon.hpp"
#include "prover_kernels.hpp"

using gl::e2;
using gl::u32;
using gl::u64;

namespace {

// ---------------------------------------------------------------- s5
// Row i: quotient chunk products prod_{j in chunk} (w_j + beta k_j x + gamma) / (w_j + beta sigma_j + gamma).
// qcp layout: [challenge][chunk][row]; rowprod: [challenge][row].
__global__ void __launch_bounds__(256) pp_rows_kernel(PpArgs a) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const u32 k = blockIdx.y;
    { const u64 pr = blockIdx.z;   // proof of the batch
      a.wires += pr * a.ps_wires; a.betas += pr * a.ps_small; a.gammas += pr * a.ps_small; a.beta_k_is += pr * a.ps_small;
      a.qcp += pr * a.ps_qcp; a.rowprod += pr * a.ps_rowprod; }
    const u64 beta = a.betas[k], gamma = a.gammas[k];
    const u64 x = a.omega_pows[i];
    const u32 R = a.num_routed, chunk = a.chunk, nchunks = a.nchunks;
    u64 nums[16], dens[16], pref[16];   // nchunks <= 16
    for (u32 cc = 0; cc < nchunks; cc++) {
        u64 pn = 1, pd = 1;
        for (u32 j = cc * chunk; j < (cc + 1) * chunk && j < R; j++) {
            const u64 w = a.wires[(u64)j * a.n + i];
            const u64 sid = gl::mul(a.beta_k_is[k * R + j], x);          // beta * k_j * x
            const u64 ssg = gl::mul(beta, a.sigmas[(u64)j * a.n + i]);   // beta * sigma_j(x)
            pn = gl::mul(pn, gl::add(gl::add(w, sid), gamma));
            pd = gl::mul(pd, gl::add(gl::add(w, ssg), gamma));
        }
        nums[cc] = pn; dens[cc] = pd;
    }
    // Montgomery batch inversion of the chunk denominators
    u64 acc = 1;
    for (u32 cc = 0; cc < nchunks; cc++) { pref[cc] = acc; acc = gl::mul(acc, dens[cc]); }
    u64 inv = gl::inv(acc);
    u64 rowp = 1;
    for (u32 cc = nchunks; cc-- > 0;) {
        const u64 dinv = gl::mul(inv, pref[cc]);
        inv = gl::mul(inv, dens[cc]);
        nums[cc] = gl::mul(nums[cc], dinv);
    }
    for (u32 cc = 0; cc < nchunks; cc++) {
        rowp = gl::mul(rowp, nums[cc]);
        a.qcp[((u64)k * nchunks + cc) * a.n + i] = gl::canon(nums[cc]);
    }
    a.rowprod[(u64)k * a.n + i] = gl::canon(rowp);
}

// Exclusive prefix product over rows (Z(x_0) = 1). One workgroup of 1024 threads per challenge.
__global__ void __launch_bounds__(1024) pp_scan_kernel(const u64 *rowprod, u64 *z_out, u64 n) {
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x, T = blockDim.x;
    const u64 *rp = rowprod + (u64)blockIdx.x * n;
    u64 *z = z_out + (u64)blockIdx.x * n;
    const u64 per = (n + T - 1) / T, lo = (u64)t * per, hi = lo + per < n ? lo + per : n;
    u64 acc = 1;
    for (u64 i = lo; i < hi; i++) acc = gl::mul(acc, rp[i]);
    part[t] = acc;
    __syncthreads();
    for (u32 off = 1; off < T; off <<= 1) {   // inclusive Hillis-Steele scan of the partial products
        u64 v = part[t];
        if (t >= off) v = gl::mul(v, part[t - off]);
        __syncthreads();
        part[t] = v;
        __syncthreads();
    }
    acc = t == 0 ? 1 : part[t - 1];
    for (u64 i = lo; i < hi; i++) { z[i] = gl::canon(acc); acc = gl::mul(acc, rp[i]); }
}

// zs_pp columns: [Z_0..Z_{nch-1}, pp_{0,*}, pp_{1,*}, ...]; pp_{k,c}(x_i) = Z_k(x_i) * prod_{c' <= c} qcp
__global__ void __launch_bounds__(256) pp_finish_kernel(PpArgs a, const u64 *z, u64 *zs_pp, u64 ps_z, u64 ps_zs) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    { const u64 pr = blockIdx.z; a.qcp += pr * a.ps_qcp; z += pr * ps_z; zs_pp += pr * ps_zs; }
    const u32 k = blockIdx.y, npp = a.nchunks - 1;
    u64 acc = z[(u64)k * a.n + i];
    zs_pp[(u64)k * a.n + i] = acc;
    for (u32 cc = 0; cc < npp; cc++) {
        acc = gl::mul(acc, a.qcp[((u64)k * a.nchunks + cc) * a.n + i]);
        zs_pp[((u64)a.nch + (u64)k * npp + cc) * a.n + i] = gl::canon(acc);
    }
}

// out[i] = in[i] * shift_inv^i (coset_ifft tail), two-level power table
__global__ void __launch_bounds__(256) scale_powers_kernel(u64 *data, u64 n, u64 ncols, const u64 *pw_lo, const u64 *pw_hi, u32 lo_bits) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 s = gl::mul(pw_hi[i >> lo_bits], pw_lo[i & ((1u << lo_bits) - 1)]);
    for (u64 c = 0; c < ncols; c++) data[c * n + i] = gl::canon(gl::mul(data[c * n + i], s));
}

// ---------------------------------------------------------------- s7
// Evaluate polynomial p (n base-field coefficients) at an extension point. One workgroup per (poly, point).
__global__ void __launch_bounds__(256) poly_eval_kernel(const u64 *coeffs, u64 n, const e2 *points, e2 *out, u64 ps_coeffs, u64 ps_points, u64 ps_out) {
    __shared__ e2 part[256];
    const u32 t = threadIdx.x, T = blockDim.x;
    { const u64 pr = blockIdx.z; coeffs += pr * ps_coeffs; points += pr * ps_points; out += pr * ps_out; }
    const u64 p = blockIdx.x;
    const e2 z = points[blockIdx.y];
    const u64 *f = coeffs + p * n;
    // thread t takes the coefficients t, t + T, t + 2T, ... (unit stride across the wave): Horner in w = z^T, then times z^t.
    // z^(2^b) on the way to w serve as the factors of z^t.
    e2 zp[8];                                   // T = 256 = 2^8
    zp[0] = z;
#pragma unroll
    for (int b = 1; b < 8; b++) zp[b] = gl::e2_mul(zp[b - 1], zp[b - 1]);
    const e2 w = gl::e2_mul(zp[7], zp[7]);
    e2 acc = gl::e2_from(0);
    if (t < n) {
        const u64 terms = (n - t + T - 1) / T;
        for (u64 k = terms; k-- > 0;) acc = gl::e2_add(gl::e2_mul(acc, w), gl::e2_from(f[t + k * T]));
        e2 zt = gl::e2_from(1);
#pragma unroll
        for (int b = 0; b < 8; b++) if ((t >> b) & 1) zt = gl::e2_mul(zt, zp[b]);
        acc = gl::e2_mul(acc, zt);
    }
    part[t] = acc;
    __syncthreads();
    for (u32 off = T >> 1; off > 0; off >>= 1) {
        if (t < off) part[t] = gl::e2_add(part[t], part[t + off]);
        __syncthreads();
    }
    if (t == 0) out[(u64)blockIdx.y * gridDim.x + blockIdx.x] = gl::e2_canon(part[0]);
}

// ---------------------------------------------------------------- s8
// comp[i] = sum_p alpha^p f_p[i] over the listed polynomials (several source batches)
__global__ void __launch_bounds__(256) reduce_polys_kernel(const ReduceArgs a) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const u64 pr = blockIdx.z;
    // the argument block stays read-only: its arrays are indexed by the loop variable, and a modified copy would live in scratch
    const e2 *alpha_pows = a.alpha_pows + pr * a.ps_alpha;
    e2 acc = gl::e2_from(0);
    u32 p = 0;
    for (u32 s = 0; s < a.nsrc; s++) {
        const u64 *base = a.src[s] + pr * a.ps_src[s];
        for (u32 c = 0; c < a.ncols[s]; c++, p++) acc = gl::e2_add(acc, gl::e2_scale(alpha_pows[p], base[(u64)c * a.n + i]));
    }
    a.comp_a[pr * a.ps_comp + i] = gl::canon(acc.a);
    a.comp_b[pr * a.ps_comp + i] = gl::canon(acc.b);
}

// q = comp / (X - z) by synthetic division: b_{i-1} = b_i z + comp_i (from the top), quotient coefficient
// q_{i-1} = b_i ... one workgroup, blocked linear-recurrence scan. final += handled by the caller's mode:
// mode 0: final = q ; mode 1: final = final * shift + q.
__global__ void __launch_bounds__(1024) divide_linear_kernel(const u64 *comp_a, const u64 *comp_b, u64 n, const e2 *zs, const e2 *shifts, int mode, u64 *fin_a, u64 *fin_b,
                                                             u64 ps_comp, u64 ps_fin) {
    __shared__ e2 carry[1024];
    const u32 t = threadIdx.x, T = blockDim.x;
    const u64 pr = blockIdx.x;   // one workgroup per proof of the batch
    comp_a += pr * ps_comp; comp_b += pr * ps_comp; fin_a += pr * ps_fin; fin_b += pr * ps_fin;
    const e2 z = zs[pr], shift = shifts[pr];
    const u64 per = (n + T - 1) / T;
    // thread t owns indices [lo, hi) counted from the TOP: index i = n-1-r
    const u64 rlo = (u64)t * per, rhi = rlo + per < n ? rlo + per : n;
    // local Horner with zero incoming carry
    e2 acc = gl::e2_from(0);
    for (u64 r = rlo; r < rhi; r++) { const u64 i = n - 1 - r; acc = gl::e2_add(gl::e2_mul(acc, z), gl::e2_make(comp_a[i], comp_b[i])); }
    const e2 zper = gl::e2_pow(z, rhi > rlo ? rhi - rlo : 0);
    // sequential-in-log combine: carry_in(t) = value of the recurrence after all elements owned by threads < t
    carry[t] = acc;
    __syncthreads();
    // Hillis-Steele over the affine maps (acc, zper): combined(t) = carry[t - off] * zpow[t] + carry[t]
    __shared__ e2 zp[1024];
    zp[t] = zper;
    __syncthreads();
    for (u32 off = 1; off < T; off <<= 1) {
        e2 c = carry[t], m = zp[t];
        if (t >= off) { c = gl::e2_add(gl::e2_mul(carry[t - off], zp[t]), carry[t]); m = gl::e2_mul(zp[t - off], zp[t]); }
        __syncthreads();
        carry[t] = c; zp[t] = m;
        __syncthreads();
    }
    e2 cin = t == 0 ? gl::e2_from(0) : carry[t - 1];
    // replay with the true incoming value: b after consuming index i is the quotient coefficient q_{i-1}
    acc = cin;
    for (u64 r = rlo; r < rhi; r++) {
        const u64 i = n - 1 - r;
        acc = gl::e2_add(gl::e2_mul(acc, z), gl::e2_make(comp_a[i], comp_b[i]));
        if (i > 0) {
            e2 q = acc;
            if (mode) q = gl::e2_add(gl::e2_mul(gl::e2_make(fin_a[i - 1], fin_b[i - 1]), shift), q);
            fin_a[i - 1] = gl::canon(q.a); fin_b[i - 1] = gl::canon(q.b);
        }
    }
    if (t == 0) {   // the padded top coefficient q_{n-1} = 0
        e2 q = gl::e2_from(0);
        if (mode) q = gl::e2_mul(gl::e2_make(fin_a[n - 1], fin_b[n - 1]), shift);
        fin_a[n - 1] = gl::canon(q.a); fin_b[n - 1] = gl::canon(q.b);
    }
}

// ---------------------------------------------------------------- s9
// rows[j] = (va[j], vb[j]) interleaved: extension values in leaf order -> row-major leaves of 2*arity felts
__global__ void __launch_bounds__(256) interleave_ext_kernel(const u64 *va, const u64 *vb, u64 n, u64 *rows, u64 ps_vals, u64 ps_rows) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    { const u64 pr = blockIdx.z; va += pr * ps_vals; vb += pr * ps_vals; rows += pr * ps_rows; }
    reinterpret_cast<ulonglong2 *>(rows)[i] = make_ulonglong2(va[i], vb[i]);
}
// new[i] = sum_{k < arity} beta^k coeffs[arity*i + k]   (in place is safe: i <= arity*i; done out of place here)
__global__ void __launch_bounds__(256) fri_fold_kernel(const u64 *ca, const u64 *cb, u64 new_n, u32 arity, const e2 *betas, u64 *oa, u64 *ob, u64 ps_in, u64 ps_out) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= new_n) return;
    const u64 pr = blockIdx.z;
    ca += pr * ps_in; cb += pr * ps_in; oa += pr * ps_out; ob += pr * ps_out;
    const e2 beta = betas[pr];
    e2 acc = gl::e2_from(0);
    for (u32 k = arity; k-- > 0;) acc = gl::e2_add(gl::e2_mul(acc, beta), gl::e2_make(ca[(u64)arity * i + k], cb[(u64)arity * i + k]));
    oa[i] = gl::canon(acc.a); ob[i] = gl::canon(acc.b);
}

// ---------------------------------------------------------------- s11
// out[q][c] = cols[c*stride + idx[q]]
__global__ void gather_rows_kernel(const u64 *cols, u64 stride, u32 ncols, const u64 *idx, u32 nq, u64 *out, u64 ps_cols, u64 ps_out) {
    const u32 q = blockIdx.x;
    { const u64 pr = blockIdx.z; cols += pr * ps_cols; idx += pr * nq; out += pr * ps_out; }
    for (u32 c = threadIdx.x; c < ncols; c += blockDim.x) out[(u64)q * ncols + c] = cols[(u64)c * stride + idx[q]];
}
// Merkle authentication paths: out[q][lvl] = digests[level lvl][ (idx[q] >> lvl) ^ 1 ]
__global__ void gather_paths_kernel(const u64 *digests, u64 n_leaves, u32 path_len, const u64 *idx, u32 shift, u64 *out, u32 nq, u64 ps_digests, u64 ps_out) {
    const u32 q = blockIdx.x, t = threadIdx.x;
    { const u64 pr = blockIdx.z; digests += pr * ps_digests; idx += pr * nq; out += pr * ps_out; }
    if (t >= path_len * 4) return;
    const u32 lvl = t >> 2, e = t & 3;
    u64 off = 0, cnt = n_leaves;
    for (u32 l = 0; l < lvl; l++) { off += cnt; cnt >>= 1; }
    const u64 node = ((idx[q] >> shift) >> lvl) ^ 1;
    out[((u64)q * path_len + lvl) * 4 + e] = digests[(off + node) * 4 + e];
}
// out[q][e] = rows[(idx[q] >> shift) * width + e]
__global__ void gather_leaf_rows_kernel(const u64 *rows, u32 width, const u64 *idx, u32 shift, u64 *out, u32 nq, u64 ps_rows, u64 ps_out) {
    const u32 q = blockIdx.x;
    { const u64 pr = blockIdx.z; rows += pr * ps_rows; idx += pr * nq; out += pr * ps_out; }
    for (u32 e = threadIdx.x; e < width; e += blockDim.x) out[(u64)q * width + e] = rows[(idx[q] >> shift) * width + e];
}

// salt columns of a blinded oracle (PolynomialBatch::from_coeffs with blinding: SALT_SIZE = 4 random columns in every
// leaf). The reference draws them from thread_rng, a CSPRNG; every opened leaf publishes its salts, so they must not be
// predictable from one another: ChaCha20 (RFC 8439 block function, 64-bit block counter) keyed with 256 bits per proof
// from the OS entropy source (or from an injected seed, which makes a proof reproducible: SURVEY.md section 0.5).
// Stream layout: nonce = (oracle_index, column); block (leaf >> 1) holds the candidates of leaves 2k and 2k+1, four 64-bit
// words each; a leaf takes its first candidate below p (rejection sampling: uniform on [0, p)).
__device__ __forceinline__ u32 rotl32(u32 x, int k) { return (x << k) | (x >> (32 - k)); }
__device__ __forceinline__ void chacha20_block(const u32 *key, u64 counter, u32 n0, u32 n1, u32 (&out)[16]) {
    u32 x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                 (u32)counter, (u32)(counter >> 32), n0, n1};
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = x[i];
#define QR(a, b, c, d) w[a] += w[b]; w[d] = rotl32(w[d] ^ w[a], 16); w[c] += w[d]; w[b] = rotl32(w[b] ^ w[c], 12); \
                       w[a] += w[b]; w[d] = rotl32(w[d] ^ w[a], 8);  w[c] += w[d]; w[b] = rotl32(w[b] ^ w[c], 7);
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        QR(0, 4, 8, 12) QR(1, 5, 9, 13) QR(2, 6, 10, 14) QR(3, 7, 11, 15)
        QR(0, 5, 10, 15) QR(1, 6, 11, 12) QR(2, 7, 8, 13) QR(3, 4, 9, 14)
    }
#undef QR
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = w[i] + x[i];
}
__global__ void __launch_bounds__(256) salt_kernel(const u32 *keys, u32 oracle_index, u64 lde_n, u64 *out) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= lde_n) return;
    const u32 *key = keys + 8 * blockIdx.z;
    out += (u64)blockIdx.z * 4 * lde_n;
    for (u32 c = 0; c < 4; c++) {
        u32 blk[16];
        chacha20_block(key, j >> 1, oracle_index, c, blk);
        const u32 h = (u32)(j & 1) * 8;
        u64 v = 0;
        bool found = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u64 cand = ((u64)blk[h + 2 * k + 1] << 32) | blk[h + 2 * k];
            if (!found && cand < gl::P) { v = cand; found = true; }
        }
        if (!found) v = (((u64)blk[h + 7] << 32) | blk[h + 6]) - gl::P;   // four rejections in a row: probability 2^-128
        out[(u64)c * lde_n + j] = v;
    }
}

// The same stream for a contiguous range of the leaves (a shard of a coset-sharded oracle): local leaf j is global leaf
// first_leaf + j, whose ChaCha20 position the salt is drawn at, so the shards' slices put together are salt_kernel's output.
// first_leaf is even (a shard holds a power of two of at least two leaves), so a block's two halves stay in one shard. out: [4][count].
__global__ void __launch_bounds__(256) salt_slice_kernel(const u32 *key, u32 oracle_index, u64 first_leaf, u64 count, u64 *out) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= count) return;
    const u64 leaf = first_leaf + j;
    for (u32 c = 0; c < 4; c++) {
        u32 blk[16];
        chacha20_block(key, leaf >> 1, oracle_index, c, blk);
        const u32 h = (u32)(leaf & 1) * 8;
        u64 v = 0;
        bool found = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u64 cand = ((u64)blk[h + 2 * k + 1] << 32) | blk[h + 2 * k];
            if (!found && cand < gl::P) { v = cand; found = true; }
        }
        if (!found) v = (((u64)blk[h + 7] << 32) | blk[h + 6]) - gl::P;
        out[(u64)c * count + j] = v;
    }
}

// RandomValueGenerator on the device (CircuitBuilder::blind's random wires of a zero-knowledge circuit): value j of witness b from
// the ChaCha20 stream of that witness's key, nonce ("BLND", 0); block (j >> 1) holds the candidates of values 2k and 2k+1, the
// first of four below p is taken (uniform on [0, p)). out: [batch][pitch], `count` values each.
__global__ void __launch_bounds__(256) random_felts_kernel(const u32 *keys, u64 count, u64 *out, u64 pitch) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= count) return;
    u32 blk[16];
    chacha20_block(keys + 8 * blockIdx.z, j >> 1, 0x444E4C42u, 0, blk);
    const u32 h = (u32)(j & 1) * 8;
    u64 v = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 cand = ((u64)blk[h + 2 * k + 1] << 32) | blk[h + 2 * k];
        if (!found && cand < gl::P) { v = cand; found = true; }
    }
    if (!found) v = (((u64)blk[h + 7] << 32) | blk[h + 6]) - gl::P;
    out[(u64)blockIdx.z * pitch + j] = v;
}

// x_coset[j] = shift * w^bitrev(j), l0_coset[j] = zh(i) / (n (x - 1))
__global__ void __launch_bounds__(256) coset_tables_kernel(u64 lde_n, u32 log_lde, u64 shift, const u64 *pw_lo, const u64 *pw_hi, u32 lo_bits,
                                                             const u64 *zh, u32 rate, u64 n_field, u64 *x_coset, u64 *l0_coset) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= lde_n) return;
    const u64 i = brev32((u32)j, log_lde);
    const u64 x = gl::canon(gl::mul(shift, gl::mul(pw_hi[i >> lo_bits], pw_lo[i & ((1u << lo_bits) - 1)])));
    x_coset[j] = x;
    l0_coset[j] = gl::canon(gl::mul(zh[i & (rate - 1)], gl::inv(gl::mul(n_field, gl::sub(x, 1)))));
}

}  // namespace

// rows of `width` words, `pitch` words apart -> one dense block (a lockstep batch's per-proof results, so that one
// contiguous copy brings them to the host; a 2D copy is issued by the runtime as one small copy per row)
__global__ void __launch_bounds__(256) pack_rows_kernel(const u64 *src, u64 pitch, u64 width, u64 total, u64 *dst) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u64 r = i / width, c = i - r * width;
    dst[i] = src[r * pitch + c];
}

// the inverse: a dense block of `total / width` rows -> rows `pitch` words apart (one upload for the per-proof tables of a lockstep
// batch instead of one copy launch per proof)
__global__ void __launch_bounds__(256) unpack_rows_kernel(const u64 *src, u64 pitch, u64 width, u64 total, u64 *dst) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u64 r = i / width, c = i - r * width;
    dst[r * pitch + c] = src[i];
}

// dst[0..bytes) = src[0..bytes): the small transfers of the proving path between pinned host memory and device memory (either
// side may be the pinned one: the device reads and writes it in place). 8-byte words when both ends are aligned, bytes otherwise.
__global__ void __launch_bounds__(256) copy_words_kernel(u64 *dst, const u64 *src, u64 words, u64 tail_bytes) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) dst[i] = src[i];
    if (i == 0) for (u64 k = 0; k < tail_bytes; k++) ((unsigned char *)(dst + words))[k] = ((const unsigned char *)(src + words))[k];
}
__global__ void __launch_bounds__(256) copy_bytes_kernel(unsigned char *dst, const unsigned char *src, u64 bytes) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < bytes) dst[i] = src[i];
}

#define LAUNCH_1D(kern, count, threads, st, ...) \
    do { if ((count) > 0) { dim3 b(threads), g((unsigned)(((count) + (threads)-1) / (threads))); hipLaunchKernelGGL(kern, g, b, 0, st, __VA_ARGS__); } } while (0)
// the same over a lockstep batch: grid.z = proof
#define LAUNCH_1D_B(kern, count, threads, nbatch, st, ...) \
    do { if ((count) > 0 && (nbatch) > 0) { dim3 b(threads), g((unsigned)(((count) + (threads)-1) / (threads)), 1, (unsigned)(nbatch)); hipLaunchKernelGGL(kern, g, b, 0, st, __VA_ARGS__); } } while (0)

hipError_t pk_pp_rows(const PpArgs &a, hipStream_t st) {
    dim3 b(256), g((unsigned)((a.n + 255) / 256), a.nch, a.batch);
    hipLaunchKernelGGL(pp_rows_kernel, g, b, 0, st, a);
    return hipGetLastError();
}
hipError_t pk_pp_scan(const u64 *rowprod, u64 *z, u64 n, u32 nch_total, hipStream_t st) {
    hipLaunchKernelGGL(pp_scan_kernel, dim3(nch_total), dim3(1024), 0, st, rowprod, z, n);
    return hipGetLastError();
}
hipError_t pk_pp_finish(const PpArgs &a, const u64 *z, u64 *zs_pp, u64 ps_z, u64 ps_zs, hipStream_t st) {
    dim3 b(256), g((unsigned)((a.n + 255) / 256), a.nch, a.batch);
    hipLaunchKernelGGL(pp_finish_kernel, g, b, 0, st, a, z, zs_pp, ps_z, ps_zs);
    return hipGetLastError();
}
hipError_t pk_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if ((((uintptr_t)dst | (uintptr_t)src) & 7) == 0) {
        const u64 words = bytes / 8, tail = bytes % 8;
        LAUNCH_1D(copy_words_kernel, words ? words : 1, 256, st, (u64 *)dst, (const u64 *)src, words, tail);
    } else {
        LAUNCH_1D(copy_bytes_kernel, bytes, 256, st, (unsigned char *)dst, (const unsigned char *)src, (u64)bytes);
    }
    return hipGetLastError();
}
hipError_t pk_pack_rows(const u64 *src, u64 pitch_words, u64 width_words, u64 rows, u64 *dst, hipStream_t st) {
    LAUNCH_1D(pack_rows_kernel, width_words * rows, 256, st, src, pitch_words, width_words, width_words * rows, dst);
    return hipGetLastError();
}
hipError_t pk_unpack_rows(const u64 *src, u64 pitch_words, u64 width_words, u64 rows, u64 *dst, hipStream_t st) {
    if (width_words * rows == 0) return hipSuccess;
    LAUNCH_1D(unpack_rows_kernel, width_words * rows, 256, st, src, pitch_words, width_words, width_words * rows, dst);
    return hipGetLastError();
}
hipError_t pk_scale_powers(u64 *data, u64 n, u64 ncols, const u64 *pw_lo, const u64 *pw_hi, u32 lo_bits, hipStream_t st) {
    LAUNCH_1D(scale_powers_kernel, n, 256, st, data, n, ncols, pw_lo, pw_hi, lo_bits);
    return hipGetLastError();
}
hipError_t pk_poly_eval(const u64 *coeffs, u64 n, u32 npolys, const e2 *points, u32 npoints, e2 *out, u32 batch, u64 ps_coeffs, u64 ps_points, u64 ps_out, hipStream_t st) {
    if (npolys == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(poly_eval_kernel, dim3(npolys, npoints, batch), dim3(256), 0, st, coeffs, n, points, out, ps_coeffs, ps_points, ps_out);
    return hipGetLastError();
}
hipError_t pk_reduce_polys(const ReduceArgs &a, hipStream_t st) {
    LAUNCH_1D_B(reduce_polys_kernel, a.n, 256, a.batch, st, a);
    return hipGetLastError();
}
hipError_t pk_divide_linear(const u64 *comp_a, const u64 *comp_b, u64 n, const e2 *zs, const e2 *shifts, int mode, u64 *fin_a, u64 *fin_b,
                            u32 batch, u64 ps_comp, u64 ps_fin, hipStream_t st) {
    if (batch == 0) return hipSuccess;
    unsigned threads = n >= 1024 ? 1024 : (n >= 64 ? (unsigned)n : 64);
    hipLaunchKernelGGL(divide_linear_kernel, dim3(batch), dim3(threads), 0, st, comp_a, comp_b, n, zs, shifts, mode, fin_a, fin_b, ps_comp, ps_fin);
    return hipGetLastError();
}
hipError_t pk_interleave_ext(const u64 *va, const u64 *vb, u64 n, u64 *rows, u32 batch, u64 ps_vals, u64 ps_rows, hipStream_t st) {
    LAUNCH_1D_B(interleave_ext_kernel, n, 256, batch, st, va, vb, n, rows, ps_vals, ps_rows);
    return hipGetLastError();
}
hipError_t pk_fri_fold(const u64 *ca, const u64 *cb, u64 new_n, u32 arity, const e2 *betas, u64 *oa, u64 *ob, u32 batch, u64 ps_in, u64 ps_out, hipStream_t st) {
    LAUNCH_1D_B(fri_fold_kernel, new_n, 256, batch, st, ca, cb, new_n, arity, betas, oa, ob, ps_in, ps_out);
    return hipGetLastError();
}
hipError_t pk_gather_rows(const u64 *cols, u64 stride, u32 ncols, const u64 *idx, u32 nq, u64 *out, u32 batch, u64 ps_cols, u64 ps_out, hipStream_t st) {
    if (nq == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(nq, 1, batch), dim3(128), 0, st, cols, stride, ncols, idx, nq, out, ps_cols, ps_out);
    return hipGetLastError();
}
hipError_t pk_gather_paths(const u64 *digests, u64 n_leaves, u32 path_len, const u64 *idx, u32 shift, u32 nq, u64 *out, u32 batch, u64 ps_digests, u64 ps_out, hipStream_t st) {
    if (path_len == 0 || nq == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_paths_kernel, dim3(nq, 1, batch), dim3(256), 0, st, digests, n_leaves, path_len, idx, shift, out, nq, ps_digests, ps_out);
    return hipGetLastError();
}
hipError_t pk_gather_leaf_rows(const u64 *rows, u32 width, const u64 *idx, u32 shift, u32 nq, u64 *out, u32 batch, u64 ps_rows, u64 ps_out, hipStream_t st) {
    if (nq == 0 || batch == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_leaf_rows_kernel, dim3(nq, 1, batch), dim3(64), 0, st, rows, width, idx, shift, out, nq, ps_rows, ps_out);
    return hipGetLastError();
}
hipError_t pk_salt(const u32 *keys, u32 oracle_index, u64 lde_n, u64 *out, u32 batch, hipStream_t st) {
    LAUNCH_1D_B(salt_kernel, lde_n, 256, batch, st, keys, oracle_index, lde_n, out);
    return hipGetLastError();
}
hipError_t pk_salt_slice(const u32 *key, u32 oracle_index, u64 first_leaf, u64 count, u64 *out, hipStream_t st) {
    LAUNCH_1D(salt_slice_kernel, count, 256, st, key, oracle_index, first_leaf, count, out);
    return hipGetLastError();
}
hipError_t pk_random_felts(const u32 *keys, u64 count, u64 *out, u64 pitch, u32 batch, hipStream_t st) {
    if (count == 0 || batch == 0) return hipSuccess;
    LAUNCH_1D_B(random_felts_kernel, count, 256, batch, st, keys, count, out, pitch);
    return hipGetLastError();
}
hipError_t pk_coset_tables(u64 lde_n, u32 log_lde, u64 shift, const u64 *pw_lo, const u64 *pw_hi, u32 lo_bits, const u64 *zh, u32 rate,
                           u64 n_field, u64 *x_coset, u64 *l0_coset, hipStream_t st) {
    LAUNCH_1D(coset_tables_kernel, lde_n, 256, st, lde_n, log_lde, shift, pw_lo, pw_hi, lo_bits, zh, rate, n_field, x_coset, l0_coset);
    return hipGetLastError();
}
