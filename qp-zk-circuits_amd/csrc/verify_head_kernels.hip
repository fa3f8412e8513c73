// verify_head_kernels.hip — the head of batch verification on gfx950 (qpgpu_verifier_verify_many_device_ex with
// QPGPU_VERIFY_HEAD_ON_DEVICE): canonical check, public-input hash, Fiat-Shamir transcript, proof of work, the vanishing
// polynomial at zeta against Z_H(zeta) * quotient(zeta), the reduced openings and the query indices. verify_head (verifier.cpp)
// is the specification; the query kernels (verify_kernels.hip) read the record these kernels leave in device memory.
//
// Three launches:
//   transcript_kernel  one thread per proof: a dependent chain of permutations (the duplex sponge), state in registers
//   identity_kernel    one thread per (proof, slot), the slot in blockIdx.y so that a wave evaluates one gate type: slot 0 the
//                      permutation argument, slot 1 + g gate g (verify_math.hpp instantiated for gl::e2 — the text the host
//                      verifier and the in-circuit verifier compile), the last slot Z_H(zeta) * quotient(zeta) and the reduced
//                      openings. A slot returns sum_i alpha_k^(index of term i) * term_i per challenge k: the reduction with
//                      alpha is linear in the terms and the field arithmetic is exact, so the sum of the slots is the host's
//                      Horner value whatever the split.
//   verdict_kernel     one thread per proof: adds the slots, compares per challenge (the first failing one is reported)
//
// Words >= p: the circuit digest is absorbed as the pack holds it, unreduced, as on the host (Challenger::observe_raw). Host and
// device run the same permutation text (poseidon.hpp, GL_HD); every primitive under it (gl64.hpp add, sub, mul, reduce96,
// reduce128, add_canonical) is exact modulo p for ANY 64-bit input, and each permutation ends by canonicalising its twelve
// words, so the output words are the same on both sides whatever representative went in. Everything else the transcript
// absorbs has passed the canonical check first.
#include <hip/hip_runtime.h>
#include "merkle.hpp"
#include "poseidon.hpp"
#include "verify_kernels.hpp"

using gl::e2;
using gl::u32;
using gl::u64;

namespace vmath_dev {
__device__ u64 poseidon_rc[poseidon::ROUNDS * poseidon::WIDTH];      // plonky2's ALL_ROUND_CONSTANTS (the PoseidonGate's)
__device__ u64 poseidon_fp[poseidon::FP_WORDS];                      // its fast-partial-round tables
__device__ poseidon2::Params poseidon2_qp;                           // qp-poseidon-core's set (the Poseidon2 gate's)
}  // namespace vmath_dev
#define VMATH_DEVICE_TABLES
#include "verify_math.hpp"

namespace vh {
__constant__ u64 c_poseidon_rc[poseidon::ROUNDS * poseidon::WIDTH];  // the table poseidon::permute takes (hashing form)
#define MERKLE_HASH_PLUGS_ONLY
#include "merkle_hash_impl.hpp"

// the little-endian word at byte offset `off` of a word array (a proof is followed by a word of padding)
__device__ __forceinline__ u64 ld(const u64 *w, u32 off) {
    const u64 *p = w + (off >> 3);
    const u32 sh = (off & 7) * 8;
    const u64 lo = p[0], hi = p[1];
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}
__device__ __forceinline__ e2 rec_ext(const u64 *rec, u32 i) { return gl::e2_make(rec[i], rec[i + 1]); }
__device__ __forceinline__ void put_ext(u64 *rec, u32 i, e2 x) { x = gl::e2_canon(x); rec[i] = x.a; rec[i + 1] = x.b; }
__device__ __forceinline__ bool same(e2 x, e2 y) { x = gl::e2_canon(x); y = gl::e2_canon(y); return x.a == y.a && x.b == y.b; }

// The duplex sponge of challenger.hpp with the buffers folded into the state: the host copies its input buffer over
// state[0..n_in) right before a permutation and reads challenges from a copy of state[0..8) taken right after one, and an
// observation discards what is left of that copy — so writing an observed word straight to state[n_in] and reading a
// challenge straight from state[n_out - 1] gives the same words. The state stays in registers: the rate word is chosen by
// compares, not by an address (n_in and n_out are the same for every proof of the batch, the layout being one).
template <class Perm>
struct Sponge {
    u64 st[12];
    int n_in, n_out;
    const poseidon2::Params *p2;
    __device__ __forceinline__ void init(const poseidon2::Params *p) {
        p2 = p; n_in = 0; n_out = 0;
#pragma unroll
        for (int i = 0; i < 12; i++) st[i] = 0;
    }
    __device__ __forceinline__ void duplex() { n_in = 0; Perm::permute(st, p2); n_out = 8; }
    __device__ __forceinline__ void observe(u64 x) {
        n_out = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = i == n_in ? x : st[i];
        if (++n_in == 8) duplex();
    }
    __device__ __forceinline__ u64 get() {
        if (n_in > 0 || n_out == 0) duplex();
        --n_out;
        u64 r = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) r = i == n_out ? st[i] : r;
        return r;
    }
    __device__ __forceinline__ e2 get_ext() { const u64 a = get(), b = get(); return gl::e2_make(a, b); }
};

template <class Perm>
__global__ void __launch_bounds__(64) transcript_kernel(VerifyLayout lay, HeadLayout hl, const u64 *proofs, u64 *recs, u64 *hrecs, u32 nproofs,
                                                        const poseidon2::Params *p2) {
    const u32 pr = blockIdx.x * blockDim.x + threadIdx.x;
    if (pr >= nproofs) return;
    u64 *rec = recs + (u64)pr * lay.rec_words, *hrec = hrecs + (u64)pr * hl.hrec_words;
    hrec[HREC_CODE] = 0;
    if (rec[VREC_LIVE] == 0) return;
    const u64 *pw = proofs + (u64)pr * lay.stride_words;

    // ---- canonical check of every word the head reads: all before the query rounds, all from the final polynomial on ----
    bool canonical = true;
    for (u32 i = 0; i < lay.queries_pos / 8; i++) canonical &= pw[i] < gl::P;
    for (u32 off = lay.final_off; off < hl.total; off += 8) canonical &= ld(pw, off) < gl::P;
    if (!canonical) { hrec[HREC_CODE] = VH_NONCANONICAL << 8; rec[VREC_LIVE] = 0; return; }

    // ---- hash_no_pad of the public inputs ----
    Sponge<Perm> sp;
    sp.init(p2);
    for (u32 i = 0; i < hl.n_pis; i += 8) {
#pragma unroll
        for (u32 k = 0; k < 8; k++)
            if (i + k < hl.n_pis) sp.st[k] = ld(pw, hl.pis_pos + 8 * (i + k));
        Perm::permute(sp.st, p2);
    }
    u64 pih[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { pih[i] = gl::canon(sp.st[i]); hrec[HREC_PIH + i] = pih[i]; }

    // ---- the transcript, in the prover's order ----
    sp.init(p2);
    for (int i = 0; i < 4; i++) sp.observe(hl.digest[i]);          // unreduced, as the pack holds it
    for (int i = 0; i < 4; i++) sp.observe(pih[i]);
    const u32 cw = hl.cap_words, nch = lay.nch;
    for (u32 i = 0; i < cw; i++) sp.observe(pw[i]);                 // wires cap
    for (u32 k = 0; k < nch; k++) hrec[HREC_BETAS + k] = sp.get();
    for (u32 k = 0; k < nch; k++) hrec[HREC_GAMMAS + k] = sp.get();
    for (u32 i = 0; i < cw; i++) sp.observe(pw[cw + i]);            // Zs / partial products cap
    for (u32 k = 0; k < nch; k++) hrec[HREC_ALPHAS + k] = sp.get();
    for (u32 i = 0; i < cw; i++) sp.observe(pw[2 * cw + i]);        // quotient cap
    const e2 zeta = sp.get_ext();
    // openings: constants and sigmas, wires, zs, partial products, quotient, zs_next (byte order: ..., zs, zs_next, pp, quotient)
    const int order[7] = {0, 1, 2, 3, 5, 6, 4};
    for (int v = 0; v < 7; v++) {
        const u64 *x = pw + hl.open_pos[order[v]] / 8;
        for (u32 i = 0; i < 2 * hl.open_cnt[order[v]]; i++) sp.observe(x[i]);
    }
    const e2 fri_alpha = sp.get_ext();
    for (u32 r = 0; r < hl.n_rounds; r++) {
        const u64 *cap = pw + hl.fri_caps_pos / 8 + r * cw;
        for (u32 i = 0; i < cw; i++) sp.observe(cap[i]);
        put_ext(rec, VREC_BETAS + 2 * r, sp.get_ext());
    }
    for (u32 i = 0; i < 2 * lay.final_n; i++) sp.observe(ld(pw, lay.final_off + 8 * i));
    sp.observe(ld(pw, hl.pow_pos));
    const u64 pow_response = sp.get();
    if (hl.pow_bits && (pow_response >> (64 - hl.pow_bits)) != 0) { hrec[HREC_CODE] = VH_POW << 8; rec[VREC_LIVE] = 0; return; }
    if (hl.pack_bad) { hrec[HREC_CODE] = VH_PACK << 8; rec[VREC_LIVE] = 0; return; }

    put_ext(rec, VREC_ZETA, zeta);
    put_ext(rec, VREC_GZETA, gl::e2_scale(zeta, gl::root_of_unity(hl.degree_bits)));
    put_ext(rec, VREC_ALPHA, fri_alpha);
    put_ext(rec, VREC_ALPHA_NCH, gl::e2_pow(fri_alpha, nch));
    const u64 mask = ((u64)1 << lay.log_lde) - 1;                   // the query rounds do not touch the transcript
    for (u32 q = 0; q < lay.nq; q++) rec[VREC_BETAS + 2 * hl.n_rounds + q] = sp.get() & mask;
}

// a gate's constraints as they arrive: constraint i of the gate is term gate_term0 + i, weighted filter * alpha_k^(gate_term0 + i)
struct GateSinkState { e2 acc[4]; u64 pw[4], alpha[4]; e2 filter; u32 nch; };
struct GateSinkRef {
    GateSinkState *s;
    __device__ __forceinline__ void operator=(e2 v) const {
        const e2 t = gl::e2_mul(s->filter, v);
        for (u32 k = 0; k < s->nch; k++) {
            s->acc[k] = gl::e2_add(s->acc[k], gl::e2_scale(t, s->pw[k]));
            s->pw[k] = gl::mul(s->pw[k], s->alpha[k]);
        }
    }
};
struct GateSink {
    GateSinkState *s;
    __device__ __forceinline__ GateSinkRef operator[](size_t) const { return GateSinkRef{s}; }   // written in increasing order, once each
};

__global__ void __launch_bounds__(64) identity_kernel(VerifyLayout lay, HeadLayout hl, const u64 *proofs, u64 *recs, const u64 *hrecs,
                                                      const u64 *table, u64 *partials, u32 nproofs) {
    const u32 pr = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y;
    if (pr >= nproofs) return;
    u64 *rec = recs + (u64)pr * lay.rec_words;
    const u64 *hrec = hrecs + (u64)pr * hl.hrec_words;
    if (rec[VREC_LIVE] == 0) return;
    const u64 *pw = proofs + (u64)pr * lay.stride_words;
    const u32 nch = lay.nch;
    const e2 *o_cs = (const e2 *)(pw + hl.open_pos[0] / 8), *o_w = (const e2 *)(pw + hl.open_pos[2] / 8), *o_zs = (const e2 *)(pw + hl.open_pos[3] / 8),
             *o_zn = (const e2 *)(pw + hl.open_pos[4] / 8), *o_pp = (const e2 *)(pw + hl.open_pos[5] / 8), *o_q = (const e2 *)(pw + hl.open_pos[6] / 8);
    const GateInfo *gates = (const GateInfo *)table;
    const u64 *k_is = table + 8 * (u64)hl.n_gates;
    const e2 zeta = rec_ext(rec, VREC_ZETA);
    e2 acc[4];
    for (int k = 0; k < 4; k++) acc[k] = gl::e2_from(0);

    if (slot == 0) {                                                // Z(1) = 1 and the partial-product chunks
        e2 zeta_n = zeta;
        for (u32 i = 0; i < hl.degree_bits; i++) zeta_n = zeta_n * zeta_n;
        const e2 one = gl::e2_from(1), zh = zeta_n - one;
        const e2 l0 = zh * gl::e2_inv(gl::scale(zeta - one, (u64)1 << hl.degree_bits));
        const u32 nchunks = hl.num_pp + 1, sig0 = hl.num_selectors + hl.num_constants;
        for (u32 k = 0; k < nch; k++) {                             // challenge whose alpha reduces
            const u64 alpha = hrec[HREC_ALPHAS + k];
            u64 p = 1;
            e2 a = gl::e2_from(0);
            for (u32 j = 0; j < nch; j++, p = gl::mul(p, alpha)) a = a + gl::scale(l0 * (o_zs[j] - one), p);
            for (u32 j = 0; j < nch; j++) {
                const e2 beta = gl::e2_from(hrec[HREC_BETAS + j]), gamma = gl::e2_from(hrec[HREC_GAMMAS + j]), zeta_beta = zeta * beta;
                for (u32 cc = 0; cc < nchunks; cc++, p = gl::mul(p, alpha)) {
                    const e2 prev = cc == 0 ? o_zs[j] : o_pp[j * hl.num_pp + cc - 1], next = cc == nchunks - 1 ? o_zn[j] : o_pp[j * hl.num_pp + cc];
                    const u32 lo = cc * hl.qdf, hi = min((cc + 1) * hl.qdf, hl.num_routed);
                    a = a + gl::scale(vmath::partial_product_term(prev, next, zeta_beta, beta, gamma, k_is, o_w, o_cs + sig0, lo, hi), p);
                }
            }
            acc[k] = a;
        }
    } else if (slot <= hl.n_gates) {                                // one gate's filtered constraints
        const u32 gi = slot - 1;
        const GateInfo g = gates[gi];
        if (g.num_constraints) {
            GateSinkState s;
            s.nch = nch;
            for (u32 k = 0; k < nch; k++) { s.acc[k] = gl::e2_from(0); s.alpha[k] = hrec[HREC_ALPHAS + k]; s.pw[k] = gl::pow(s.alpha[k], hl.gate_term0); }
            s.filter = vmath::gate_filter(g, (u64)gi, o_cs[g.selector_index], gl::e2_from(1), (u64)hl.num_selectors);
            e2 pih[4];
            for (int i = 0; i < 4; i++) pih[i] = gl::e2_from(hrec[HREC_PIH + i]);
            vmath::gate_constraints_to(g, hl.p2, o_cs + hl.num_selectors, o_w, pih, GateSink{&s});
            for (u32 k = 0; k < nch; k++) acc[k] = s.acc[k];
        }
    } else {                                                        // Z_H(zeta) * quotient(zeta), and the reduced openings
        e2 zeta_n = zeta;
        for (u32 i = 0; i < hl.degree_bits; i++) zeta_n = zeta_n * zeta_n;
        const e2 zh = zeta_n - gl::e2_from(1);
        for (u32 k = 0; k < nch; k++) {
            e2 qv = gl::e2_from(0);
            for (u32 j = hl.qdf; j-- > 0;) qv = qv * zeta_n + o_q[k * hl.qdf + j];
            acc[k] = zh * qv;
        }
        const e2 fri_alpha = rec_ext(rec, VREC_ALPHA);
        e2 red0 = gl::e2_from(0), red1 = gl::e2_from(0);            // batch 0 in oracle order (constants and sigmas, wires, zs, pp, quotient)
        const int parts[5] = {0, 2, 3, 5, 6};
        for (int p = 5; p-- > 0;) {
            const e2 *x = (const e2 *)(pw + hl.open_pos[parts[p]] / 8);
            const u32 cnt = hl.open_cnt[parts[p]] + (p == 0 ? hl.open_cnt[1] : 0);
            for (u32 j = cnt; j-- > 0;) red0 = red0 * fri_alpha + x[j];
        }
        for (u32 j = nch; j-- > 0;) red1 = red1 * fri_alpha + o_zn[j];
        put_ext(rec, VREC_RED0, red0);
        put_ext(rec, VREC_RED1, red1);
    }
    u64 *out = partials + ((u64)pr * hl.n_slots + slot) * VERIFY_PARTIAL_WORDS;
    for (u32 k = 0; k < nch; k++) put_ext(out, 2 * k, acc[k]);
}

__global__ void __launch_bounds__(64) verdict_kernel(VerifyLayout lay, HeadLayout hl, u64 *recs, const u64 *hrecs, const u64 *partials, u32 *hcodes,
                                                     u32 nproofs) {
    const u32 pr = blockIdx.x * blockDim.x + threadIdx.x;
    if (pr >= nproofs) return;
    u64 *rec = recs + (u64)pr * lay.rec_words;
    u32 code = (u32)hrecs[(u64)pr * hl.hrec_words + HREC_CODE];
    if (code == 0 && rec[VREC_LIVE] != 0) {
        const u64 *part = partials + (u64)pr * hl.n_slots * VERIFY_PARTIAL_WORDS;
        for (u32 k = 0; k < lay.nch && code == 0; k++) {
            e2 van = gl::e2_from(0);
            for (u32 s = 0; s + 1 < hl.n_slots; s++) van = van + rec_ext(part + (u64)s * VERIFY_PARTIAL_WORDS, 2 * k);
            if (!same(van, rec_ext(part + (u64)(hl.n_slots - 1) * VERIFY_PARTIAL_WORDS, 2 * k))) code = VH_QUOTIENT << 8 | k;
        }
        if (code) rec[VREC_LIVE] = 0;
    }
    hcodes[pr] = code;
}

}  // namespace vh

hipError_t verify_head_upload_constants(const u64 *rc360) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(vh::c_poseidon_rc), rc360, sizeof(u64) * poseidon::ROUNDS * poseidon::WIDTH);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(vmath_dev::poseidon_rc), poseidon::host_round_constants(), sizeof(u64) * poseidon::ROUNDS * poseidon::WIDTH);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(vmath_dev::poseidon_fp), poseidon::host_fast_partial(), sizeof(u64) * poseidon::FP_WORDS);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(vmath_dev::poseidon2_qp), &poseidon2::qp_params(), sizeof(poseidon2::Params));
    return e;
}

hipError_t verify_head_transcript(const VerifyLayout &lay, const HeadLayout &hl, const u64 *proofs, u64 *recs, u64 *hrecs, u32 nproofs,
                                  const HasherDev &h, hipStream_t st) {
    if (nproofs == 0) return hipSuccess;
    const dim3 block(64), grid((nproofs + 63) / 64);
    if (h.kind == hasher::POSEIDON2 && h.qp)
        hipLaunchKernelGGL((vh::transcript_kernel<vh::Poseidon2QP>), grid, block, 0, st, lay, hl, proofs, recs, hrecs, nproofs, h.p2);
    else if (h.kind == hasher::POSEIDON2)
        hipLaunchKernelGGL((vh::transcript_kernel<vh::Poseidon2P>), grid, block, 0, st, lay, hl, proofs, recs, hrecs, nproofs, h.p2);
    else
        hipLaunchKernelGGL((vh::transcript_kernel<vh::PoseidonV1>), grid, block, 0, st, lay, hl, proofs, recs, hrecs, nproofs, h.p2);
    return hipGetLastError();
}

hipError_t verify_head_identity(const VerifyLayout &lay, const HeadLayout &hl, const u64 *proofs, u64 *recs, const u64 *hrecs, const u64 *table,
                                u64 *partials, u32 nproofs, hipStream_t st) {
    if (nproofs == 0) return hipSuccess;
    hipLaunchKernelGGL(vh::identity_kernel, dim3((nproofs + 63) / 64, hl.n_slots), dim3(64), 0, st, lay, hl, proofs, recs, hrecs, table, partials, nproofs);
    return hipGetLastError();
}

hipError_t verify_head_verdict(const VerifyLayout &lay, const HeadLayout &hl, u64 *recs, const u64 *hrecs, const u64 *partials, u32 *hcodes,
                               u32 nproofs, hipStream_t st) {
    if (nproofs == 0) return hipSuccess;
    hipLaunchKernelGGL(vh::verdict_kernel, dim3((nproofs + 63) / 64), dim3(64), 0, st, lay, hl, recs, hrecs, partials, hcodes, nproofs);
    return hipGetLastError();
}
