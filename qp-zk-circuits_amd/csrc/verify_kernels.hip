// verify_kernels.hip — the query rounds of batch verification on gfx950 (qpgpu_verifier_verify_many_device): for every proof of
// a lockstep batch of one circuit, the Merkle paths of the four initial oracles and of every FRI round, the FRI continuation,
// the coset interpolation at beta and the final polynomial. The host verifier's query loop (verifier.cpp: verify_impl) is the
// specification; the transcript, proof of work and quotient identity stay on the host (verify_device.cpp).
//
// Two launches: one thread per opening (proof x query x {4 initial oracles + FRI rounds}) hashes the opened row and climbs its
// path, then one thread per (proof, query) runs the FRI arithmetic and merges the Merkle verdicts into the first failing check of
// the query. Proof bytes are read in place: a one-byte path length precedes every path, so most words of a query round are not
// 8-byte aligned; words are assembled from the two aligned words they straddle (each proof starts on a word and is followed by a
// word of padding).
#include <hip/hip_runtime.h>
#include "merkle.hpp"
#include "poseidon.hpp"
#include "prover_kernels.hpp"
#include "verify_kernels.hpp"

using gl::e2;
using gl::u32;
using gl::u64;

namespace vk {
__constant__ u64 c_poseidon_rc[poseidon::ROUNDS * poseidon::WIDTH];
#define MERKLE_HASH_PLUGS_ONLY
#include "merkle_hash_impl.hpp"

// the little-endian word at byte offset `off` of a word array
__device__ __forceinline__ u64 ld(const u64 *w, u32 off) {
    const u64 *p = w + (off >> 3);
    const u32 sh = (off & 7) * 8;
    const u64 lo = p[0], hi = p[1];
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}
__device__ __forceinline__ e2 ld_ext(const u64 *w, u32 off) { return gl::e2_make(ld(w, off), ld(w, off + 8)); }
__device__ __forceinline__ e2 rec_ext(const u64 *rec, u32 i) { return gl::e2_make(rec[i], rec[i + 1]); }
__device__ __forceinline__ bool same(e2 x, e2 y) { x = gl::e2_canon(x); y = gl::e2_canon(y); return x.a == y.a && x.b == y.b; }
__device__ __forceinline__ u32 bitrev(u32 x, u32 bits) { return __brev(x) >> (32 - bits); }

// blockIdx.y = opening (wave-uniform, so the layout entry is read from the kernel arguments with scalar loads)
template <class Perm>
__global__ void __launch_bounds__(256) merkle_open_kernel(VerifyLayout lay, const u64 *proofs, const u64 *recs, const u64 *cs_cap, u32 nproofs,
                                                          uint8_t *mcodes, const poseidon2::Params *p2) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= (u64)nproofs * lay.nq) return;
    const u32 k = blockIdx.y;
    const u32 pr = (u32)(t / lay.nq), qi = (u32)(t - (u64)pr * lay.nq);
    const u64 *rec = recs + (u64)pr * lay.rec_words;
    uint8_t *out = mcodes + t * lay.n_open + k;
    if (rec[VREC_LIVE] == 0) { *out = 0; return; }
    const VerifyOpening op = lay.op[k];
    const u64 *pw = proofs + (u64)pr * lay.stride_words;
    const u32 row = lay.queries_pos + qi * lay.q_bytes + op.off;
    const u32 plen = (u32)(ld(pw, row + 8 * op.width) & 0xff);
    if (plen > 60) { *out = VQ_ORACLE_PLEN; return; }       // the kind is refined by the FRI kernel (oracle or round)
    if (plen != op.plen) { *out = VQ_ORACLE_PATH; return; }
    u64 index = rec[VREC_BETAS + 2 * (lay.n_open - 4) + qi] >> op.shift;
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
    if (op.width <= 4) {                                        // hash_or_noop: a short row is its own digest
#pragma unroll
        for (u32 i = 0; i < 4; i++) s[i] = i < op.width ? ld(pw, row + 8 * i) : 0;
    } else {
        for (u32 c = 0; c < op.width; c += 8) {                 // hash_n_to_hash_no_pad: overwrite absorption, rate 8
#pragma unroll
            for (u32 i = 0; i < 8; i++)
                if (c + i < op.width) s[i] = ld(pw, row + 8 * (c + i));
            Perm::permute(s, p2);
        }
    }
    u32 at = row + 8 * op.width + 1;
    for (u32 l = 0; l < plen; l++, at += 32) {
        u64 sib[4];
#pragma unroll
        for (int i = 0; i < 4; i++) sib[i] = ld(pw, at + 8 * i);
        const bool right = index & 1;
#pragma unroll
        for (int i = 0; i < 4; i++) { const u64 cur = s[i]; s[i] = right ? sib[i] : cur; s[4 + i] = right ? cur : sib[i]; s[8 + i] = 0; }
        Perm::permute(s, p2);
        index >>= 1;
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 want = op.cap_off == VERIFY_CAP_VERIFIER ? cs_cap[4 * index + i] : pw[(op.cap_off >> 3) + 4 * index + i];   // caps: word offsets
        ok &= s[i] == want;
    }
    *out = ok ? 0 : VQ_ORACLE_PATH;
}

// one thread per (proof, query): fri_combine_initial, the FRI rounds (continuation, coset interpolation at beta), the final
// polynomial; the first failing check of the query in the host verifier's order
__global__ void __launch_bounds__(256) fri_query_kernel(VerifyLayout lay, const u64 *proofs, const u64 *recs, const uint8_t *mcodes, u32 nproofs,
                                                        u32 *qcodes) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= (u64)nproofs * lay.nq) return;
    const u32 pr = (u32)(t / lay.nq), qi = (u32)(t - (u64)pr * lay.nq);
    const u64 *rec = recs + (u64)pr * lay.rec_words;
    if (rec[VREC_LIVE] == 0) { qcodes[t] = 0; return; }
    const uint8_t *mc = mcodes + t * lay.n_open;
    for (u32 o = 0; o < 4; o++)
        if (mc[o]) { qcodes[t] = (mc[o] == VQ_ORACLE_PLEN ? VQ_ORACLE_PLEN : VQ_ORACLE_PATH) << 8 | o; return; }
    const u32 n_rounds = lay.n_open - 4;
    const u64 *pw = proofs + (u64)pr * lay.stride_words;
    const u32 qbase = lay.queries_pos + qi * lay.q_bytes;
    u64 x_index = rec[VREC_BETAS + 2 * n_rounds + qi];
    const e2 alpha = rec_ext(rec, VREC_ALPHA);
    e2 e0 = gl::e2_from(0), e1 = gl::e2_from(0);                // fri_combine_initial: salts are not opened
    for (int o = 3; o >= 0; o--) {
        const u32 row = qbase + lay.op[o].off;
        for (u32 j = lay.polys[o]; j-- > 0;) e0 = gl::e2_add(gl::e2_mul(e0, alpha), gl::e2_from(ld(pw, row + 8 * j)));
    }
    for (u32 j = lay.nch; j-- > 0;) e1 = gl::e2_add(gl::e2_mul(e1, alpha), gl::e2_from(ld(pw, qbase + lay.op[2].off + 8 * j)));
    u64 subgroup_x = gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity(lay.log_lde), bitrev((u32)x_index, lay.log_lde)));
    const e2 sx = gl::e2_from(subgroup_x);
    e2 sum = gl::e2_mul(gl::e2_sub(e0, rec_ext(rec, VREC_RED0)), gl::e2_inv(gl::e2_sub(sx, rec_ext(rec, VREC_ZETA))));
    sum = gl::e2_add(gl::e2_mul(sum, rec_ext(rec, VREC_ALPHA_NCH)),
                     gl::e2_mul(gl::e2_sub(e1, rec_ext(rec, VREC_RED1)), gl::e2_inv(gl::e2_sub(sx, rec_ext(rec, VREC_GZETA)))));
    e2 old_eval = sum;
    for (u32 r = 0; r < n_rounds; r++) {
        const u32 m = mc[4 + r];
        if (m == VQ_ORACLE_PLEN) { qcodes[t] = VQ_ROUND_PLEN << 8 | r; return; }
        const u32 ab = lay.arity_bits[r], arity = 1u << ab;
        const u32 ev = qbase + lay.op[4 + r].off;
        const u32 within = (u32)x_index & (arity - 1);
        if (!same(ld_ext(pw, ev + 16 * within), old_eval)) { qcodes[t] = VQ_ROUND_CONT << 8 | r; return; }
        if (m) { qcodes[t] = VQ_ROUND_PATH << 8 | r; return; }
        // compute_evaluation: the coset's points x_i = start g^i carry the values ev[bitrev(i)]; barycentric form
        //   p(beta) = (beta^n - start^n) / (n start^n) * sum_i y_i x_i / (beta - x_i),  accumulated as one fraction num / den
        const u64 g = gl::root_of_unity(ab);
        const u64 start = gl::mul(subgroup_x, gl::pow(g, arity - bitrev(within, ab)));
        const e2 beta = rec_ext(rec, VREC_BETAS + 2 * r);
        e2 num = gl::e2_from(0), den = gl::e2_from(1), hit = gl::e2_from(0);
        bool at_point = false;
        u64 x = start;
        for (u32 i = 0; i < arity; i++, x = gl::mul(x, g)) {
            const e2 y = ld_ext(pw, ev + 16 * bitrev(i, ab));
            const e2 d = gl::e2_canon(gl::e2_sub(beta, gl::e2_from(x)));
            if (d.a == 0 && d.b == 0) { at_point = true; hit = y; continue; }
            num = gl::e2_add(gl::e2_mul(num, d), gl::e2_mul(gl::e2_scale(y, x), den));
            den = gl::e2_mul(den, d);
        }
        const u64 start_n = gl::pow(start, arity);
        e2 beta_n = beta;
        for (u32 i = 0; i < ab; i++) beta_n = gl::e2_mul(beta_n, beta_n);
        const e2 zb = gl::e2_sub(beta_n, gl::e2_from(start_n));
        const e2 val = gl::e2_scale(gl::e2_mul(gl::e2_mul(zb, num), gl::e2_inv(den)), gl::inv(gl::mul(start_n, arity)));
        old_eval = at_point ? hit : val;
        subgroup_x = gl::pow(subgroup_x, arity);
        x_index >>= ab;
    }
    e2 fe = gl::e2_from(0);
    const e2 sxe = gl::e2_from(subgroup_x);
    for (u32 i = lay.final_n; i-- > 0;) fe = gl::e2_add(gl::e2_mul(fe, sxe), ld_ext(pw, lay.final_off + 16 * i));
    qcodes[t] = same(fe, old_eval) ? 0 : VQ_FINAL << 8;
}

}  // namespace vk

hipError_t verify_upload_constants(const u64 *rc360) {
    return hipMemcpyToSymbol(HIP_SYMBOL(vk::c_poseidon_rc), rc360, sizeof(u64) * poseidon::ROUNDS * poseidon::WIDTH);
}

hipError_t verify_query_rounds(const VerifyLayout &lay, const u64 *proofs, const u64 *recs, const u64 *cs_cap, u32 nproofs, uint8_t *mcodes,
                               u32 *qcodes, const HasherDev &h, hipStream_t st) {
    const u64 n = (u64)nproofs * lay.nq;
    if (n == 0) return hipSuccess;
    const dim3 block(256), grid_m((unsigned)((n + 255) / 256), lay.n_open), grid_f((unsigned)((n + 255) / 256));
    if (h.kind == hasher::POSEIDON2 && h.qp)
        hipLaunchKernelGGL((vk::merkle_open_kernel<vk::Poseidon2QP>), grid_m, block, 0, st, lay, proofs, recs, cs_cap, nproofs, mcodes, h.p2);
    else if (h.kind == hasher::POSEIDON2)
        hipLaunchKernelGGL((vk::merkle_open_kernel<vk::Poseidon2P>), grid_m, block, 0, st, lay, proofs, recs, cs_cap, nproofs, mcodes, h.p2);
    else
        hipLaunchKernelGGL((vk::merkle_open_kernel<vk::PoseidonV1>), grid_m, block, 0, st, lay, proofs, recs, cs_cap, nproofs, mcodes, h.p2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vk::fri_query_kernel, grid_f, block, 0, st, lay, proofs, recs, mcodes, nproofs, qcodes);
    return hipGetLastError();
}
