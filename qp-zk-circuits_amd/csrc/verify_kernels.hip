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

#include "verify_dev.hpp"     // ld, hash_row, climb_path, coset_interpolate, final_poly_at: shared with fri_verify_kernels.hip

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
    hash_row<Perm>(s, pw, row, op.width, p2);
    climb_path<Perm>(s, pw, row + 8 * op.width + 1, plen, index, p2);
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
        old_eval = coset_interpolate(pw, ev, ab, within, subgroup_x, rec_ext(rec, VREC_BETAS + 2 * r));
        subgroup_x = gl::pow(subgroup_x, arity);
        x_index >>= ab;
    }
    const e2 fe = final_poly_at(pw, lay.final_off, lay.final_n, subgroup_x);
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
