// fri_verify_kernels.hip — the query rounds of qpgpu_fri_verify_many_device on gfx950: for every proof of a batch of one FRI
// instance, the Merkle paths of the initial oracles and of every FRI round, the reduction of the opened rows over the opening
// batches, the FRI continuation, the coset interpolation at beta and the final polynomial. The host loop (fri_verify.cpp:
// friv::query_rounds) is the specification; lengths, canonical elements and the proof of work stay on the host
// (fri_verify_device.cpp). The general form of verify_kernels.hip, with which it shares its device functions (verify_dev.hpp).
//
// Two launches: one thread per opening (proof x query x {initial oracles + FRI rounds}) hashes the opened row and climbs its
// path, then one thread per (proof, query) runs the FRI arithmetic and merges the Merkle verdicts into the first failing check of
// the query. Every offset and every loop bound comes from the layout (FvLayout), none from proof bytes: the path-length byte is
// compared with the layout's and is otherwise not used, and the query indices were range-checked on the host, so no input moves
// a load out of its proof's slot (stride_words, one word of padding included) or a cap read out of its cap.
#include <hip/hip_runtime.h>
#include "fri_verify_kernels.hpp"
#include "merkle.hpp"
#include "poseidon.hpp"
#include "prover_kernels.hpp"
#include "verify_kernels.hpp"

using gl::e2;
using gl::u32;
using gl::u64;

namespace fvk {
__constant__ u64 c_poseidon_rc[poseidon::ROUNDS * poseidon::WIDTH];
#define MERKLE_HASH_PLUGS_ONLY
#include "merkle_hash_impl.hpp"

#include "verify_dev.hpp"

// blockIdx.y = opening (wave-uniform, so the layout entry is read from the kernel arguments with scalar loads)
template <class Perm>
__global__ void __launch_bounds__(256) merkle_open_kernel(FvLayout lay, const u64 *proofs, const u64 *recs, const u64 *caps, u32 nproofs,
                                                          uint8_t *mcodes, const poseidon2::Params *p2) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= (u64)nproofs * lay.nq) return;
    const u32 k = blockIdx.y, n_open = lay.n_oracles + lay.n_rounds;
    const u32 pr = (u32)(t / lay.nq), qi = (u32)(t - (u64)pr * lay.nq);
    const u64 *rec = recs + (u64)pr * lay.rec_words;
    uint8_t *out = mcodes + t * n_open + k;
    if (rec[FREC_LIVE] == 0) { *out = 0; return; }
    const FvOpening op = lay.op[k];
    const u64 *pw = proofs + (u64)pr * lay.stride_words;
    const u32 row = lay.queries_pos + qi * lay.q_bytes + op.off;
    const u32 plen = (u32)(ld(pw, row + 8 * op.width) & 0xff);
    if (plen > 60) { *out = VQ_ORACLE_PLEN; return; }       // the kind is refined by the FRI kernel (oracle or round)
    if (plen != op.plen) { *out = VQ_ORACLE_PATH; return; }
    u64 index = rec[frec_betas(lay.n_batches) + 2 * lay.n_rounds + qi] >> op.shift;      // below 2^(plen + cap height)
    u64 s[12];
    hash_row<Perm>(s, pw, row, op.width, p2);
    climb_path<Perm>(s, pw, row + 8 * op.width + 1, op.plen, index, p2);
    const u64 *cap = op.cap_stride == FV_CAP_IN_PROOF ? pw + op.cap_off : caps + op.cap_off + (u64)pr * op.cap_stride;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) ok &= s[i] == cap[4 * index + i];
    *out = ok ? 0 : VQ_ORACLE_PATH;
}

// one thread per (proof, query): fri_combine_initial over the opening batches, the FRI rounds (continuation, coset interpolation
// at beta), the final polynomial; the first failing check of the query in the host verifier's order
__global__ void __launch_bounds__(256) fri_query_kernel(FvLayout lay, const u64 *proofs, const u64 *recs, const uint8_t *mcodes, u32 nproofs,
                                                        u32 *qcodes) {
    const u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (t >= (u64)nproofs * lay.nq) return;
    const u32 pr = (u32)(t / lay.nq), qi = (u32)(t - (u64)pr * lay.nq);
    const u64 *rec = recs + (u64)pr * lay.rec_words;
    if (rec[FREC_LIVE] == 0) { qcodes[t] = 0; return; }
    const u32 n_oracles = lay.n_oracles, n_rounds = lay.n_rounds;
    const uint8_t *mc = mcodes + t * (n_oracles + n_rounds);
    for (u32 o = 0; o < n_oracles; o++)
        if (mc[o]) { qcodes[t] = (mc[o] == VQ_ORACLE_PLEN ? VQ_ORACLE_PLEN : VQ_ORACLE_PATH) << 8 | o; return; }
    const u64 *pw = proofs + (u64)pr * lay.stride_words;
    const u32 qbase = lay.queries_pos + qi * lay.q_bytes;
    const u32 betas_at = frec_betas(lay.n_batches);
    u64 x_index = rec[betas_at + 2 * n_rounds + qi];
    const e2 alpha = rec_ext(rec, FREC_ALPHA);
    u64 subgroup_x = gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity(lay.log_lde), bitrev((u32)x_index, lay.log_lde)));
    const e2 sx = gl::e2_from(subgroup_x);
    e2 sum = gl::e2_from(0);                                    // fri_combine_initial: salts are not opened
    for (u32 b = 0; b < lay.n_batches; b++) {
        const u32 at = FREC_BATCHES + FREC_BATCH_WORDS * b;     // point, reduced openings, alpha^(polynomials of the batch)
        e2 e = gl::e2_from(0);
        for (u32 k = lay.batch[b].num_ranges; k-- > 0;) {
            const u32 row = qbase + lay.batch[b].ranges[k].row_off;
            for (u32 j = lay.batch[b].ranges[k].count; j-- > 0;) e = gl::e2_add(gl::e2_mul(e, alpha), gl::e2_from(ld(pw, row + 8 * j)));
        }
        sum = gl::e2_add(gl::e2_mul(sum, rec_ext(rec, at + 4)),
                         gl::e2_mul(gl::e2_sub(e, rec_ext(rec, at + 2)), gl::e2_inv(gl::e2_sub(sx, rec_ext(rec, at)))));
    }
    e2 old_eval = sum;
    for (u32 r = 0; r < n_rounds; r++) {
        const u32 m = mc[n_oracles + r];
        if (m == VQ_ORACLE_PLEN) { qcodes[t] = VQ_ROUND_PLEN << 8 | r; return; }
        const u32 ab = lay.arity_bits[r], arity = 1u << ab;
        const u32 ev = qbase + lay.op[n_oracles + r].off;
        const u32 within = (u32)x_index & (arity - 1);
        if (!same(ld_ext(pw, ev + 16 * within), old_eval)) { qcodes[t] = VQ_ROUND_CONT << 8 | r; return; }
        if (m) { qcodes[t] = VQ_ROUND_PATH << 8 | r; return; }
        old_eval = coset_interpolate(pw, ev, ab, within, subgroup_x, rec_ext(rec, betas_at + 2 * r));
        subgroup_x = gl::pow(subgroup_x, arity);
        x_index >>= ab;
    }
    const e2 fe = final_poly_at(pw, lay.final_off, lay.final_n, subgroup_x);
    qcodes[t] = same(fe, old_eval) ? 0 : VQ_FINAL << 8;
}

}  // namespace fvk

hipError_t fri_verify_upload_constants(const u64 *rc360) {
    return hipMemcpyToSymbol(HIP_SYMBOL(fvk::c_poseidon_rc), rc360, sizeof(u64) * poseidon::ROUNDS * poseidon::WIDTH);
}

hipError_t fri_verify_query_rounds(const FvLayout &lay, const u64 *proofs, const u64 *recs, const u64 *caps, u32 nproofs, uint8_t *mcodes,
                                   u32 *qcodes, const HasherDev &h, hipStream_t st) {
    const u64 n = (u64)nproofs * lay.nq;
    if (n == 0) return hipSuccess;
    const dim3 block(256), grid_m((unsigned)((n + 255) / 256), lay.n_oracles + lay.n_rounds), grid_f((unsigned)((n + 255) / 256));
    if (h.kind == hasher::POSEIDON2 && h.qp)
        hipLaunchKernelGGL((fvk::merkle_open_kernel<fvk::Poseidon2QP>), grid_m, block, 0, st, lay, proofs, recs, caps, nproofs, mcodes, h.p2);
    else if (h.kind == hasher::POSEIDON2)
        hipLaunchKernelGGL((fvk::merkle_open_kernel<fvk::Poseidon2P>), grid_m, block, 0, st, lay, proofs, recs, caps, nproofs, mcodes, h.p2);
    else
        hipLaunchKernelGGL((fvk::merkle_open_kernel<fvk::PoseidonV1>), grid_m, block, 0, st, lay, proofs, recs, caps, nproofs, mcodes, h.p2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fvk::fri_query_kernel, grid_f, block, 0, st, lay, proofs, recs, mcodes, nproofs, qcodes);
    return hipGetLastError();
}
