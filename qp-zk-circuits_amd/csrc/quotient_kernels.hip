// quotient_kernels.hip — stage s6 of plonky2's prove() (compute_quotient_polys) as gfx950 kernels, and the witness check that
// runs the same gate kernels on the trace rows.
//   quotient_perm_kernel                                  L_0(x)(Z(x) - 1) and the partial-product checks
//   quotient_gates_kernel                                 every gate but the two hash gates
//   quotient_perm_gates_kernel                            both of the above in one pass over the routed wires, for circuits whose
//                                                         other gates are Constant, PublicInput, Arithmetic and BaseSum<2> only
//   quotient_poseidon_kernel, quotient_poseidon2_kernel   the hash gates, linear layers folded into the alpha weights by
//   quotient_fold_sweep_kernel                            (quotient_fold.hpp: Schedule, sweep)
//   quotient_hash_pair_kernel                             both folded hash gates in one pass where they sit on the same wires
//                                                         (qfold::pairable: the leaf circuit), S-boxes and linear term shared
//   quotient_hash_rounds_kernel                           the hash gates round by round: the forward walk of the same Schedule
//                                                         (qfold::walk), the fold's A/B partner under QPGPU_QUOTIENT_FOLD=0
// Layout as in prover_kernels.hip: LDEs column-major in leaf order (slot j = point bitrev(j)).
// The hash gates share their end (quotient_add_store) and their swap prologue (qfold::swapped_inputs over the WireAt / WeighInto
// functors). quotient_gates_kernel keeps its own statement of the store, and the chunk products stay in the two kernels that form
// them: every shared form tried changed the instruction counts of quotient_gates_kernel<3|4, *> or of pp_rows_kernel
// (profiles/quotient_unit_isa.txt, notes at its end), which a refactor of this stage may not.
#include <hip/hip_runtime.h>
#include "gl64.hpp"
#include "poseidon.hpp"
#include "quotient_kernels.hpp"
#include "quotient_map.hpp"

using gl::e2;
using gl::u32;
using gl::u64;

namespace {

__device__ __forceinline__ u64 gate_filter(const QuotientArgs &a, u32 gi, u64 s) {
    const GateDev g = a.gates[gi];
    u64 f = 1;
    for (u32 j = g.group_start; j < g.group_end; j++)
        if (j != gi) f = gl::mul(f, gl::sub((u64)j, s));
    if (a.num_selectors > 1) f = gl::mul(f, gl::sub(0xFFFFFFFFull, s));
    return f;
}

// ---- s6 is three kernels over the LDE slots (thread = slot j, point index i = bitrev(j)), each adding its
// alpha-weighted terms into acc[c][j] (slot order, unit stride); the last one multiplies by 1/Z_H(x) and stores the
// quotient values in natural order for the inverse NTT. NCH (number of challenges) is a compile-time constant so the
// per-challenge accumulators live in registers.

// proof blockIdx.z of a lockstep batch: move the per-proof pointers
__device__ __forceinline__ void quotient_select_proof(QuotientArgs &a) {
    const u64 pr = blockIdx.z;
    a.wires += pr * a.ps_wires; a.zs_pp += pr * a.ps_zs;
    a.alpha_pows += pr * a.ps_small; a.beta_k_is += pr * a.ps_small; a.betas += pr * a.ps_small; a.gammas += pr * a.ps_small; a.pi_hash += pr * a.ps_small;
    a.acc += pr * a.ps_acc; a.out += pr * a.ps_out;
    if (a.fold) a.fold += pr * a.ps_fold;
}

// A hash gate's end at slot j: its filter f times its alpha-weighted sums joins the running sums, which go back in slot order or,
// on the stage's last launch, times 1/Z_H(x) to the quotient values in natural order for the inverse NTT.
template <int NCH>
__device__ __forceinline__ void quotient_add_store(const QuotientArgs &a, u64 S, u64 j, u64 f, const u64 (&sum)[NCH], int finalize) {
    if (finalize) {
        const u64 i = brev32((u32)j, a.log_lde);
        const u64 zi = a.zh_inv[i & (a.rate - 1)];
#pragma unroll
        for (int c = 0; c < NCH; c++) a.out[(u64)c * a.q_n + (i >> a.q_shift)] = gl::canon(gl::mul(gl::add(a.acc[(u64)c * S + j], gl::mul(f, sum[c])), zi));
    } else {
#pragma unroll
        for (int c = 0; c < NCH; c++) a.acc[(u64)c * S + j] = gl::add(a.acc[(u64)c * S + j], gl::mul(f, sum[c]));
    }
}

// how the hash-gate kernels read a wire at slot j and weigh constraint q of the gate into the per-challenge sums (plain structs:
// as lambdas handed to qfold::swapped_inputs they changed the folded kernels' code)
struct WireAt {
    const u64 *wires; u64 S, j;
    __device__ __forceinline__ u64 operator()(u32 w) const { return wires[(u64)w * S + j]; }
};
template <int NCH>
struct WeighInto {
    gl::Acc192 (&wsum)[NCH]; const u64 *ap; u32 nterms;
    __device__ __forceinline__ void operator()(u32 q, u64 cst) const {
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(wsum[c], cst, ap[(u64)c * nterms + q]);
    }
};

// (1) L_0(x)(Z(x) - 1) and the partial-product checks
template <int NCH>
__global__ void __launch_bounds__(256) quotient_perm_kernel(QuotientArgs a) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    quotient_select_proof(a);
    const u32 logL = a.log_lde, R = a.num_routed, chunk = a.chunk, nchunks = a.nchunks, npp = nchunks - 1;
    const u64 i = brev32((u32)j, logL);
    const u64 jn = brev32((u32)((i + a.rate) & (a.lde_n - 1)), logL);   // slot of the next row g*x
    const u64 x = a.x_coset[j], l0 = a.l0_coset[j], S = a.lde_n;
    gl::Acc192 acc[NCH];      // alpha-weighted sums as unreduced 192-bit accumulators (gl64.hpp): one reduction per challenge at the end
#pragma unroll
    for (int c = 0; c < NCH; c++) acc[c] = gl::acc_zero();
    u32 t = 0;
#pragma unroll
    for (int k = 0; k < NCH; k++, t++) {
        const u64 term = gl::mul(l0, gl::sub(a.zs_pp[(u64)k * S + j], 1));
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(acc[c], term, a.alpha_pows[(u64)c * a.nterms + t]);
    }
#pragma unroll
    for (int k = 0; k < NCH; k++) {
        const u64 beta = a.betas[k], gamma = a.gammas[k];
        u64 prev = a.zs_pp[(u64)k * S + j];
        for (u32 cc = 0; cc < nchunks; cc++, t++) {
            u64 pn = 1, pd = 1;
            for (u32 r = cc * chunk; r < (cc + 1) * chunk && r < R; r++) {
                const u64 w = a.wires[(u64)r * S + j];
                const u64 sid = gl::mul(a.beta_k_is[k * R + r], x);
                const u64 ssg = gl::mul(beta, a.cs[(u64)(a.sig0 + r) * S + j]);
                pn = gl::mul(pn, gl::add(gl::add(w, sid), gamma));
                pd = gl::mul(pd, gl::add(gl::add(w, ssg), gamma));
            }
            const u64 next = cc == nchunks - 1 ? a.zs_pp[(u64)k * S + jn] : a.zs_pp[((u64)NCH + (u64)k * npp + cc) * S + j];
            const u64 term = gl::sub(gl::mul(prev, pn), gl::mul(next, pd));
#pragma unroll
            for (int c = 0; c < NCH; c++) gl::acc_mul(acc[c], term, a.alpha_pows[(u64)c * a.nterms + t]);
            prev = next;
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; c++) a.acc[(u64)c * S + j] = gl::acc_reduce(acc[c]);
}

// One copy of a RandomAccessGate with 2^BITS list entries: out[0..BITS) the bit constraints, out[BITS] the index
// reconstruction, out[BITS+1] the list folded by the bits against the claimed element. BITS is a compile-time constant so
// the item array stays in registers (a dynamically indexed array went to scratch). The 32-entry form, which standard
// configurations do not use (arity 16, cap height 4), lives in its own kernel instance (WIDE) so that it does not set the
// register count of the common one.
template <int BITS>
__device__ __forceinline__ void random_access_values(const u64 *cw, const u64 *bw, u64 S, u64 *out) {
    constexpr int VEC = 1 << BITS;
    u64 items[VEC], bit[BITS];
#pragma unroll
    for (int i = 0; i < VEC; i++) items[i] = cw[(u64)(2 + i) * S];
#pragma unroll
    for (int i = 0; i < BITS; i++) { bit[i] = bw[(u64)i * S]; out[i] = gl::mul(bit[i], gl::sub(bit[i], 1)); }
    u64 idx = 0;
#pragma unroll
    for (int i = BITS - 1; i >= 0; i--) idx = gl::add(gl::add(idx, idx), bit[i]);
    out[BITS] = gl::sub(idx, cw[0]);
#pragma unroll
    for (int b = 0; b < BITS; b++) {
#pragma unroll
        for (int i = 0; i < (VEC >> (b + 1)); i++) items[i] = gl::add(items[2 * i], gl::mul(bit[b], gl::sub(items[2 * i + 1], items[2 * i])));
    }
    out[BITS + 1] = gl::sub(items[0], cw[S]);
}

// (2) every gate except PoseidonGate: Constant, PublicInput, BaseSum<2>, Arithmetic, the extension-arithmetic pair and the
// recursion set (Reducing*, RandomAccess, Exponentiation, PoseidonMds, CosetInterpolation). t0 = index of the first gate constraint.
template <int NCH, bool WIDE>
__global__ void __launch_bounds__(256) quotient_gates_kernel(QuotientArgs a, u32 t0, int finalize) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    quotient_select_proof(a);
    const u64 S = a.lde_n;
    u64 acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) acc[c] = a.acc[(u64)c * S + j];
    const u64 *consts_base = a.cs + (u64)a.num_selectors * S + j;
    const u64 *ap = a.alpha_pows + t0;
    for (u32 gi = 0; gi < a.num_gates; gi++) {
        const GateDev g = a.gates[gi];
        if (g.num_constraints == 0 || g.type == 4 || g.type == 14) continue;   // the hash gates have kernels of their own
        const u64 f = gate_filter(a, gi, a.cs[(u64)g.selector_index * S + j]);
        gl::Acc192 sum[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) sum[c] = gl::acc_zero();
        auto emit = [&](u32 q, u64 cst) {
#pragma unroll
            for (int c = 0; c < NCH; c++) gl::acc_mul(sum[c], cst, ap[(u64)c * a.nterms + q]);
        };
        // The leaf circuit's gate types run in fixed-size chunks: a chunk's wire loads are issued together, ahead of its arithmetic
        // (every load of a column is strided by S and independent of the others), and the chunk bodies unroll at compile time.
        if (g.type == 1) {            // ConstantGate: const_i - wire_i
            u32 q = 0;
#pragma unroll 1
            for (; q + 2 <= g.param0; q += 2) {
                const u64 k0 = consts_base[(u64)q * S], k1 = consts_base[(u64)(q + 1) * S], w0 = a.wires[(u64)q * S + j], w1 = a.wires[(u64)(q + 1) * S + j];
                emit(q, gl::sub(k0, w0)); emit(q + 1, gl::sub(k1, w1));
            }
            for (; q < g.param0; q++) emit(q, gl::sub(consts_base[(u64)q * S], a.wires[(u64)q * S + j]));
        } else if (g.type == 2) {     // PublicInputGate: wire_i - pi_hash_i
            u64 v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = a.wires[(u64)q * S + j];
#pragma unroll
            for (int q = 0; q < 4; q++) emit(q, gl::sub(v[q], a.pi_hash[q]));
        } else if (g.type == 3) {     // ArithmeticGate: out - (c0 m0 m1 + c1 addend), four operations per chunk
            const u64 c0 = consts_base[0], c1 = consts_base[S];
            const u64 *w = a.wires + j;
            u32 q = 0;
#pragma unroll 1
            for (; q + 4 <= g.param0; q += 4) {
                u64 v[16];
#pragma unroll
                for (int i = 0; i < 16; i++) v[i] = w[(u64)(4 * q + i) * S];
#pragma unroll
                for (int i = 0; i < 4; i++) emit(q + i, gl::sub(v[4 * i + 3], gl::add(gl::mul(gl::mul(v[4 * i], v[4 * i + 1]), c0), gl::mul(v[4 * i + 2], c1))));
            }
            for (; q < g.param0; q++) {
                const u64 m0 = w[(u64)(4 * q) * S], m1 = w[(u64)(4 * q + 1) * S], ad = w[(u64)(4 * q + 2) * S], out = w[(u64)(4 * q + 3) * S];
                emit(q, gl::sub(out, gl::add(gl::mul(gl::mul(m0, m1), c0), gl::mul(ad, c1))));
            }
        } else if (g.type == 6) {     // ArithmeticExtensionGate<2>: out - (c0 m0 m1 + c1 addend) over F[x]/(x^2-7)
            const u64 c0 = consts_base[0], c1 = consts_base[S];
            for (u32 q = 0; q < g.param0; q++) {
                const u64 *w = a.wires + (u64)(8 * q) * S + j;
                const e2 m0 = gl::e2_make(w[0], w[S]), m1 = gl::e2_make(w[2 * S], w[3 * S]), ad = gl::e2_make(w[4 * S], w[5 * S]);
                const e2 out = gl::e2_make(w[6 * S], w[7 * S]);
                const e2 d = gl::e2_sub(out, gl::e2_add(gl::e2_scale(gl::e2_mul(m0, m1), c0), gl::e2_scale(ad, c1)));
                emit(2 * q, d.a); emit(2 * q + 1, d.b);
            }
        } else if (g.type == 7) {     // MulExtensionGate<2>: out - c0 m0 m1
            const u64 c0 = consts_base[0];
            for (u32 q = 0; q < g.param0; q++) {
                const u64 *w = a.wires + (u64)(6 * q) * S + j;
                const e2 d = gl::e2_sub(gl::e2_make(w[4 * S], w[5 * S]),
                                        gl::e2_scale(gl::e2_mul(gl::e2_make(w[0], w[S]), gl::e2_make(w[2 * S], w[3 * S])), c0));
                emit(2 * q, d.a); emit(2 * q + 1, d.b);
            }
        } else if (g.type == 8 || g.type == 9) {   // ReducingGate / ReducingExtensionGate: acc*alpha + coeff_i - acc_i, chained
            const bool ext = g.type == 9;
            const u32 nc = g.param0, start_accs = 6 + (ext ? 2 * nc : nc);
            const u64 *w = a.wires + j;
            const e2 alpha = gl::e2_make(w[2 * S], w[3 * S]);
            e2 acc = gl::e2_make(w[4 * S], w[5 * S]);
            for (u32 q = 0; q < nc; q++) {
                const u32 nx = q == nc - 1 ? 0 : start_accs + 2 * q;
                const e2 next = gl::e2_make(w[(u64)nx * S], w[(u64)(nx + 1) * S]);
                e2 t = gl::e2_mul(acc, alpha);
                if (ext) t = gl::e2_add(t, gl::e2_make(w[(u64)(6 + 2 * q) * S], w[(u64)(7 + 2 * q) * S]));
                else t.a = gl::add(t.a, w[(u64)(6 + q) * S]);
                emit(2 * q, gl::sub(t.a, next.a)); emit(2 * q + 1, gl::sub(t.b, next.b));
                acc = next;
            }
        } else if (g.type == 10) {    // RandomAccessGate(bits, copies, extra constants)
            const u32 bits = g.param0, copies = g.param1, extra = g.param2, vec = 1u << bits;
            const u32 routed = (2 + vec) * copies + extra;
            u32 q = 0;
            for (u32 cp = 0; cp < copies; cp++) {
                const u64 *cw = a.wires + (u64)((2 + vec) * cp) * S + j, *bw = a.wires + (u64)(routed + cp * bits) * S + j;
                u64 vals[7];
                switch (bits) {
                    case 1: random_access_values<1>(cw, bw, S, vals); break;
                    case 2: random_access_values<2>(cw, bw, S, vals); break;
                    case 3: random_access_values<3>(cw, bw, S, vals); break;
                    case 4: random_access_values<4>(cw, bw, S, vals); break;
                    default: if constexpr (WIDE) random_access_values<5>(cw, bw, S, vals); break;
                }
                for (u32 i = 0; i < bits + 2; i++) emit(q++, vals[i]);
            }
            for (u32 i = 0; i < extra; i++) emit(q++, gl::sub(consts_base[(u64)i * S], a.wires[(u64)((2 + vec) * copies + i) * S + j]));
        } else if (g.type == 11) {    // ExponentiationGate: square-and-multiply chain over the power bits (big-endian walk)
            const u32 n = g.param0;
            const u64 *w = a.wires + j;
            const u64 base = w[0];
            for (u32 q = 0; q < n; q++) {
                const u64 pi = q == 0 ? 1 : w[(u64)(2 + n + q - 1) * S];
                const u64 prev = q == 0 ? 1 : gl::mul(pi, pi);
                const u64 bit = w[(u64)(1 + (n - 1 - q)) * S];
                const u64 computed = gl::mul(prev, gl::add(gl::mul(bit, base), gl::sub(1, bit)));
                emit(q, gl::sub(computed, w[(u64)(2 + n + q) * S]));
            }
            emit(n, gl::sub(w[(u64)(1 + n) * S], w[(u64)(2 + n + n - 1) * S]));
        } else if (g.type == 12) {    // PoseidonMdsGate: out - MDS(in) on 12 extension-algebra elements, component by component
            const u64 *w = a.wires + j;
            for (u32 comp = 0; comp < 2; comp++) {
                u64 st[12];
#pragma unroll
                for (int i = 0; i < 12; i++) st[i] = w[(u64)(2 * i + comp) * S];
                poseidon::mds_layer(st);
#pragma unroll
                for (int i = 0; i < 12; i++) emit(2 * i + comp, gl::sub(w[(u64)(24 + 2 * i + comp) * S], st[i]));
            }
        } else if (g.type == 13) {    // CosetInterpolationGate(subgroup_bits, degree): chunked barycentric interpolation
            const u32 bits = g.param0, deg = g.param1, np = 1u << bits, ni = (np - 2) / (deg - 1);
            const u32 s_ep = 1 + 2 * np, s_ev = s_ep + 2, s_int = s_ev + 2;
            const u64 *w = a.wires + j;
            auto ld = [&](u32 c) { return gl::e2_make(w[(u64)c * S], w[(u64)(c + 1) * S]); };
            const u64 shift = w[0];
            const e2 ep = ld(s_ep), sp = ld(s_int + 4 * ni);
            emit(0, gl::sub(ep.a, gl::mul(sp.a, shift))); emit(1, gl::sub(ep.b, gl::mul(sp.b, shift)));
            // subgroup of order 2^bits: generator 2^(192 >> bits); barycentric weight of x_i is x_i / 2^bits, and
            // 1 / 2^bits = -2^(96 - bits) = p - (2^(64-bits) - 2^(32-bits))
            const u64 omega = 1ull << (192u >> bits), inv_n = gl::P - ((1ull << (64 - bits)) - (1ull << (32 - bits)));
            e2 ev = gl::e2_from(0), pr = gl::e2_from(1);
            u64 x = 1;
            u32 lo = 0, hi = deg, q_out = 2;
            for (u32 c = 0; c <= ni; c++) {
                for (u32 q = lo; q < hi; q++) {
                    e2 term = sp; term.a = gl::sub(term.a, x);
                    const e2 t = gl::e2_scale(gl::e2_mul(ld(1 + 2 * q), pr), gl::mul(x, inv_n));
                    ev = gl::e2_add(gl::e2_mul(ev, term), t);
                    pr = gl::e2_mul(pr, term);
                    x = gl::mul(x, omega);
                }
                if (c == ni) break;
                const e2 ie = ld(s_int + 2 * c), ip = ld(s_int + 2 * (ni + c));
                emit(q_out++, gl::sub(ie.a, ev.a)); emit(q_out++, gl::sub(ie.b, ev.b));
                emit(q_out++, gl::sub(ip.a, pr.a)); emit(q_out++, gl::sub(ip.b, pr.b));
                ev = ie; pr = ip;
                lo = 1 + (deg - 1) * (c + 1); hi = lo + deg - 1 < np ? lo + deg - 1 : np;
            }
            const e2 val = ld(s_ev);
            emit(q_out++, gl::sub(val.a, ev.a)); emit(q_out++, gl::sub(val.b, ev.b));
        } else if (g.type == 5) {     // BaseSumGate<2>: sum - sum_i 2^i limb_i, and limb_i (limb_i - 1); every limb is loaded once,
            // from the top limb down (Horner), eight per chunk
            const u64 *w = a.wires + S + j;      // limb 0
            u64 s2 = 0;
            u32 q = g.param0;
            for (; q & 7; ) {
                const u64 limb = w[(u64)--q * S];
                s2 = gl::add(gl::add(s2, s2), limb);
                emit(1 + q, gl::mul(limb, gl::sub(limb, 1)));
            }
#pragma unroll 1
            while (q) {
                q -= 8;
                u64 v[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = w[(u64)(q + i) * S];
#pragma unroll
                for (int i = 7; i >= 0; i--) {
                    s2 = gl::add(gl::add(s2, s2), v[i]);
                    emit(1 + q + i, gl::mul(v[i], gl::sub(v[i], 1)));
                }
            }
            emit(0, gl::sub(s2, a.wires[j]));
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = gl::add(acc[c], gl::mul(f, gl::acc_reduce(sum[c])));
    }
    if (finalize) {
        const u64 i = brev32((u32)j, a.log_lde);
        const u64 zi = a.zh_inv[i & (a.rate - 1)];
#pragma unroll
        for (int c = 0; c < NCH; c++) a.out[(u64)c * a.q_n + (i >> a.q_shift)] = gl::canon(gl::mul(acc[c], zi));
    } else {
#pragma unroll
        for (int c = 0; c < NCH; c++) a.acc[(u64)c * S + j] = acc[c];
    }
}

// (1+2) The permutation terms and the wire-local gates (Constant, PublicInput, Arithmetic, BaseSum<2>) in one pass over the routed
// wires: what quotient_perm_kernel and quotient_gates_kernel leave in acc (or, without a hash gate, in out) for a circuit whose
// other gates are all of these four types and read routed wires only (fused_gates below decides). The walk goes by the permutation
// argument's chunks of FUSED_CHUNK wires, from the last chunk down to chunk 0: a chunk's wires and sigmas are loaded once, serve
// pn and pd of every challenge, and while the wires are in registers the gates take what they need of them: Arithmetic operations
// 2cc and 2cc+1, the BaseSum limbs (top limb first, so the limb sum is the Horner value quotient_gates_kernel forms; chunk 0 ends
// with the sum wire), and in chunk 0 the Constant and PublicInput wires. One Acc192 per gate and challenge; filters and the add
// into the running sums once at the end. The 1-D grid's workgroup id -> (tile, proof) is qmap::place (quotient_map.hpp).
constexpr u32 FUSED_CHUNK = 8;
constexpr u32 FUSED_NONE = 0xFFFFFFFFu;

template <int NCH>
__global__ void __launch_bounds__(256, NCH <= 2 ? 4 : NCH == 3 ? 3 : 2) quotient_perm_gates_kernel(QuotientArgs a, FusedGates fg, u32 tiles, u32 grouped, int finalize) {
    const qmap::Place pl = qmap::place(blockIdx.x, tiles, a.batch, grouped != 0);
    if (!pl.valid) return;
    const u64 j = pl.tile * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    {
        const u64 pr = pl.proof;
        a.wires += pr * a.ps_wires; a.zs_pp += pr * a.ps_zs;
        a.alpha_pows += pr * a.ps_small; a.beta_k_is += pr * a.ps_small; a.betas += pr * a.ps_small; a.gammas += pr * a.ps_small; a.pi_hash += pr * a.ps_small;
        a.acc += pr * a.ps_acc; a.out += pr * a.ps_out;
    }
    const u32 logL = a.log_lde, R = a.num_routed, nchunks = a.nchunks, npp = nchunks - 1;
    const u64 i = brev32((u32)j, logL);
    const u64 jn = brev32((u32)((i + a.rate) & (a.lde_n - 1)), logL);   // slot of the next row g*x
    const u64 x = a.x_coset[j], S = a.lde_n;
    const u64 *consts_base = a.cs + (u64)a.num_selectors * S + j;
    const u64 *gp = a.alpha_pows + NCH + NCH * nchunks;                 // weights of the gate constraints
    const u32 n_ops = fg.n_ops, n_limbs = fg.n_limbs;
    gl::Acc192 acc[NCH], asum[NCH], bsum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) { acc[c] = gl::acc_zero(); asum[c] = gl::acc_zero(); bsum[c] = gl::acc_zero(); }
    u64 nxt[NCH];       // the partial product behind the chunk being walked: Z(g x) behind the last one
    {
        const u64 l0 = a.l0_coset[j];
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const u64 term = gl::mul(l0, gl::sub(a.zs_pp[(u64)k * S + j], 1));
#pragma unroll
            for (int c = 0; c < NCH; c++) gl::acc_mul(acc[c], term, a.alpha_pows[(u64)c * a.nterms + k]);
            nxt[k] = a.zs_pp[(u64)k * S + jn];
        }
    }
    u64 s2 = 0;         // the BaseSum limbs seen so far, top limb first (Horner)
    u64 gsum[NCH];      // filtered sums of the gates that are done
#pragma unroll
    for (int c = 0; c < NCH; c++) gsum[c] = 0;
    auto fold_gate = [&](u32 gi, const gl::Acc192 (&sum)[NCH]) {
        const u64 f = gate_filter(a, gi, a.cs[(u64)a.gates[gi].selector_index * S + j]);
#pragma unroll
        for (int c = 0; c < NCH; c++) gsum[c] = gl::add(gsum[c], gl::mul(f, gl::acc_reduce(sum[c])));
    };
    // One chunk per turn, from the last one down. A whole chunk is one straight run of code: its eight wires and eight sigmas are
    // loaded together ahead of the arithmetic, and what a gate does not want of a wire goes in with weight zero (a scalar select)
    // instead of round a branch, which would put every wire's loads behind the wire before it. Only the last chunk can hold fewer
    // than FUSED_CHUNK wires (m of them) and goes wire by wire. (Skipping the limb work of the chunks past the last limb, or the
    // Arithmetic work past the last operation, behind chunk-uniform branches costs the two-challenge kernel 20 to 28 bytes of
    // scratch at four waves per SIMD: profiles/quotient_pass_notes.txt.)
    auto wire = [&](u32 r, u64 v, u64 sg, u64 (&pn)[NCH], u64 (&pd)[NCH]) {
        // A factor is beta_k k_r x + (v + gamma_k), resp. beta_k sigma + (v + gamma_k): v + gamma_k once for both, and the 128-bit
        // product takes it as a 64-bit addend before its ONE reduction (gl::mul_add, exact for any 64-bit operands; the table's
        // beta_k k_r are canonical, stage_fill_betas) where a reduced product and two modular sums cost 29 vector instructions.
        // gamma_k is canonical in the table (stage_fill_betas), so v + gamma_k needs one carry fold (gl::add_canonical).
        if constexpr (NCH == 1) {
            // one challenge: the reduced forms stay (the forms below cost this instantiation its fifth wave per SIMD: 102 registers for 96)
            const u64 sid = gl::mul(a.beta_k_is[r], x);
            const u64 ssg = gl::mul(a.betas[0], sg);
            pn[0] = gl::mul(pn[0], gl::add(gl::add(v, sid), a.gammas[0]));
            pd[0] = gl::mul(pd[0], gl::add(gl::add(v, ssg), a.gammas[0]));
        } else {
#pragma unroll
            for (int k = 0; k < NCH; k++) {
                const u64 vg = gl::add_canonical(v, a.gammas[k]);
                pn[k] = gl::mul(pn[k], gl::mul_add(a.beta_k_is[k * R + r], x, vg));
                pd[k] = gl::mul(pd[k], gl::mul_add(a.betas[k], sg, vg));
            }
        }
        // BaseSumGate<2>: limb l on wire 1 + l, constraint 1 + l (the sum, wire 0, after the walk)
        const bool limb = r >= 1 && r <= n_limbs;
        const u64 twice = gl::add(gl::add(s2, s2), v), cst = gl::mul(v, gl::sub(v, 1));
        s2 = limb ? twice : s2;
#pragma unroll
        for (int c = 0; c < NCH; c++) { const u64 wt = gp[(u64)c * a.nterms + (limb ? r : 0)]; gl::acc_mul(bsum[c], cst, limb ? wt : 0); }
    };
    // ArithmeticGate: out - (c0 m0 m1 + c1 addend), operation q on wires 4q..4q+3; c0, c1 = the first two constant columns
    auto arith = [&](u32 q, u64 m0, u64 m1, u64 ad, u64 out, u64 c0, u64 c1) {
        const bool op = q < n_ops;
        const u64 cst = gl::sub(out, gl::add(gl::mul(gl::mul(m0, m1), c0), gl::mul(ad, c1)));
#pragma unroll
        for (int c = 0; c < NCH; c++) { const u64 wt = gp[(u64)c * a.nterms + (op ? q : 0)]; gl::acc_mul(asum[c], cst, op ? wt : 0); }
    };
#pragma unroll 1
    for (u32 cc = nchunks; cc-- > 0; ) {
        const u32 r0 = cc * FUSED_CHUNK, m = R - r0 < FUSED_CHUNK ? R - r0 : FUSED_CHUNK;
        u64 w[FUSED_CHUNK], pn[NCH], pd[NCH], prv[NCH];
#pragma unroll
        for (int k = 0; k < NCH; k++) { pn[k] = 1; pd[k] = 1; prv[k] = cc == 0 ? a.zs_pp[(u64)k * S + j] : a.zs_pp[((u64)NCH + (u64)k * npp + cc - 1) * S + j]; }
        const u64 c0 = consts_base[0], c1 = consts_base[S];
        if (m == FUSED_CHUNK) {
            u64 sg[FUSED_CHUNK];
#pragma unroll
            for (u32 t = 0; t < FUSED_CHUNK; t++) { w[t] = a.wires[(u64)(r0 + t) * S + j]; sg[t] = a.cs[(u64)(a.sig0 + r0 + t) * S + j]; }
#pragma unroll
            for (int t = FUSED_CHUNK - 1; t >= 0; t--) {
                wire(r0 + t, w[t], sg[t], pn, pd);
                if (t % 4 == 0) arith((r0 + t) / 4, w[t], w[t + 1], w[t + 2], w[t + 3], c0, c1);
            }
        } else {
#pragma unroll
            for (int t = FUSED_CHUNK - 1; t >= 0; t--) {
                w[t] = 0;
                if ((u32)t < m) { w[t] = a.wires[(u64)(r0 + t) * S + j]; wire(r0 + t, w[t], a.cs[(u64)(a.sig0 + r0 + t) * S + j], pn, pd); }
                if (t % 4 == 0 && (r0 + t) / 4 < n_ops) arith((r0 + t) / 4, w[t], w[t + 1], w[t + 2], w[t + 3], c0, c1);
            }
        }
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const u64 term = gl::sub(gl::mul(prv[k], pn[k]), gl::mul(nxt[k], pd[k]));
#pragma unroll
            for (int c = 0; c < NCH; c++) gl::acc_mul(acc[c], term, a.alpha_pows[(u64)c * a.nterms + NCH + k * nchunks + cc]);
            nxt[k] = prv[k];
        }
        if (cc == 0) {       // chunk 0 is whole: the gates that live on its wires, and the end of the two that ran along
            if (fg.base_sum != FUSED_NONE) {
                const u64 cst = gl::sub(s2, w[0]);
#pragma unroll
                for (int c = 0; c < NCH; c++) gl::acc_mul(bsum[c], cst, gp[(u64)c * a.nterms]);
                fold_gate(fg.base_sum, bsum);
            }
            if (fg.arithmetic != FUSED_NONE) fold_gate(fg.arithmetic, asum);
            if (fg.constant != FUSED_NONE) {      // ConstantGate: const_i - wire_i
                gl::Acc192 sum[NCH];
#pragma unroll
                for (int c = 0; c < NCH; c++) sum[c] = gl::acc_zero();
#pragma unroll
                for (u32 q = 0; q < 4; q++)
                    if (q < fg.n_consts) {
                        const u64 cst = gl::sub(consts_base[(u64)q * S], w[q]);
#pragma unroll
                        for (int c = 0; c < NCH; c++) gl::acc_mul(sum[c], cst, gp[(u64)c * a.nterms + q]);
                    }
                fold_gate(fg.constant, sum);
            }
            if (fg.public_input != FUSED_NONE) {  // PublicInputGate: wire_i - pi_hash_i
                gl::Acc192 sum[NCH];
#pragma unroll
                for (int c = 0; c < NCH; c++) sum[c] = gl::acc_zero();
#pragma unroll
                for (u32 q = 0; q < 4; q++) {
                    const u64 cst = gl::sub(w[q], a.pi_hash[q]);
#pragma unroll
                    for (int c = 0; c < NCH; c++) gl::acc_mul(sum[c], cst, gp[(u64)c * a.nterms + q]);
                }
                fold_gate(fg.public_input, sum);
            }
        }
    }
    if (finalize) {
        const u64 zi = a.zh_inv[i & (a.rate - 1)];
#pragma unroll
        for (int c = 0; c < NCH; c++) a.out[(u64)c * a.q_n + (i >> a.q_shift)] = gl::canon(gl::mul(gl::add(gl::acc_reduce(acc[c]), gsum[c]), zi));
    } else {
#pragma unroll
        for (int c = 0; c < NCH; c++) a.acc[(u64)c * S + j] = gl::add(gl::acc_reduce(acc[c]), gsum[c]);
    }
}

// (3), (4) the two hash gates at one point, round by round (QuotientArgs::fold == nullptr): every constraint of qfold::walk weighted
// by alpha_c^(t0+q) on the fly. PoseidonGate (plonky2::gates::poseidon): wires 0..11 input, 12..23 output, 24 swap, 25..28 delta,
// 29..64 / 65..86 / 87..134 S-box inputs of the full / partial / full rounds, 123 constraints; the partial rounds run in the textbook
// schedule (the value fed to the S-box is the same in upstream's fast-partial basis, which leaves lane 0 alone). The qp fork's
// Poseidon2 gate (type 14; the gate behind `hash_n_to_hash_no_pad_p2`, reference call sites
// wormhole/circuit/src/zk_merkle_proof.rs:482,504,606, nullifier.rs:298-299, unspendable_account.rs:229-231,
// block_header/mod.rs:66): the permutation is qp-poseidon-core's Poseidon2 (pinned by the reference's seven known-answer vectors);
// the wire layout comes from the pack (P2GateLayout, default = upstream PoseidonGate's layout carried over: LAYOUT UNPINNED), with
// an optional swap and optionally round 0's S-box inputs on wires as well. Both structures are the Schedule's (quotient_fold.hpp).
// KIND pins s.kind, so the other gate's branches fold away.
template <int NCH, u32 KIND>
__global__ void __launch_bounds__(256) quotient_hash_rounds_kernel(QuotientArgs a, qfold::Schedule s, u32 gi, u32 t0, int finalize) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    s.kind = KIND;
    quotient_select_proof(a);
    const u64 S = a.lde_n;
    const u64 *ap = a.alpha_pows + t0;
    gl::Acc192 wsum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) wsum[c] = gl::acc_zero();
    qfold::walk(s, qfold::Consts{a.poseidon_rc, a.p2_gate}, WireAt{a.wires, S, j}, WeighInto<NCH>{wsum, ap, a.nterms});
    const u64 f = gate_filter(a, gi, a.cs[(u64)a.gates[gi].selector_index * S + j]);
    u64 sum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) sum[c] = gl::acc_reduce(wsum[c]);
    quotient_add_store(a, S, j, f, sum, finalize);
}

// ---- (3'), (4') the hash gates with their linear layers folded into the alpha weights (quotient_fold.hpp) ----
// x^7 of N independent values as rare-fold product groups (gl::mul_group: 12 instead of 15 vector instructions per product, one
// scalar branch per group and stage). These launches are large (q_n x batch threads), the regime that form is for.
template <int N>
__device__ __forceinline__ void sbox7_group(u64 (&x)[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
    u64 x2[N], x3[N], x4[N];
    gl::mul_group(x2, x, x);
    gl::mul_group(x4, x2, x2);
    gl::mul_group(x3, x, x2);
    gl::mul_group(x, x3, x4);
#else
    for (int i = 0; i < N; i++) x[i] = poseidon::sbox7(x[i]);   // host pass of the unit: parsed, never called
#endif
}
// Wires per product group (it divides 12; 106 and 118 wires leave the same tail). The group's temporaries set the kernels' register
// count: 12 per group (a full round's worth) needs 134 VGPRs, 6 needs 98, 4 needs 86-88 and runs five waves per SIMD. Measured per
// lockstep batch of 32 at 2^13 rows, PoseidonGate / Poseidon2 gate: 514 / 522 us, 476 / 481 us, 443 / 440 us
// (profiles/quotient_fold_notes.txt).
#ifndef FOLD_GROUP
#define FOLD_GROUP 4
#endif
constexpr int FOLD_TAIL = 106 % FOLD_GROUP, FOLD_HEAD = FOLD_GROUP;   // FOLD_GROUP divides 12
static_assert(12 % FOLD_GROUP == 0, "the head's twelve S-boxes go in whole groups");
static_assert(118 % FOLD_GROUP == FOLD_TAIL && FOLD_TAIL > 0, "the tail group serves both wire counts");
// N target wires from number j0 on: each adds wire * (-alpha^q) and wire^7 * omega. Their S-box inputs are all wires, hence
// independent of one another also across partial rounds: one product group per stage for the N of them.
template <int NCH, int N>
__device__ __forceinline__ void fold_targets(const QuotientArgs &a, const qfold::Schedule &s, const u64 *F, u64 j, u32 j0, gl::Acc192 (&wsum)[NCH]) {
    u64 v[N];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = a.wires[(u64)qfold::target_wire(s, j0 + i) * a.lde_n + j];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(wsum[c], v[i], F[c * qfold::WORDS + qfold::T_NALPHA + j0 + i]);
    sbox7_group(v);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(wsum[c], v[i], F[c * qfold::WORDS + qfold::T_OMEGA + j0 + i]);
}
// One point of one hash gate. Shared with the round-by-round kernel: the swap / delta constraints (qfold::swapped_inputs),
// gate_filter, the end (quotient_add_store) and the proof selection.
// Acc192::top counts the carries out of 128 bits of at most 5 + 12 + 2 * 118 + 12 = 265
// products below 2^128: it stays below 2^9 of its 32 bits.
template <int NCH>
__device__ __forceinline__ void hash_gate_folded(QuotientArgs &a, const qfold::Schedule &s, u32 gi, u32 t0, u32 slot, int finalize) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    quotient_select_proof(a);
    const u64 S = a.lde_n;
    const u64 *ap = a.alpha_pows + t0;
    const u64 *F = a.fold + (u64)slot * NCH * qfold::WORDS;
    const qfold::Consts K = {a.poseidon_rc, a.p2_gate};
    auto W = [&](u32 i) -> u64 { return a.wires[(u64)i * S + j]; };
    gl::Acc192 wsum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) wsum[c] = gl::acc_zero();
    u64 st[12];
    qfold::swapped_inputs(s, WireAt{a.wires, S, j}, WeighInto<NCH>{wsum, ap, a.nterms}, st);
    qfold::head_inputs(s, K, st);
    if (s.head == qfold::HEAD_SBOX) {      // in groups of FOLD_GROUP like the target wires: the group size sets the kernel's register count
#pragma unroll
        for (int g0 = 0; g0 < 12; g0 += FOLD_HEAD) {
            u64 h[FOLD_HEAD];
#pragma unroll
            for (int i = 0; i < FOLD_HEAD; i++) h[i] = st[g0 + i];
            sbox7_group(h);
#pragma unroll
            for (int i = 0; i < FOLD_HEAD; i++) st[g0 + i] = h[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 12; i++)
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(wsum[c], st[i], F[c * qfold::WORDS + qfold::T_HEAD + i]);
    u32 j0 = 0;
#pragma unroll 1
    for (; j0 + FOLD_GROUP <= s.nw; j0 += FOLD_GROUP) fold_targets<NCH, FOLD_GROUP>(a, s, F, j, j0, wsum);
    if (s.nw - j0 == FOLD_TAIL) { fold_targets<NCH, FOLD_TAIL>(a, s, F, j, j0, wsum); j0 += FOLD_TAIL; }   // 106 and 118 both leave this many
#pragma unroll 1
    for (; j0 < s.nw; j0++) fold_targets<NCH, 1>(a, s, F, j, j0, wsum);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const u64 o = W(s.w_output + i);
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(wsum[c], o, F[c * qfold::WORDS + qfold::T_NALPHA + s.nw + i]);
    }
    const u64 f = gate_filter(a, gi, a.cs[(u64)a.gates[gi].selector_index * S + j]);
    u64 sum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) sum[c] = gl::add(gl::acc_reduce(wsum[c]), F[c * qfold::WORDS + qfold::T_KAPPA]);
    quotient_add_store(a, S, j, f, sum, finalize);
}
template <int NCH>
__global__ void __launch_bounds__(256) quotient_poseidon_kernel(QuotientArgs a, qfold::Schedule s, u32 gi, u32 t0, u32 slot, int finalize) {
    s.kind = GATE_POSEIDON; s.head = qfold::HEAD_SBOX;    // known here: the other gate's branches fold away
    hash_gate_folded<NCH>(a, s, gi, t0, slot, finalize);
}
template <int NCH>
__global__ void __launch_bounds__(256) quotient_poseidon2_kernel(QuotientArgs a, qfold::Schedule s, u32 gi, u32 t0, u32 slot, int finalize) {
    s.kind = GATE_POSEIDON2;
    hash_gate_folded<NCH>(a, s, gi, t0, slot, finalize);
}
// ---- (3'+4') a PoseidonGate and a Poseidon2 gate on the same wires (qfold::pairable) in one pass ----
// Both gates' layout is then qfold::poseidon_schedule(), known here. What the two folded kernels each did on their own is done once:
// the swapped inputs, the swap / delta constraints, the load of every target wire and output, their -alpha^q weights and the
// target wires' S-boxes. Per challenge three sums: lin (swap / delta constraints, targets and outputs by -alpha^q; T_NALPHA is read
// from table slot 0, the other slot holds the same values) and omA, omB (each gate's head and wire S-boxes by its own omega). A
// target wire costs one S-box and 3 * NCH weighted products instead of two and 4 * NCH. PAIR_GROUP: wires per product group, as
// FOLD_GROUP above (it divides 12 and leaves the same tail); resources and times of 4 and 6 in profiles/quotient_pair_notes.txt.
// Acc192::top: lin takes 5 + 106 + 12 = 123 products below 2^128, omA and omB 12 + 106 = 118 each, and the sum of lin and one of
// them counts at most 241 carries and one of its own: below 2^8, under the 265 of hash_gate_folded.
#ifndef PAIR_GROUP
#define PAIR_GROUP FOLD_GROUP
#endif
constexpr int PAIR_TAIL = 106 % PAIR_GROUP;
static_assert(12 % PAIR_GROUP == 0 && PAIR_TAIL > 0, "whole groups in the head, one tail group behind the 106 target wires");
__device__ __forceinline__ gl::Acc192 acc_sum(const gl::Acc192 &x, const gl::Acc192 &y) {
    gl::Acc192 r;
    r.lo = x.lo + y.lo;
    const u64 c0 = r.lo < x.lo ? 1 : 0, h = x.hi + y.hi;
    r.hi = h + c0;
    r.top = x.top + y.top + (u32)(h < x.hi ? 1 : 0) + (u32)(r.hi < c0 ? 1 : 0);
    return r;
}
// the twelve head S-boxes of one gate, in product groups, weighted into its omega sums
template <int NCH>
__device__ __forceinline__ void pair_head(const u64 (&st)[12], const u64 *F, gl::Acc192 (&om)[NCH]) {
#pragma unroll
    for (int g0 = 0; g0 < 12; g0 += PAIR_GROUP) {
        u64 h[PAIR_GROUP];
#pragma unroll
        for (int i = 0; i < PAIR_GROUP; i++) h[i] = st[g0 + i];
        sbox7_group(h);
#pragma unroll
        for (int i = 0; i < PAIR_GROUP; i++)
#pragma unroll
            for (int c = 0; c < NCH; c++) gl::acc_mul(om[c], h[i], F[c * qfold::WORDS + qfold::T_HEAD + g0 + i]);
    }
}
// N target wires from number j0 on: loaded once, wire * (-alpha^q) into lin, one S-box, wire^7 * omega into each gate's sums
template <int NCH, int N>
__device__ __forceinline__ void pair_targets(const QuotientArgs &a, const qfold::Schedule &s, const u64 *FA, const u64 *FB, u64 j, u32 j0,
                                             gl::Acc192 (&lin)[NCH], gl::Acc192 (&omA)[NCH], gl::Acc192 (&omB)[NCH]) {
    u64 v[N];
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = a.wires[(u64)qfold::target_wire(s, j0 + i) * a.lde_n + j];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(lin[c], v[i], a.fold[c * qfold::WORDS + qfold::T_NALPHA + j0 + i]);
    sbox7_group(v);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            gl::acc_mul(omA[c], v[i], FA[c * qfold::WORDS + qfold::T_OMEGA + j0 + i]);
            gl::acc_mul(omB[c], v[i], FB[c * qfold::WORDS + qfold::T_OMEGA + j0 + i]);
        }
}
// giA / slotA: the PoseidonGate's index in the gate list and its table slot, giB / slotB: the Poseidon2 gate's
template <int NCH>
__global__ void __launch_bounds__(256, NCH <= 2 ? 4 : 2) quotient_hash_pair_kernel(QuotientArgs a, u32 giA, u32 giB, u32 slotA, u32 slotB, u32 t0, int finalize) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= a.q_n) return;
    quotient_select_proof(a);
    const u64 S = a.lde_n;
    const u64 *ap = a.alpha_pows + t0;
    const u64 *FA = a.fold + (u64)slotA * NCH * qfold::WORDS, *FB = a.fold + (u64)slotB * NCH * qfold::WORDS;
    const qfold::Consts K = {a.poseidon_rc, a.p2_gate};
    const qfold::Schedule s = qfold::poseidon_schedule();
    qfold::Schedule sB = s;
    sB.kind = GATE_POSEIDON2;
    gl::Acc192 lin[NCH], omA[NCH], omB[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) { lin[c] = gl::acc_zero(); omA[c] = gl::acc_zero(); omB[c] = gl::acc_zero(); }
    u64 st[12];
    qfold::swapped_inputs(s, WireAt{a.wires, S, j}, WeighInto<NCH>{lin, ap, a.nterms}, st);
    {
        u64 h[12];
#pragma unroll
        for (int i = 0; i < 12; i++) h[i] = st[i];
        qfold::head_inputs(s, K, h);
        pair_head<NCH>(h, FA, omA);
    }
    qfold::head_inputs(sB, K, st);
    pair_head<NCH>(st, FB, omB);
    u32 j0 = 0;
#pragma unroll 1
    for (; j0 + PAIR_GROUP <= s.nw; j0 += PAIR_GROUP) pair_targets<NCH, PAIR_GROUP>(a, s, FA, FB, j, j0, lin, omA, omB);
    pair_targets<NCH, PAIR_TAIL>(a, s, FA, FB, j, j0, lin, omA, omB);
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const u64 o = a.wires[(u64)(s.w_output + i) * S + j];
#pragma unroll
        for (int c = 0; c < NCH; c++) gl::acc_mul(lin[c], o, a.fold[c * qfold::WORDS + qfold::T_NALPHA + s.nw + i]);
    }
    const u64 fA = gate_filter(a, giA, a.cs[(u64)a.gates[giA].selector_index * S + j]);
    const u64 fB = gate_filter(a, giB, a.cs[(u64)a.gates[giB].selector_index * S + j]);
    u64 sum[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const u64 gA = gl::add(gl::acc_reduce(acc_sum(omA[c], lin[c])), FA[c * qfold::WORDS + qfold::T_KAPPA]);
        const u64 gB = gl::add(gl::acc_reduce(acc_sum(omB[c], lin[c])), FB[c * qfold::WORDS + qfold::T_KAPPA]);
        sum[c] = gl::add(gl::mul(fA, gA), gl::mul(fB, gB));
    }
    quotient_add_store(a, S, j, 1, sum, finalize);     // the filters are in already
}
// the backward walk: block (hash gate, challenge, proof), one wave; 48 of its lanes share a step's 144 products
__global__ void __launch_bounds__(64) quotient_fold_sweep_kernel(FoldSweepArgs fa) {
    __shared__ qfold::Scratch scratch;
    const u32 slot = blockIdx.x, c = blockIdx.y;
    const u64 pr = blockIdx.z;
    const u64 *ap = fa.alpha_pows + pr * fa.ps_small + (u64)c * fa.nterms + fa.t0;
    u64 *table = fa.fold + pr * fa.ps_fold + ((u64)slot * fa.nch + c) * qfold::WORDS;
    const qfold::Consts K = {fa.poseidon_rc, fa.p2_gate};
    qfold::sweep(fa.sched[slot], K, ap, scratch, table, threadIdx.x, blockDim.x, [] { __syncthreads(); });
}

// Witness check on the trace rows (optional): acc holds the alpha-weighted gate-constraint sums per row (the gate kernels
// run on the value arrays, S = n). result[0] = smallest row with a non-zero sum, result[1] = 1 when a permutation
// product does not close (Z(g x_{n-1}) != 1), i.e. a copy constraint is violated.
__global__ void __launch_bounds__(256) witness_check_kernel(const u64 *acc, u64 n, u32 nch, const u64 *z, const u64 *rowprod, u64 *result) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    { const u64 pr = blockIdx.z; acc += pr * nch * n; z += pr * nch * n; rowprod += pr * nch * n; result += pr * 2; }
    bool bad = false;
    for (u32 c = 0; c < nch; c++) bad |= gl::canon(acc[(u64)c * n + i]) != 0;
    if (bad) atomicMin((unsigned long long *)&result[0], (unsigned long long)i);
    if (i == n - 1)
        for (u32 c = 0; c < nch; c++)
            if (gl::canon(gl::mul(z[(u64)c * n + i], rowprod[(u64)c * n + i])) != 1) atomicMax((unsigned long long *)&result[1], 1ull);
}

}  // namespace

static bool wide_random_access(const QuotientArgs &a, const GateDev *host_gates) {
    for (u32 i = 0; i < a.num_gates; i++) if (host_gates[i].type == 10 && host_gates[i].param0 > 4) return true;
    return false;
}
static bool is_hash_gate(const GateDev &g) { return (g.type == GATE_POSEIDON || g.type == GATE_POSEIDON2) && g.num_constraints; }
uint32_t pk_count_hash_gates(const GateDev *host_gates, uint32_t num_gates) {
    uint32_t n = 0;
    for (u32 i = 0; i < num_gates; i++) if (is_hash_gate(host_gates[i])) n++;
    return n;
}
static qfold::Schedule hash_gate_schedule(const QuotientArgs &a, const GateDev &g) {
    return g.type == GATE_POSEIDON ? qfold::poseidon_schedule() : qfold::poseidon2_schedule(a.p2_layout);
}
// hash gate number `slot` (gate gi of the list): the one call site of the folded and the round-by-round form
template <int NCH>
static void hash_gate_launch(const QuotientArgs &a, const GateDev *host_gates, u32 gi, u32 t0, u32 slot, int finalize, dim3 g, dim3 b, hipStream_t st) {
    const bool p1 = host_gates[gi].type == GATE_POSEIDON;
    const qfold::Schedule s = hash_gate_schedule(a, host_gates[gi]);
    if (a.fold) {
        if (p1) hipLaunchKernelGGL((quotient_poseidon_kernel<NCH>), g, b, 0, st, a, s, gi, t0, slot, finalize);
        else hipLaunchKernelGGL((quotient_poseidon2_kernel<NCH>), g, b, 0, st, a, s, gi, t0, slot, finalize);
    } else {
        if (p1) hipLaunchKernelGGL((quotient_hash_rounds_kernel<NCH, GATE_POSEIDON>), g, b, 0, st, a, s, gi, t0, finalize);
        else hipLaunchKernelGGL((quotient_hash_rounds_kernel<NCH, GATE_POSEIDON2>), g, b, 0, st, a, s, gi, t0, finalize);
    }
}
// the two hash gates of a pairable list: idx[0], idx[1] in gate-list order (their table slots are 0 and 1)
static bool hash_gate_pair(const GateDev *host_gates, u32 num_gates, const P2GateLayout &lay, u32 (&idx)[2]) {
    u32 n = 0;
    for (u32 i = 0; i < num_gates; i++)
        if (is_hash_gate(host_gates[i])) { if (n == 2) return false; idx[n++] = i; }
    if (n != 2) return false;
    auto sched = [&](u32 i) { return host_gates[i].type == GATE_POSEIDON ? qfold::poseidon_schedule() : qfold::poseidon2_schedule(lay); };
    return qfold::pairable(sched(idx[0]), sched(idx[1]));
}
bool pk_quotient_pairable(const GateDev *host_gates, uint32_t num_gates, const P2GateLayout &p2_layout) {
    u32 idx[2];
    return hash_gate_pair(host_gates, num_gates, p2_layout, idx);
}
hipError_t pk_quotient_fold_sweep(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st) {
    if (!a.fold || a.batch == 0) return hipSuccess;
    FoldSweepArgs fa{};
    for (u32 i = 0; i < a.num_gates; i++)
        if (is_hash_gate(host_gates[i])) {
            if (fa.ngates == qfold::MAX_GATES) return hipErrorInvalidValue;
            fa.sched[fa.ngates++] = hash_gate_schedule(a, host_gates[i]);
        }
    if (fa.ngates == 0) return hipSuccess;
    fa.nch = a.nch; fa.nterms = a.nterms; fa.t0 = a.nch + a.nch * a.nchunks; fa.batch = a.batch;
    fa.alpha_pows = a.alpha_pows; fa.poseidon_rc = a.poseidon_rc; fa.p2_gate = a.p2_gate;
    fa.fold = const_cast<u64 *>(a.fold); fa.ps_small = a.ps_small; fa.ps_fold = a.ps_fold;
    hipLaunchKernelGGL(quotient_fold_sweep_kernel, dim3(fa.ngates, fa.nch, fa.batch), dim3(64), 0, st, fa);
    return hipGetLastError();
}
// Which circuits quotient_perm_gates_kernel serves: every gate that carries constraints and is no hash gate is a ConstantGate, a
// PublicInputGate, an ArithmeticGate or a BaseSumGate<2>, one of each at most (the kernel keeps one sum per type), and every wire
// they read is a routed one, i.e. falls into a chunk of the walk: Constant and PublicInput wires into the first four of chunk 0. The chunks are the
// kernel's FUSED_CHUNK wide. The base of a BaseSumGate is not looked at: the loader admits base 2 only as this gate type
// (circuit.cpp). Everything else (the recursion gate set, the extension arithmetic, a wide RandomAccess) keeps the
// two launches.
bool pk_quotient_fused_gates(const GateDev *host_gates, uint32_t num_gates, uint32_t num_routed, uint32_t chunk, uint32_t nchunks, FusedGates *out) {
    FusedGates fg{FUSED_NONE, FUSED_NONE, FUSED_NONE, FUSED_NONE, 0, 0, 0};
    if (chunk != FUSED_CHUNK || num_routed < FUSED_CHUNK || nchunks != (num_routed + FUSED_CHUNK - 1) / FUSED_CHUNK) return false;
    for (u32 i = 0; i < num_gates; i++) {
        const GateDev &g = host_gates[i];
        if (g.num_constraints == 0 || g.type == GATE_POSEIDON || g.type == GATE_POSEIDON2) continue;
        if (g.type == GATE_CONSTANT && fg.constant == FUSED_NONE && g.param0 <= 4) { fg.constant = i; fg.n_consts = g.param0; }
        else if (g.type == GATE_PUBLIC_INPUT && fg.public_input == FUSED_NONE) fg.public_input = i;
        else if (g.type == GATE_ARITHMETIC && fg.arithmetic == FUSED_NONE && g.param0 >= 1 && (uint64_t)4 * g.param0 <= num_routed) { fg.arithmetic = i; fg.n_ops = g.param0; }
        else if (g.type == GATE_BASE_SUM && fg.base_sum == FUSED_NONE && g.param0 >= 1 && (uint64_t)g.param0 + 1 <= num_routed) { fg.base_sum = i; fg.n_limbs = g.param0; }
        else return false;
    }
    if (out) *out = fg;
    return true;
}
// The stage's launches: the permutation terms (perm), every other gate, then the hash gates (heavy, one launch each, or one for
// the two of a folded pair); with `finalize` the last of them also applies 1/Z_H and stores. Without either: the gate sums alone,
// for the witness check.
template <int NCH>
static hipError_t quotient_launch(const QuotientArgs &a, const GateDev *host_gates, bool perm, bool finalize, hipStream_t st) {
    dim3 b(256), g((unsigned)((a.q_n + 255) / 256), 1, a.batch);
    const u32 t0 = a.nch + a.nch * a.nchunks;
    const u32 n_hash = pk_count_hash_gates(host_gates, a.num_gates);
    const int fin_gates = finalize && n_hash == 0;
    FusedGates fg;
    const u32 tiles = g.x;
    const bool grouped = a.fused_plain_map == 0;
    if (perm && a.fused && pk_quotient_fused_gates(host_gates, a.num_gates, a.num_routed, a.chunk, a.nchunks, &fg) &&
        qmap::grid_size(tiles, a.batch, grouped) <= 0x7FFFFFFFull) {
        hipLaunchKernelGGL((quotient_perm_gates_kernel<NCH>), dim3((unsigned)qmap::grid_size(tiles, a.batch, grouped)), b, 0, st, a, fg, tiles, grouped ? 1u : 0u, fin_gates);
    } else {
        if (perm) hipLaunchKernelGGL((quotient_perm_kernel<NCH>), g, b, 0, st, a);
        if (wide_random_access(a, host_gates)) hipLaunchKernelGGL((quotient_gates_kernel<NCH, true>), g, b, 0, st, a, t0, fin_gates);
        else hipLaunchKernelGGL((quotient_gates_kernel<NCH, false>), g, b, 0, st, a, t0, fin_gates);
    }
    u32 pr[2];
    if (a.fold && a.pair && hash_gate_pair(host_gates, a.num_gates, a.p2_layout, pr)) {
        const u32 sa = host_gates[pr[0]].type == GATE_POSEIDON ? 0 : 1;      // the PoseidonGate's table slot
        hipLaunchKernelGGL((quotient_hash_pair_kernel<NCH>), g, b, 0, st, a, pr[sa], pr[sa ^ 1], sa, sa ^ 1, t0, finalize ? 1 : 0);
        return hipGetLastError();
    }
    u32 slot = 0;
    for (u32 i = 0; i < a.num_gates; i++)
        if (is_hash_gate(host_gates[i])) {
            hash_gate_launch<NCH>(a, host_gates, i, t0, slot, finalize && slot + 1 == n_hash, g, b, st);
            slot++;
        }
    return hipGetLastError();
}
static hipError_t quotient_dispatch(const QuotientArgs &a, const GateDev *host_gates, bool perm, bool finalize, hipStream_t st) {
    switch (a.nch) {
        case 1: return quotient_launch<1>(a, host_gates, perm, finalize, st);
        case 2: return quotient_launch<2>(a, host_gates, perm, finalize, st);
        case 3: return quotient_launch<3>(a, host_gates, perm, finalize, st);
        case 4: return quotient_launch<4>(a, host_gates, perm, finalize, st);
        default: return hipErrorInvalidValue;
    }
}
hipError_t pk_quotient(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st) {
    if (a.q_n == 0 || a.batch == 0) return hipSuccess;
    return quotient_dispatch(a, host_gates, true, true, st);
}
hipError_t pk_gate_sums(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st) { return quotient_dispatch(a, host_gates, false, false, st); }
hipError_t pk_witness_check(const u64 *acc, u64 n, u32 nch, const u64 *z, const u64 *rowprod, u64 *result, u32 batch, hipStream_t st) {
    // the launch LAUNCH_1D_B of prover_kernels.hip makes: one thread per row, grid.z = proof, nothing for an empty batch
    if (n > 0 && batch > 0) hipLaunchKernelGGL(witness_check_kernel, dim3((unsigned)((n + 255) / 256), 1, batch), dim3(256), 0, st, acc, n, nch, z, rowprod, result);
    return hipGetLastError();
}

// ---------------------------------------------------------------- s6 on a coset-sharded oracle: the shards' coefficients -> the chunks
// Working shard g of Gq = 2^lq (quotient_shard_map.hpp) leaves B_e[j] = sum_c (q_(j + cM) g_mult^(cM)) w_Gq^(e c), e = brev_lq(g),
// j < M, in block g of `gather` ([Gq][nch][M]). This is the last radix-Gq pass of the size Gq M inverse transform, with the coset
// scaling of the high index folded in: q_(j + cM) = scale[c] sum_e w_Gq^(-e c) B_e[j], scale[c] = g_mult^(-cM) / Gq. tab: [Gq] the
// powers w_Gq^-k, then [Gq] scale. Threads run along j (VEC adjacent ones each, 16-byte accesses at VEC = 2), the challenge is
// grid.y: each of the Gq read streams and the Gq write streams is unit-stride, every word is read once and written once.
namespace {

template <int VEC> struct MergeWord;
template <> struct MergeWord<1> {
    u64 v[1];
    __device__ __forceinline__ void load(const u64 *p) { v[0] = *p; }
    __device__ __forceinline__ void store(u64 *p) const { *p = v[0]; }
};
template <> struct MergeWord<2> {
    u64 v[2];
    __device__ __forceinline__ void load(const u64 *p) { const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(p); v[0] = t.x; v[1] = t.y; }
    __device__ __forceinline__ void store(u64 *p) const { *reinterpret_cast<ulonglong2 *>(p) = make_ulonglong2(v[0], v[1]); }
};

// the Gq values of one j in registers; block g holds exponent brev(g), so the decimation-in-time butterflies run on them as they lie
template <int LQ, int VEC>
__global__ void __launch_bounds__(256) quotient_merge_kernel(const u64 *gather, u64 *out, u64 m, u32 nch, const u64 *tab) {
    constexpr int GQ = 1 << LQ;
    const u64 j = (blockIdx.x * (u64)blockDim.x + threadIdx.x) * VEC;
    if (j >= m) return;
    const u64 ch = blockIdx.y;
    MergeWord<VEC> x[GQ];
#pragma unroll
    for (int g = 0; g < GQ; g++) x[g].load(gather + ((u64)g * nch + ch) * m + j);
#pragma unroll
    for (int s = 1; s <= LQ; s++) {
        const int half = 1 << (s - 1), step = GQ >> s;
#pragma unroll
        for (int k = 0; k < GQ; k += 2 * half)
#pragma unroll
            for (int t = 0; t < half; t++) {
                const u64 w = tab[t * step];
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    const u64 u = x[k + t].v[e], v = t ? gl::mul(x[k + t + half].v[e], w) : x[k + t + half].v[e];
                    x[k + t].v[e] = gl::add(u, v); x[k + t + half].v[e] = gl::sub(u, v);
                }
            }
    }
#pragma unroll
    for (int c = 0; c < GQ; c++) {
        const u64 sc = tab[GQ + c];
#pragma unroll
        for (int e = 0; e < VEC; e++) x[c].v[e] = gl::canon(gl::mul(x[c].v[e], sc));
        x[c].store(out + (ch * GQ + c) * m + j);
    }
}

// any Gq: one output chunk c per grid.z, the Gq-term sum written out (the blocks are read Gq times, through the cache)
__global__ void __launch_bounds__(256) quotient_merge_loop_kernel(const u64 *gather, u64 *out, u64 m, u32 nch, u32 lq, const u64 *tab) {
    const u64 j = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (j >= m) return;
    const u32 gq = 1u << lq, c = blockIdx.z;
    const u64 ch = blockIdx.y;
    u64 sum = 0;
    for (u32 e = 0; e < gq; e++) {
        const u32 g = brev32(e, lq);
        sum = gl::add(sum, gl::mul(gather[((u64)g * nch + ch) * m + j], tab[(e * c) & (gq - 1)]));
    }
    out[(ch * gq + c) * m + j] = gl::canon(gl::mul(sum, tab[gq + c]));
}

template <int LQ>
void merge_launch(const u64 *gather, u64 *out, u64 m, u32 nch, const u64 *tab, hipStream_t st) {
    // two adjacent j per thread where both ends allow 16-byte accesses: m is even, so every row then starts aligned
    const bool vec = m % 2 == 0 && (((uintptr_t)gather | (uintptr_t)out) & 15) == 0;
    const u64 threads = vec ? m / 2 : m;
    dim3 b(256), g((unsigned)((threads + 255) / 256), nch);
    if (vec) hipLaunchKernelGGL((quotient_merge_kernel<LQ, 2>), g, b, 0, st, gather, out, m, nch, tab);
    else hipLaunchKernelGGL((quotient_merge_kernel<LQ, 1>), g, b, 0, st, gather, out, m, nch, tab);
}

}  // namespace

hipError_t pk_quotient_merge(const u64 *gather, u64 *out, u64 m, u32 nch, u32 lq, const u64 *tab, hipStream_t st) {
    if (m == 0 || nch == 0 || lq == 0 || lq > 8) return hipErrorInvalidValue;   // quotient_degree_factor <= 256 (circuit.cpp)
    switch (lq) {
        case 1: merge_launch<1>(gather, out, m, nch, tab, st); break;
        case 2: merge_launch<2>(gather, out, m, nch, tab, st); break;
        case 3: merge_launch<3>(gather, out, m, nch, tab, st); break;
        default:
            hipLaunchKernelGGL(quotient_merge_loop_kernel, dim3((unsigned)((m + 255) / 256), nch, 1u << lq), dim3(256), 0, st, gather, out, m, nch, lq, tab);
    }
    return hipGetLastError();
}
