// quotient_fold.hpp — the hash gates of the quotient stage with their linear layers folded into the alpha weights.
//
// In PoseidonGate and in the Poseidon2 gate every S-box input but the first round's is a wire, and every state that leaves a
// linear layer (matrix, then round constants) meets nothing but an affine constraint `state - wire` before a wire replaces it
// (lanes 1..11 of a partial round: before it runs on through further linear layers). The alpha-weighted constraint sum of a
// gate at one point is therefore affine in the S-box outputs y_s and the target wires W_k,
//     sum_q alpha^q c_q = sum_s omega_s y_s - sum_k alpha^(q_k) W_k + kappa + (swap / delta terms, kept as they are),
// with omega and kappa functions of alpha and the gate's constants alone. They come from one backward (adjoint) walk over the
// linear layers: lambda starts as the alpha powers of the output constraints; through a layer lambda <- L^T lambda and
// kappa += lambda . rc; where a lane was replaced by a wire, omega of the S-box behind that wire is the incoming lambda and
// the lane's lambda restarts at the alpha power of that wire's constraint. One walk per (proof, challenge, hash gate) and
// lockstep batch; the per-point kernel then computes S-boxes and weighted sums only (quotient_kernels.hip).
//
// ONE description of the round structure (Schedule, seg_*) serves the backward walk (sweep), the forward walk it is the adjoint
// of (walk: the round-by-round form of the constraints, the fold's A/B partner under QPGPU_QUOTIENT_FOLD=0), the per-point kernels
// (quotient_kernels.hip) and the host form of the folded sum (folded_sum); walk and folded_sum are checked against verify_math.hpp
// by tools/host_checks/quotient_fold_check.cpp. L^T is taken from the forward layers themselves (their images of the unit
// vectors), so a change there cannot drift from here.
#pragma once
#include "circuit.hpp"
#include "gl64.hpp"
#include "poseidon.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define QFOLD_UNROLL _Pragma("unroll")
#else
#define QFOLD_UNROLL
#endif

namespace qfold {
using gl::u32;
using gl::u64;

enum Lin : u32 { LIN_MDS = 0, LIN_P2_EXT = 1, LIN_P2_INT = 2 };
// what enters the first linear layer of the walk: the first round's S-box outputs (inputs computed from the gate's input wires),
// or, for a Poseidon2 layout that records round 0's S-box inputs too, the (swapped) inputs themselves through the initial layer
enum Head : u32 { HEAD_SBOX = 0, HEAD_RAW = 1 };

// Segment k = one linear layer, the constants added after it, and the constraints that follow (12 lanes, or lane 0 in the
// partial rounds). round(k) counts from the layer behind the first S-boxes: 0..2 first-half full rounds, 3..24 the layers in
// front of the 22 partial-round constraints, 25..28 in front of the second half's, 29 in front of the outputs; -1 is HEAD_RAW's
// initial layer. The target wires are numbered in constraint order (j = 0..nw-1, constraint q0 + j), the outputs follow.
struct Schedule {
    u32 kind;                       // GATE_POSEIDON or GATE_POSEIDON2
    u32 head;
    u32 q0;                         // constraints in front of the first target wire: swap boolean and four deltas, or none
    u32 nw;                         // S-box-input wires: 106, or 118 with round 0 recorded
    u32 nseg;                       // linear layers of the walk: 30 or 31
    u32 run_wire[3], run_len[3];    // the target wires as three runs: first-half full rounds, partial rounds, second half
    u32 w_input, w_output, w_swap, w_delta;
};
constexpr u32 NO_SWAP = P2GateLayout::NO_SWAP;
// per (hash gate, challenge) table: omega of the head values, omega of the wire S-boxes, -alpha^q of targets and outputs, kappa
constexpr u32 T_HEAD = 0, T_OMEGA = 12, T_NALPHA = 130, T_KAPPA = 260, WORDS = 264;
constexpr u32 MAX_GATES = 2;        // hash gates of one circuit that get a table (PoseidonGate, Poseidon2 gate)

GL_HD Schedule poseidon_schedule() {
    Schedule s{};
    s.kind = GATE_POSEIDON; s.head = HEAD_SBOX; s.q0 = 5; s.nw = 106; s.nseg = 30;
    s.run_wire[0] = 29; s.run_len[0] = 36; s.run_wire[1] = 65; s.run_len[1] = 22; s.run_wire[2] = 87; s.run_len[2] = 48;
    s.w_input = 0; s.w_output = 12; s.w_swap = 24; s.w_delta = 25;
    return s;
}
inline Schedule poseidon2_schedule(const P2GateLayout &lay) {
    Schedule s{};
    s.kind = GATE_POSEIDON2; s.head = lay.first_round_wires ? HEAD_RAW : HEAD_SBOX; s.q0 = lay.has_swap() ? 5 : 0;
    s.run_wire[0] = lay.w_full0; s.run_len[0] = 12 * lay.full0_rounds(); s.run_wire[1] = lay.w_partial; s.run_len[1] = 22;
    s.run_wire[2] = lay.w_full1; s.run_len[2] = 48;
    s.nw = s.run_len[0] + 70; s.nseg = lay.first_round_wires ? 31 : 30;
    s.w_input = lay.w_input; s.w_output = lay.w_output; s.w_swap = lay.w_swap; s.w_delta = lay.w_delta;
    return s;
}

// Two hash gates whose sums one pass over the wires can form together (quotient_hash_pair_kernel): a PoseidonGate and a Poseidon2
// gate, both with their first S-boxes computed from the inputs, on the same wires in the same constraint order. Then the swap and
// delta constraints, the target wires with their S-boxes and the -alpha^q weights of targets and outputs (T_NALPHA) are the same
// for both, and the Poseidon2 gate's layout is PoseidonGate's (poseidon_schedule is the only one that gate has); omega, kappa, the
// twelve head S-boxes and the filter stay each gate's own. Anything else (no swap, round 0 on wires, one hash gate) is not a pair.
GL_HD bool pairable(const Schedule &a, const Schedule &b) {
    if (!((a.kind == GATE_POSEIDON && b.kind == GATE_POSEIDON2) || (a.kind == GATE_POSEIDON2 && b.kind == GATE_POSEIDON))) return false;
    if (a.head != HEAD_SBOX || b.head != HEAD_SBOX || a.q0 != b.q0 || a.nw != b.nw) return false;
    for (int r = 0; r < 3; r++) if (a.run_wire[r] != b.run_wire[r] || a.run_len[r] != b.run_len[r]) return false;
    return a.w_input == b.w_input && a.w_output == b.w_output && a.w_swap == b.w_swap && a.w_delta == b.w_delta;
}

struct Consts { const u64 *rc; const poseidon2::Params *p2; };   // PoseidonGate's 360 round constants; the Poseidon2 gate's set

GL_HD int seg_round(const Schedule &s, int k) { return k - (s.head == HEAD_RAW ? 1 : 0); }
GL_HD u32 seg_targets(const Schedule &s, int k) { const int r = seg_round(s, k); return r >= 3 && r <= 24 ? 1u : 12u; }
GL_HD u32 seg_lin(const Schedule &s, int k) {
    if (s.kind == GATE_POSEIDON) return LIN_MDS;
    const int r = seg_round(s, k);
    return r >= 4 && r <= 25 ? LIN_P2_INT : LIN_P2_EXT;
}
// the constant added to lane i behind segment k's layer (canonical). The indices are formed unsigned: none is negative, and the
// compiler need not prove it at every call site to spare the sign extension
GL_HD u64 seg_rc(const Schedule &s, const Consts &c, int k, int i) {
    const int r = seg_round(s, k);
    if (r == 29) return 0;
    if (s.kind == GATE_POSEIDON) return c.rc[(u32)((r + 1) * 12 + i)];
    if (r < 3) return c.p2->rc_ext[(u32)((r + 1) * 12 + i)];
    if (r < 25) return i == 0 ? c.p2->rc_int[(u32)(r - 3)] : 0;
    return c.p2->rc_ext[(u32)((r - 21) * 12 + i)];
}
GL_HD void apply_lin(u32 lin, u64 (&x)[12], const Consts &c) {
    if (lin == LIN_MDS) poseidon::mds_layer(x);
    else if (lin == LIN_P2_EXT) poseidon2::ext_layer_qp(x);
    else poseidon2::int_layer(x, *c.p2);
}
GL_HD u32 target_wire(const Schedule &s, u32 j) {
    if (j < s.run_len[0]) return s.run_wire[0] + j;
    j -= s.run_len[0];
    return j < s.run_len[1] ? s.run_wire[1] + j : s.run_wire[2] + (j - s.run_len[1]);
}
// the inputs of the head's S-boxes from the (swapped) gate inputs; HEAD_RAW: the inputs stay as they are (and get no S-box)
GL_HD void head_inputs(const Schedule &s, const Consts &c, u64 (&st)[12]) {
    if (s.kind == GATE_POSEIDON) {
        QFOLD_UNROLL
        for (int i = 0; i < 12; i++) st[i] = gl::add(st[i], c.rc[i]);
    } else if (s.head == HEAD_SBOX) {
        poseidon2::ext_layer_qp(st);
        QFOLD_UNROLL
        for (int i = 0; i < 12; i++) st[i] = gl::add(st[i], c.p2->rc_ext[i]);
    }
}

// Scratch of one walk (LDS on the device): the layers' columns, the constants behind every layer and the alpha powers of the
// gate's targets (staged once, so that no step of the walk waits for global memory), lambda (double buffered), the four partial
// sums of a step's twelve dot products, and the per-lane parts of kappa.
constexpr u32 MAX_SEG = 31, MAX_TARGETS = 130, SWEEP_LANES = 48;
struct Scratch { u64 cols[3 * 144], rc[MAX_SEG * 12], ap[MAX_TARGETS], lam[24], part[SWEEP_LANES], kap[12]; };

// The backward walk for one challenge. ap = that challenge's alpha powers from the gate constraints' first index on. The work is
// written as loops `t = tid, tid + nthreads, ...` over its items, with `barrier` between dependent phases: a device block runs it
// with one thread per item (nthreads >= SWEEP_LANES, __syncthreads; every thread calls the barrier equally often), the host with
// tid 0 of 1 and no barrier. A step's 144 products are spread over 48 items: item (part, lane) sums three of lane's twelve.
template <class Barrier>
GL_HD void sweep(const Schedule &s, const Consts &c, const u64 *ap, Scratch &w, u64 *table, u32 tid, u32 nthreads, Barrier barrier) {
    for (u32 t = tid; t < s.nseg * 12; t += nthreads) w.rc[t] = seg_rc(s, c, (int)(t / 12), (int)(t % 12));
    for (u32 t = tid; t < s.nw + 12; t += nthreads) {
        const u64 a = ap[s.q0 + t];
        w.ap[t] = a;
        table[T_NALPHA + t] = gl::canon(gl::neg(a));
    }
    for (u32 t = tid; t < 36; t += nthreads) {
        const u32 lin = t / 12, j = t % 12;
        if ((s.kind == GATE_POSEIDON) != (lin == LIN_MDS)) continue;
        u64 e[12];
        for (u32 i = 0; i < 12; i++) e[i] = i == j ? 1 : 0;
        apply_lin(lin, e, c);
        for (u32 i = 0; i < 12; i++) w.cols[(lin * 12 + j) * 12 + i] = gl::canon(e[i]);
    }
    for (u32 t = tid; t < 12; t += nthreads) { w.lam[t] = ap[s.q0 + s.nw + t]; w.kap[t] = 0; }
    barrier();
    u32 cur = 0, sc = s.nw;      // sc: target wires not yet passed
    for (int k = (int)s.nseg - 1; k >= 0; k--) {
        const u32 lin = seg_lin(s, k), np = k ? seg_targets(s, k - 1) : 0;
        const u64 *l = w.lam + 12 * cur;
        u64 *next = w.lam + 12 * (cur ^ 1);
        for (u32 t = tid; t < SWEEP_LANES; t += nthreads) {
            const u32 part = t / 12, j = t % 12;
            const u64 *col = w.cols + (lin * 12 + j) * 12;
            gl::Acc192 a = gl::acc_zero();
            for (u32 i = 3 * part; i < 3 * part + 3; i++) gl::acc_mul(a, l[i], col[i]);
            w.part[t] = gl::acc_reduce(a);
        }
        barrier();
        for (u32 j = tid; j < 12; j += nthreads) {
            w.kap[j] = gl::add(w.kap[j], gl::mul(l[j], w.rc[k * 12 + j]));
            const u64 mu = gl::canon(gl::add(gl::add(w.part[j], w.part[12 + j]), gl::add(w.part[24 + j], w.part[36 + j])));
            if (k == 0) table[T_HEAD + j] = mu;
            else if (j < np) { table[T_OMEGA + sc - np + j] = mu; next[j] = w.ap[sc - np + j]; }
            else next[j] = mu;
        }
        sc -= np; cur ^= 1;
        barrier();
    }
    if (tid == 0) {
        u64 kappa = 0;
        for (int i = 0; i < 12; i++) kappa = gl::add(kappa, w.kap[i]);
        table[T_KAPPA] = gl::canon(kappa);
    }
}

// The hash gates' prologue: the swap boolean (constraint 0), the four delta constraints (1..4) and the state that enters the
// permutation, its first two groups of four swapped by the deltas; without a swap wire the inputs as they are. read(wire) gives a
// wire's value at the point, emit(q, c) takes constraint q of the gate.
template <class Read, class Emit>
GL_HD void swapped_inputs(const Schedule &s, Read read, Emit emit, u64 (&st)[12]) {
    if (s.w_swap != NO_SWAP) {
        const u64 swap = read(s.w_swap);
        emit(0u, gl::mul(swap, gl::sub(swap, 1)));
        QFOLD_UNROLL
        for (int i = 0; i < 4; i++) {
            const u64 lhs = read(s.w_input + i), rhs = read(s.w_input + 4 + i), delta = read(s.w_delta + i);
            emit(1u + i, gl::sub(gl::mul(swap, gl::sub(rhs, lhs)), delta));
            st[i] = gl::add(lhs, delta); st[i + 4] = gl::sub(rhs, delta);
        }
    } else {
        QFOLD_UNROLL
        for (int i = 0; i < 8; i++) st[i] = read(s.w_input + i);
    }
    QFOLD_UNROLL
    for (int i = 8; i < 12; i++) st[i] = read(s.w_input + i);
}

// The forward walk, of which sweep is the adjoint: every constraint of the gate at one point, round by round. Behind each layer
// and its constants the target lanes meet their wires (`state - wire`, constraint q0 + j in the order of target_wire, the last
// segment's the twelve outputs); the wire replaces the lane and goes through the S-box.
template <class Read, class Emit>
GL_HD void walk(const Schedule &s, const Consts &c, Read read, Emit emit) {
    u64 st[12];
    swapped_inputs(s, read, emit, st);
    head_inputs(s, c, st);
    if (s.head == HEAD_SBOX) poseidon::sbox7_layer(st);
    u32 j = 0;
    for (int k = 0; k < (int)s.nseg; k++) {
        apply_lin(seg_lin(s, k), st, c);
        const bool last = k == (int)s.nseg - 1;
        const u32 nt = seg_targets(s, k);
        QFOLD_UNROLL
        for (int i = 0; i < 12; i++) {      // the lane index stays a compile-time constant: the state lives in registers
            st[i] = gl::add(st[i], seg_rc(s, c, k, i));
            if ((u32)i >= nt) continue;
            const u64 w = read(last ? s.w_output + i : target_wire(s, j + i));
            emit(s.q0 + j + i, gl::sub(st[i], w));
            if (!last) st[i] = poseidon::sbox7_lane(w);
        }
        j += nt;
    }
}

// The folded sum at one point in plain arithmetic: what the per-point kernels compute (there with grouped S-box products and
// 192-bit accumulators). row = the wire values at the point, ap and table as in sweep.
GL_HD u64 folded_sum(const Schedule &s, const Consts &c, const u64 *row, const u64 *ap, const u64 *table) {
    u64 sum = table[T_KAPPA], st[12];
    swapped_inputs(s, [&](u32 w) { return row[w]; }, [&](u32 q, u64 cst) { sum = gl::add(sum, gl::mul(ap[q], cst)); }, st);
    head_inputs(s, c, st);
    for (int i = 0; i < 12; i++) sum = gl::add(sum, gl::mul(table[T_HEAD + i], s.head == HEAD_SBOX ? poseidon::sbox7(st[i]) : st[i]));
    for (u32 j = 0; j < s.nw; j++) {
        const u64 v = row[target_wire(s, j)];
        sum = gl::add(sum, gl::add(gl::mul(table[T_OMEGA + j], poseidon::sbox7(v)), gl::mul(table[T_NALPHA + j], v)));
    }
    for (int i = 0; i < 12; i++) sum = gl::add(sum, gl::mul(table[T_NALPHA + s.nw + i], row[s.w_output + i]));
    return gl::canon(sum);
}

// The filtered sums of a pairable pair of gates at one point in plain arithmetic: what quotient_hash_pair_kernel computes. The
// linear part (swap and delta constraints, targets and outputs by -alpha^q) and every target wire's S-box are formed once and
// serve both gates; T_NALPHA is read from gate a's table alone (equal in b's: both copy the same alpha powers). fa, fb: the filters.
GL_HD u64 pair_sum(const Schedule &a, const Schedule &b, const Consts &c, const u64 *row, const u64 *ap, const u64 *ta, const u64 *tb, u64 fa, u64 fb) {
    u64 lin = 0, oma = 0, omb = 0, st[12], h[12];
    swapped_inputs(a, [&](u32 w) { return row[w]; }, [&](u32 q, u64 cst) { lin = gl::add(lin, gl::mul(ap[q], cst)); }, st);
    for (int i = 0; i < 12; i++) h[i] = st[i];
    head_inputs(a, c, h);
    for (int i = 0; i < 12; i++) oma = gl::add(oma, gl::mul(ta[T_HEAD + i], poseidon::sbox7(h[i])));
    head_inputs(b, c, st);
    for (int i = 0; i < 12; i++) omb = gl::add(omb, gl::mul(tb[T_HEAD + i], poseidon::sbox7(st[i])));
    for (u32 j = 0; j < a.nw; j++) {
        const u64 v = row[target_wire(a, j)], y = poseidon::sbox7(v);
        lin = gl::add(lin, gl::mul(ta[T_NALPHA + j], v));
        oma = gl::add(oma, gl::mul(ta[T_OMEGA + j], y));
        omb = gl::add(omb, gl::mul(tb[T_OMEGA + j], y));
    }
    for (int i = 0; i < 12; i++) lin = gl::add(lin, gl::mul(ta[T_NALPHA + a.nw + i], row[a.w_output + i]));
    const u64 sa = gl::add(gl::add(oma, lin), ta[T_KAPPA]), sb = gl::add(gl::add(omb, lin), tb[T_KAPPA]);
    return gl::canon(gl::add(gl::mul(fa, sa), gl::mul(fb, sb)));
}

#undef QFOLD_UNROLL
}  // namespace qfold
