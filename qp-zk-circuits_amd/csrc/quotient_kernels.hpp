// quotient_kernels.hpp — argument blocks and launchers of quotient_kernels.hip: stage s6 (the quotient) and the witness check
// that runs its gate kernels on the trace rows. Lockstep batches and the `ps_*` strides as in prover_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "circuit.hpp"
#include "gl64.hpp"
#include "quotient_fold.hpp"

struct GateDev { uint32_t type, param0, param1, selector_index, group_start, group_end, num_constraints, param2; };

struct QuotientArgs {
    const uint64_t *wires, *cs, *zs_pp;   // LDE, column-major, leaf order, stride lde_n
    const uint64_t *x_coset, *l0_coset;   // [lde_n] slot order
    const uint64_t *zh_inv;               // [rate]
    const uint64_t *alpha_pows;           // [nch][nterms]
    const uint64_t *beta_k_is, *betas, *gammas, *pi_hash;
    const GateDev *gates;
    const uint64_t *poseidon_rc;          // 360 round constants (PoseidonGate)
    const poseidon2::Params *p2_gate;     // constants of the Poseidon2 gate (qp-poseidon-core's set), device block
    P2GateLayout p2_layout;               // its wire layout (circuit.hpp)
    uint64_t *acc;                        // [nch][lde_n] slot order: running alpha-weighted sums between the s6 kernels
    uint64_t *out;                        // [nch][lde_n] natural order
    uint64_t lde_n;                       // column stride of the LDE batches (slots)
    uint64_t q_n;                         // points the quotient is evaluated on: the first q_n slots = the coset g<w_{n*qdf}>
    uint32_t q_shift;                     // rate_bits - log2(quotient_degree_factor): natural LDE index >> q_shift = quotient index
    uint32_t log_lde, rate, nch, num_routed, chunk, nchunks, sig0, num_selectors, num_gates, nterms;
    uint32_t batch;
    uint64_t ps_wires, ps_zs, ps_small, ps_acc, ps_out;   // per-proof strides (alpha_pows, beta_k_is, betas, gammas, pi_hash share ps_small)
    // folded hash gates (quotient_fold.hpp): [hash gate in gate-list order][nch][qfold::WORDS] per proof, written by pk_quotient_fold_sweep
    // for this batch's alphas; nullptr = the hash-gate kernel walks the rounds with their linear layers (qfold::walk, the fold's A/B partner)
    const uint64_t *fold;
    uint64_t ps_fold;
    // pk_quotient: 1 = quotient_perm_gates_kernel where the gate list allows it (pk_quotient_fused_gates), 0 = always the two
    // launches; fused_plain_map = 1 gives that kernel the proof-major workgroup order of the (tiles, 1, batch) grids (measurement)
    uint32_t fused, fused_plain_map;
    // 1 = both hash gates from quotient_hash_pair_kernel where they are a pair (pk_quotient_pairable) and fold is set, 0 = one launch each
    uint32_t pair;
};

// the gates quotient_perm_gates_kernel evaluates on its walk: their indices in the gate list (0xFFFFFFFF = the circuit has none)
// and sizes (ConstantGate constants, ArithmeticGate operations, BaseSumGate limbs)
struct FusedGates { uint32_t constant, public_input, arithmetic, base_sum, n_consts, n_ops, n_limbs; };

// the backward walk that fills QuotientArgs::fold: one workgroup per (hash gate, challenge, proof)
struct FoldSweepArgs {
    qfold::Schedule sched[qfold::MAX_GATES];
    uint32_t ngates, nch, nterms, t0, batch;
    const uint64_t *alpha_pows;           // [nch][nterms] per proof, stride ps_small
    const uint64_t *poseidon_rc;
    const poseidon2::Params *p2_gate;
    uint64_t *fold;
    uint64_t ps_small, ps_fold;
};

hipError_t pk_quotient(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st);
// true (and *out, unless nullptr): the circuit's permutation terms and non-hash gates go through quotient_perm_gates_kernel
bool pk_quotient_fused_gates(const GateDev *host_gates, uint32_t num_gates, uint32_t num_routed, uint32_t chunk, uint32_t nchunks, FusedGates *out);
// hash gates of the list that carry constraints; more than qfold::MAX_GATES: the circuit runs without the fold
uint32_t pk_count_hash_gates(const GateDev *host_gates, uint32_t num_gates);
// true: the list holds exactly two hash gates and their schedules are qfold::pairable (one launch serves both, given the fold)
bool pk_quotient_pairable(const GateDev *host_gates, uint32_t num_gates, const P2GateLayout &p2_layout);
// fills a.fold for the batch from its alpha powers (run before pk_quotient / pk_gate_sums whenever QuotientArgs::fold is set)
hipError_t pk_quotient_fold_sweep(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st);
// gate kernels only (no permutation terms, no 1/Z_H): the witness check runs them on the trace rows
hipError_t pk_gate_sums(const QuotientArgs &a, const GateDev *host_gates, hipStream_t st);
// result: [batch][2]
hipError_t pk_witness_check(const uint64_t *acc, uint64_t n, uint32_t nch, const uint64_t *z, const uint64_t *rowprod, uint64_t *result, uint32_t batch, hipStream_t st);

// s6 over a coset-sharded oracle, the home context's step: gather [2^lq][nch][m], block g = working shard g's coefficients (the
// size-m inverse transform of its values, coefficient j times its shift^-j); tab: [2^lq] powers of w_(2^lq)^-1, then [2^lq]
// g_mult^(-c m) / 2^lq. out: [nch][2^lq m], the coefficient chunks as pk_scale_powers leaves them on one context. lq: 1..8
hipError_t pk_quotient_merge(const uint64_t *gather, uint64_t *out, uint64_t m, uint32_t nch, uint32_t lq, const uint64_t *tab, hipStream_t st);

// slot <-> point index of the leaf-ordered LDEs (s6, and the coset tables of prover_kernels.hip)
__device__ __forceinline__ uint32_t brev32(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0; }
