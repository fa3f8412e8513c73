// fri_prover.hpp — the FRI opening proof (prover_host.hpp: fri_prove) as the steps it is made of, cut where the Fiat-Shamir
// transcript intervenes. fri_prove is the loop over them with its Challenger calls in between; the stage-level ABI
// (fri_api.cpp: qpgpu_fri_session) hands the same steps to a caller who keeps the transcript. One sequence of launches, copies
// and synchronisations, two callers.
//
//   fri_begin            s8: validation, alpha powers, batched opening polynomial; first layer's values (LDE)
//   fri_round_commit     s9, round r: interleave, leaf hash, reduce to the cap, read the cap back (one synchronisation)
//   fri_round_fold       ... fold with the round's betas, then the next layer's values unless it was the last round
//   fri_final_poly       the coefficients left after the last fold (one synchronisation)
//   fri_grind            s10: minimum proof-of-work nonce (independent of a FriState: it needs the transcripts only)
//   fri_gather           s11: rows and paths at the query indices, written as FriQueryRound bytes (one synchronisation)
//
// Everything works on a lockstep batch of nb proofs, as fri_prove does. The order of the steps is FriSteps's (fri_steps.hpp);
// the step functions do not check it, their callers do.
#pragma once
#include "fri_steps.hpp"
#include "prover_host.hpp"

struct FriState {
    qpgpu_ctx *ctx = nullptr;
    FriParams p;                     // num_queries: the most indices one fri_gather takes (the workspace's gather area)
    std::vector<const PolyOracle *> oracles;
    uint32_t nb = 0;
    FriWork *w = nullptr;
    Stager *stage = nullptr;
    // one_call: all steps run inside one call (fri_prove), so "prove_fri_commit" is ONE profile bracket from the first layer's LDE
    // to the final polynomial's read-back; otherwise every step brackets its own part of it
    bool one_call = false;
    FriSteps steps;
    // the round cursor
    gl::u64 *coef = nullptr;         // current coefficients, [2][valid] per proof
    gl::u64 valid = 0, shift = 0;
    unsigned log_len = 0;
    size_t slot = 0;
    std::vector<unsigned> tree_log_leaves;
    std::vector<std::vector<gl::u64>> caps;   // per committed round: [nb][cap_words]
    size_t cap_words() const { return (size_t)4 << p.cap_h; }
    gl::u64 lde_n() const { return 1ull << (p.degree_bits + p.rate_bits); }
};

// alphas: the nb FRI alphas. p.pow_bits is not read. On success `s` is at round 0 with the first layer's values queued.
int fri_begin(qpgpu_ctx *ctx, const FriParams &p, const PolyOracle *const *oracles, size_t n_oracles, const std::vector<FriBatch> &batches,
              uint32_t nb, const gl::e2 *alphas, FriWork &w, Stager &stage, bool one_call, FriState &s);
// the cap lands in s.caps.back() ([nb][cap_words]); stream synchronised
int fri_round_commit(FriState &s);
int fri_round_fold(FriState &s, const gl::e2 *betas);      // betas: [nb], canonical
// out: per proof the component arrays [a_0 .. a_{valid-1}][b_0 .. b_{valid-1}], 2 * s.valid words; stream synchronised
int fri_final_poly(FriState &s, std::vector<gl::u64> &out);
// device tables of the proof-of-work search: [nb][12], [nb], [nb] words
struct PowTables { gl::u64 *states, *bases, *results; };
// per proof the minimum w for which a copy of chs[b], after observe(w), answers get() with pow_bits leading zero bits; chs are
// not modified. pow_bits 0: all zero, no launch.
int fri_grind(qpgpu_ctx *ctx, const Challenger *chs, uint32_t nb, unsigned pow_bits, const PowTables &t, Stager &stage, gl::u64 *witness);
// qidx: [nb][nq] leaf indices below lde_n, nq <= s.p.num_queries. Appends to outs[b] the nq query rounds of proof b in
// write_fri_proof order; stream synchronised.
int fri_gather(FriState &s, const gl::u64 *qidx, uint32_t nq, ByteWriter *outs);
