// challenger.hpp — the duplex sponge of the Fiat-Shamir transcript on the host (plonky2::iop::challenger::Challenger), one
// definition for the prover (prover.cpp, fri_prover.cpp, oracle_api.cpp) and the verifier (verifier.cpp). Host only.
#pragma once
#include <cstring>
#include "../../include/qpgpu.h"
#include "gl64.hpp"
#include "poseidon.hpp"

struct Challenger {
    const hasher::Config *h;
    gl::u64 state[12] = {0};
    gl::u64 in[8]; int n_in = 0;
    gl::u64 out[8]; int n_out = 0;
    explicit Challenger(const hasher::Config &cfg) : h(&cfg) {}
    void duplex() {
        for (int i = 0; i < n_in; i++) state[i] = in[i];
        n_in = 0;
        h->permute(state);
        std::memcpy(out, state, sizeof out);
        n_out = 8;
    }
    // absorbs the words as they are: the verifier's circuit digest, which comes from the pack unreduced
    void observe_raw(const gl::u64 *x, size_t n) {
        for (size_t i = 0; i < n; i++) { n_out = 0; in[n_in++] = x[i]; if (n_in == 8) duplex(); }
    }
    void observe(const gl::u64 *x, size_t n) {
        for (size_t i = 0; i < n; i++) { const gl::u64 c = gl::canon(x[i]); observe_raw(&c, 1); }
    }
    gl::u64 get() { if (n_in > 0 || n_out == 0) duplex(); return out[--n_out]; }
    gl::e2 get_ext() { gl::u64 a = get(), b = get(); return gl::e2_make(a, b); }
};

// ---- qpgpu_challenger (include/qpgpu.h: the transcript as plain data) <-> Challenger, for the entries that take a transcript ----
// plonky2 never holds a full input buffer (a duplex runs when the eighth element arrives) nor more than eight outputs: a
// state that says otherwise is invalid input
inline bool challenger_to_host(const qpgpu_challenger *c, Challenger &ch) {
    if (c->input_len >= 8 || c->output_len > 8) return false;
    std::memcpy(ch.state, c->sponge_state, sizeof ch.state);
    ch.n_in = (int)c->input_len; ch.n_out = (int)c->output_len;
    std::memcpy(ch.in, c->input_buffer, sizeof ch.in);
    std::memcpy(ch.out, c->output_buffer, sizeof ch.out);
    return true;
}
inline void challenger_from_host(const Challenger &ch, qpgpu_challenger *c) {
    std::memcpy(c->sponge_state, ch.state, sizeof ch.state);
    std::memset(c->input_buffer, 0, sizeof c->input_buffer); std::memset(c->output_buffer, 0, sizeof c->output_buffer);
    for (int i = 0; i < ch.n_in; i++) c->input_buffer[i] = ch.in[i];
    for (int i = 0; i < ch.n_out; i++) c->output_buffer[i] = ch.out[i];
    c->input_len = (uint32_t)ch.n_in; c->output_len = (uint32_t)ch.n_out;
}
