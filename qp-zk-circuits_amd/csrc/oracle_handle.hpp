// oracle_handle.hpp — the stage-level ABI's committed polynomial batch (include/qpgpu.h: qpgpu_oracle), shared by the entries
// that create it (oracle_api.cpp) and the ones that read its resident data in place (stage_api.cpp, fri_api.cpp), and the
// qpgpu_challenger <-> Challenger conversion of the entries that take a transcript.
#pragma once
#include "prover_host.hpp"

struct qpgpu_oracle {
    qpgpu_ctx *ctx = nullptr;
    PolyOracle o;
    gl::u64 *block = nullptr;     // one allocation: coeffs | lde | digests | salt | eval scratch | salt keys, each [o.nb][...]
    size_t block_words = 0;
    gl::e2 *d_point = nullptr, *d_eval = nullptr;   // [nb] opening points, [nb][ncols] evaluations
    uint32_t *d_key = nullptr;                      // [nb][8]
};

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
