// oracle_handle.hpp — the stage-level ABI's committed polynomial batch (include/qpgpu.h: qpgpu_oracle), shared by the entries
// that create it (oracle_api.cpp) and the ones that read its resident data in place (stage_api.cpp, fri_api.cpp). The
// qpgpu_challenger <-> Challenger conversion of the entries that take a transcript: challenger.hpp.
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

