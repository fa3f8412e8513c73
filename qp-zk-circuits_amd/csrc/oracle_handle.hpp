// oracle_handle.hpp — the stage-level ABI's committed polynomial batch (include/qpgpu.h: qpgpu_oracle), shared by the entries
// that create it (oracle_api.cpp) and the ones that read its resident data in place (stage_api.cpp).
#pragma once
#include "prover_host.hpp"

struct qpgpu_oracle {
    qpgpu_ctx *ctx = nullptr;
    PolyOracle o;
    gl::u64 *block = nullptr;     // one allocation: coeffs | lde | digests | salt | eval scratch | salt key
    size_t block_words = 0;
    gl::e2 *d_point = nullptr, *d_eval = nullptr;
    uint32_t *d_key = nullptr;
};
