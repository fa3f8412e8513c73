// verifier.hpp — the verifier handle and the head of verification (verifier.cpp), shared by the host query loop and the device
// query rounds (verify_device.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "circuit.hpp"
#include "fri_verify.hpp"
#include "gl64.hpp"
#include "poseidon.hpp"
#include "proof_layout.hpp"

struct qpgpu_verifier {
    CircuitPack pack;
    hasher::Config hash;
    std::vector<gl::u64> cs_cap;
    proof_layout::Proof layout;      // byte layout of this circuit's proofs
    std::string pack_why;            // "" or what vanishing_at_zeta finds inconsistent in the pack's gate table (it depends on the pack alone)
    friv::Instance fri;              // the proof's FRI part as an instance: four oracles, everything at zeta, the Zs at g zeta
};

// Everything the query rounds need, as the head of verify_impl leaves it: the transcript replayed through the proof of work,
// the quotient identity checked at zeta, the query indices drawn.
struct VerifyHead {
    std::vector<gl::u64> wires_cap, zs_cap, q_cap, fri_caps;   // 4 << cap_height words each (fri_caps: one per round)
    std::vector<gl::e2> final_poly, fri_betas;
    gl::e2 zeta, g_zeta, fri_alpha, alpha_nch, red0, red1;    // red0 / red1: reduced openings at zeta / g zeta
    std::vector<size_t> x_indices;                            // num_query_rounds
};

// the reason (printf form) into the caller's QPGPU_VERIFY_ERR_CAP bytes, where there are any; returns `code`
namespace verify {
int fail(char *err, int code, const char *fmt, ...);
// the proof system's permutation as the _create entries take it (qpgpu_ctx_set_hasher's kinds); 0 or QPGPU_EINVAL with err
int parse_hasher(int hasher_kind, const uint64_t *hasher_params, size_t n_params, hasher::Config &out, char *err);
bool same_hasher(const hasher::Config &a, const hasher::Config &b);      // a verifier's against a context's, parameter blocks included
}

// 0, or the code and reason the verifier gives for a proof that fails before its query rounds (size, layout, non-canonical
// element, proof of work, quotient identity)
int verify_head(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err, VerifyHead &h);
