// verify_kernels.hpp — launch interface of the query-round kernels of batch verification (verify_kernels.hip, driven by
// verify_device.cpp). A proof of a circuit has one layout (proof_layout.hpp), so every opening of every query round
// sits at a byte offset that depends only on (query, oracle or FRI round): the host describes it once per call in VerifyLayout.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "circuit.hpp"
#include "fri_verify.hpp"
#include "merkle.hpp"

// one Merkle opening of a query round: the four initial oracles, then one per FRI round
struct VerifyOpening {
    uint32_t off;       // byte offset of the opened row from the start of its query round
    uint32_t width;     // row words (salt included); the path-length byte follows the row, the path the byte
    uint32_t plen;      // the path length of the layout (log2 leaves - cap height)
    uint32_t shift;     // leaf index = x_index >> shift
    uint32_t cap_off;   // byte offset of the cap in the proof; VERIFY_CAP_VERIFIER: the verifier's constants/sigmas cap
};
constexpr uint32_t VERIFY_CAP_VERIFIER = 0xFFFFFFFFu;
constexpr int VERIFY_MAX_ROUNDS = 16;

struct VerifyLayout {
    uint32_t nq;                // query rounds per proof
    uint32_t n_open;            // 4 + FRI rounds
    uint32_t queries_pos;       // byte offset of query round 0
    uint32_t q_bytes;           // bytes of one query round
    uint32_t final_off;         // byte offset of the final polynomial
    uint32_t final_n;           // its coefficients (extension elements)
    uint32_t stride_words;      // words between two proofs in the device buffer (>= one word of padding behind a proof)
    uint32_t rec_words;         // words of a per-proof record (below)
    uint32_t log_lde;           // log2 of the LDE size
    uint32_t nch;               // num_challenges
    uint32_t polys[4];          // opened polynomials per initial oracle (the salt columns are not opened)
    uint32_t arity_bits[VERIFY_MAX_ROUNDS];
    VerifyOpening op[4 + VERIFY_MAX_ROUNDS];
};

// per-proof record, words: [0] 1 = verify this proof, 0 = skip it (decided on the host); then zeta, g zeta, FRI alpha,
// alpha^num_challenges, the two reduced openings (extension elements, two words each); the FRI betas; the query indices
enum : uint32_t { VREC_LIVE = 0, VREC_ZETA = 1, VREC_GZETA = 3, VREC_ALPHA = 5, VREC_ALPHA_NCH = 7, VREC_RED0 = 9, VREC_RED1 = 11, VREC_BETAS = 13 };
inline uint32_t vrec_words(uint32_t rounds, uint32_t nq) { return VREC_BETAS + 2 * rounds + nq; }

// the verdict codes of a query round (VQ_*): fri_verify.hpp, shared with the host loop

hipError_t verify_upload_constants(const uint64_t *rc360);   // plonky2 Poseidon round constants of this unit (merkle_upload_constants)
// proofs: nproofs x stride_words; recs: nproofs x rec_words; mcodes: nproofs x nq x n_open bytes (scratch); qcodes: nproofs x nq
hipError_t verify_query_rounds(const VerifyLayout &lay, const uint64_t *proofs, const uint64_t *recs, const uint64_t *cs_cap, uint32_t nproofs,
                               uint8_t *mcodes, uint32_t *qcodes, const HasherDev &h, hipStream_t st);

// ---- the head of verification on the device (verify_head_kernels.hip): transcript, proof of work, quotient identity ----
// What the head reads of a proof, stated once per call from proof_layout.hpp and the pack. Byte offsets below queries_pos are
// multiples of 8 (caps and extension elements only); final_pos and what follows it need not be (a query round holds single bytes).
struct HeadLayout {
    uint32_t cap_words;             // words of one Merkle cap
    uint32_t n_rounds;              // FRI rounds
    uint32_t open_pos[7], open_cnt[7];   // byte offset / extension elements: constants, sigmas, wires, zs, zs_next, partial products, quotient
    uint32_t fri_caps_pos, final_pos, pow_pos, pis_pos, n_pis, total;
    uint32_t degree_bits, pow_bits;
    uint32_t num_selectors, num_constants, num_routed, num_pp, qdf;      // qdf: quotient_degree_factor
    uint32_t n_gates, n_slots;      // identity kernel: slot 0 = permutation argument, 1 + g = gate g, n_gates + 1 = quotient side and reduced openings
    uint32_t gate_term0;            // index of the first gate constraint among the terms the alphas reduce
    uint32_t pack_bad;              // the pack's gate table is inconsistent (the host's message goes to every proof past the proof of work)
    uint32_t hrec_words;
    uint64_t digest[4];             // circuit digest, absorbed unreduced
    P2GateLayout p2;
};
// per-proof head record, words: the head verdict, then betas, gammas, alphas (four slots each) and the public-input hash
enum : uint32_t { HREC_CODE = 0, HREC_BETAS = 1, HREC_GAMMAS = 5, HREC_ALPHAS = 9, HREC_PIH = 13, HREC_WORDS = 17 };
// head verdict: 0 = passed; kind << 8 | challenge
enum : uint32_t { VH_NONCANONICAL = 1, VH_POW = 2, VH_PACK = 3, VH_QUOTIENT = 4 };
constexpr uint32_t VERIFY_PARTIAL_WORDS = 8;    // one identity-kernel slot: an extension element per challenge (at most four)

// the gate tables of this unit (plonky2's Poseidon constants and fast partial rounds, qp-poseidon-core's Poseidon2 set) and the
// hashing constants of its permutation plugs; once per device (merkle_upload_constants)
hipError_t verify_head_upload_constants(const uint64_t *rc360);
// table: n_gates GateInfo (8 words each), then k_is. recs: VREC_LIVE set by the host, the rest written here; a proof the head
// rejects leaves with VREC_LIVE = 0 and its verdict in hcodes. hrecs: nproofs x HREC_WORDS; partials: nproofs x n_slots x
// VERIFY_PARTIAL_WORDS. The three launches are separate calls so that a profile can tell them apart.
hipError_t verify_head_transcript(const VerifyLayout &lay, const HeadLayout &hl, const uint64_t *proofs, uint64_t *recs, uint64_t *hrecs,
                                  uint32_t nproofs, const HasherDev &h, hipStream_t st);
hipError_t verify_head_identity(const VerifyLayout &lay, const HeadLayout &hl, const uint64_t *proofs, uint64_t *recs, const uint64_t *hrecs,
                                const uint64_t *table, uint64_t *partials, uint32_t nproofs, hipStream_t st);
hipError_t verify_head_verdict(const VerifyLayout &lay, const HeadLayout &hl, uint64_t *recs, const uint64_t *hrecs, const uint64_t *partials,
                               uint32_t *hcodes, uint32_t nproofs, hipStream_t st);
