// verify_kernels.hpp — launch interface of the query-round kernels of batch verification (verify_kernels.hip, driven by
// verify_device.cpp). A proof of a circuit has one layout (proof_layout.hpp), so every opening of every query round
// sits at a byte offset that depends only on (query, oracle or FRI round): the host describes it once per call in VerifyLayout.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
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

// first failing check of a query round, in the host verifier's order: code = kind << 8 | oracle or round; 0 = accepted
enum : uint32_t { VQ_ORACLE_PLEN = 1, VQ_ORACLE_PATH = 2, VQ_ROUND_PLEN = 3, VQ_ROUND_CONT = 4, VQ_ROUND_PATH = 5, VQ_FINAL = 6 };

hipError_t verify_upload_constants(const uint64_t *rc360);   // plonky2 Poseidon round constants of this unit (merkle_upload_constants)
// proofs: nproofs x stride_words; recs: nproofs x rec_words; mcodes: nproofs x nq x n_open bytes (scratch); qcodes: nproofs x nq
hipError_t verify_query_rounds(const VerifyLayout &lay, const uint64_t *proofs, const uint64_t *recs, const uint64_t *cs_cap, uint32_t nproofs,
                               uint8_t *mcodes, uint32_t *qcodes, const HasherDev &h, hipStream_t st);
