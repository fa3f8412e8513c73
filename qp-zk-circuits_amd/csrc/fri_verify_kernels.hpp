// fri_verify_kernels.hpp — launch interface of the query-round kernels of qpgpu_fri_verify_many_device (fri_verify_kernels.hip,
// driven by fri_verify_device.cpp): VerifyLayout (verify_kernels.hpp) without the Plonk proof in it. The proofs of one instance
// have one layout, so every opening of every query round sits at a byte offset that depends only on (query, oracle or round);
// the host states it once per call. No kernel takes a length or an offset from proof bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "merkle.hpp"

constexpr int FV_MAX_ORACLES = 16, FV_MAX_ROUNDS = 16, FV_MAX_BATCHES = 8, FV_MAX_RANGES = 8;

// one Merkle opening of a query round: the initial oracles, then one per FRI round
struct FvOpening {
    uint32_t off;         // byte offset of the opened row from the start of its query round
    uint32_t width;       // row words (salt included); the path-length byte follows the row, the path the byte
    uint32_t plen;        // the path length of the layout (log2 leaves - cap height): the loop bound
    uint32_t shift;       // leaf index = x_index >> shift
    uint32_t cap_off;     // words: a round's cap from the start of its proof; an oracle's cap from the start of the cap area
    uint32_t cap_stride;  // an oracle's cap: words from one proof's to the next (0: shared by all proofs); FV_CAP_IN_PROOF: a round's
};
constexpr uint32_t FV_CAP_IN_PROOF = 0xFFFFFFFFu;

// FriPolynomialInfo::from_range as the consistency kernel reads it
struct FvRange { uint32_t row_off, count; };      // byte offset of polynomial `first` of its oracle's row in the query round
struct FvBatch { uint32_t num_ranges; FvRange ranges[FV_MAX_RANGES]; };

struct FvLayout {
    uint32_t nq;                // query rounds per proof
    uint32_t n_oracles, n_rounds, n_batches;
    uint32_t queries_pos;       // byte offset of query round 0 in a proof
    uint32_t q_bytes;           // bytes of one query round
    uint32_t final_off;         // byte offset of the final polynomial
    uint32_t final_n;           // its coefficients (extension elements)
    uint32_t stride_words;      // words between two proofs in the device buffer (>= one word of padding behind a proof)
    uint32_t rec_words;         // words of a per-proof record (below)
    uint32_t log_lde;
    uint32_t arity_bits[FV_MAX_ROUNDS];
    FvOpening op[FV_MAX_ORACLES + FV_MAX_ROUNDS];
    FvBatch batch[FV_MAX_BATCHES];
};

// per-proof record, words: [0] 1 = verify this proof, 0 = skip it (decided on the host); alpha; per batch the point, the reduced
// openings and alpha^(polynomials of the batch) (extension elements, two words each); the betas; the query indices (range-checked
// on the host)
enum : uint32_t { FREC_LIVE = 0, FREC_ALPHA = 1, FREC_BATCHES = 3, FREC_BATCH_WORDS = 6 };
constexpr uint32_t frec_betas(uint32_t batches) { return FREC_BATCHES + FREC_BATCH_WORDS * batches; }     // host and device
constexpr uint32_t frec_words(uint32_t batches, uint32_t rounds, uint32_t nq) { return frec_betas(batches) + 2 * rounds + nq; }

hipError_t fri_verify_upload_constants(const uint64_t *rc360);   // plonky2 Poseidon round constants of this unit (merkle_upload_constants)
// proofs: nproofs x stride_words; recs: nproofs x rec_words; caps: the initial oracles' caps; mcodes: nproofs x nq x (oracles +
// rounds) bytes (scratch); qcodes: nproofs x nq, the codes of verify_kernels.hpp (VQ_*)
hipError_t fri_verify_query_rounds(const FvLayout &lay, const uint64_t *proofs, const uint64_t *recs, const uint64_t *caps, uint32_t nproofs,
                                   uint8_t *mcodes, uint32_t *qcodes, const HasherDev &h, hipStream_t st);
