/*
 * qpgpu_verify.h — proof verification on the host (no GPU): the check every caller of the proving path applies to the proofs
 * it receives and to the proofs it made. SURVEY.md section 8 row f3.
 *
 *   leaf verification at the private batch's commit      wormhole/aggregator/src/private_batch/prover/lib.rs:274-281
 *   private-batch verification at the public batch       wormhole/aggregator/src/public_batch/prover/lib.rs:338-349
 *   self-verification after proving                      wormhole/aggregator/src/aggregator.rs:224-225
 *   WormholeVerifier::verify                             wormhole/verifier/src/lib.rs
 *
 * All of those call qp-plonky2's `VerifierCircuitData::verify` (plonk::verifier::verify_with_challenges +
 * fri::verifier::verify_fri_proof). This is that algorithm over a circuit pack: the Fiat-Shamir transcript replayed, the
 * vanishing polynomial (permutation argument + the selector-filtered constraints of the fourteen gate types) evaluated at
 * zeta in the quadratic extension and compared with Z_H(zeta) * quotient(zeta), the proof-of-work response, and for every
 * query round the Merkle paths of the four initial oracles, the reduced opening, each FRI reduction (coset interpolation at
 * beta) with its Merkle path, and the final polynomial. A verifier is verifier data (constants/sigmas cap + circuit digest +
 * common data), so it is created once per circuit and shared.
 */
#ifndef QPGPU_VERIFY_H
#define QPGPU_VERIFY_H
#include <stddef.h>
#include <stdint.h>
#include "qpgpu.h"      /* qpgpu_fri_params, qpgpu_fri_batch, qpgpu_challenger: the FRI verifier below */

#ifdef __cplusplus
extern "C" {
#endif

#define QPGPU_EVERIFY (-6)        /* the proof is not accepted; err names the first failing check */
#define QPGPU_VERIFY_ERR_CAP 200

typedef struct qpgpu_verifier qpgpu_verifier;

/* pack: the circuit pack (csrc/circuit.hpp). cs_cap: the constants/sigmas Merkle cap, 4 << cap_height words — what
 * qpgpu_circuit_constants_sigmas_cap returns for a loaded circuit (VerifierOnlyCircuitData::constants_sigmas_cap); NULL
 * (cap_words 0): computed here from the pack's constants/sigmas columns on one host core (LDE + Merkle tree: a fraction of a
 * second at 2^10 rows, several seconds at 2^13 — prefer the cap of the GPU handle). hasher_kind / params: the proof system's
 * permutation as in qpgpu_ctx_set_hasher (QPGPU_HASH_POSEIDON, or QPGPU_HASH_POSEIDON2 with a parameter block; NULL, 0
 * selects the built-in qp-poseidon-core set). Returns 0 or QPGPU_EINVAL with the reason in err. */
int qpgpu_verifier_create(const uint64_t *pack_words, size_t n_words, const uint64_t *cs_cap, size_t cap_words, int hasher_kind,
                          const uint64_t *hasher_params, size_t n_params, qpgpu_verifier **out, char *err);
void qpgpu_verifier_free(qpgpu_verifier *v);
size_t qpgpu_verifier_proof_size(const qpgpu_verifier *v);      /* the one length a proof of this circuit has */
/* the verifier data's cap (4 << cap_height words), e.g. to compare with a pinned value */
int qpgpu_verifier_constants_sigmas_cap(const qpgpu_verifier *v, uint64_t *out, size_t out_words);
/* 0: accepted. QPGPU_EVERIFY: rejected, err says why (size, non-canonical element, proof of work, quotient identity,
 * Merkle path of oracle k at query q, FRI round consistency, final polynomial). Thread-safe on a shared verifier. */
int qpgpu_verifier_verify(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err);

/* The FRI query indices of a proof (num_query_rounds words): the transcript replayed up to and including the proof of work,
 * everything it absorbs checked on the way; the query rounds themselves are not looked at, so a proof whose opened rows or
 * Merkle paths were tampered with still yields its indices. They are what a recursive verifier derives in-circuit; a wrapper
 * circuit that checks the Merkle paths only (qpgpu_wrapper_circuit_build, include/qpgpu_batch.h) takes them as inputs. */
int qpgpu_verifier_query_indices(const qpgpu_verifier *v, const uint8_t *proof, size_t len, uint64_t *out, size_t cap, char *err);

/* The same for `count` proofs of the circuit on up to `threads` host threads (0 = all cores): results[i] = 0 or
 * QPGPU_EVERIFY per proof; returns 0 when all are accepted, else QPGPU_EVERIFY with the first rejected proof's index and
 * reason in err. What PrivateBatchProver::commit does to its leaf proofs one after the other. */
int qpgpu_verifier_verify_many(const qpgpu_verifier *v, const uint8_t *const *proofs, const size_t *lens, size_t count, unsigned threads,
                               int *results, char *err);

/* verify_many with the query rounds of every proof on ctx's GPU: Merkle paths of the four initial oracles and of every FRI
 * round, FRI continuation, coset interpolation at beta, final polynomial. The transcript, proof of work and quotient identity
 * run on up to `threads` host threads (0 = all cores). results[i] and the return value / err are exactly what
 * qpgpu_verifier_verify_many would give. reasons: NULL, or count * QPGPU_VERIFY_ERR_CAP bytes; row i receives the text
 * qpgpu_verifier_verify gives for proof i ("" when accepted). The verifier's hasher must equal the context's
 * (qpgpu_ctx_set_hasher), else QPGPU_EINVAL. count == 0 returns 0 at once. A HIP error returns QPGPU_EDEVICE with
 * qpgpu_last_error(ctx) set; the proofs not decided by then get results[i] = QPGPU_EDEVICE (no host fallback). Synchronous on
 * the ctx stream; same threading rule as every ctx call. */
int qpgpu_verifier_verify_many_device(const qpgpu_verifier *v, struct qpgpu_ctx *ctx, const uint8_t *const *proofs, const size_t *lens,
                                      size_t count, unsigned threads, int *results, char *reasons, char *err);

/* The same with flags. flags = 0 is qpgpu_verifier_verify_many_device exactly. QPGPU_VERIFY_HEAD_ON_DEVICE moves the rest of
 * the verification to the GPU as well: canonical check, public-input hash, Fiat-Shamir transcript, proof of work, the
 * vanishing polynomial at zeta against Z_H(zeta) * quotient(zeta), reduced openings and query indices run as kernels, so a
 * proof goes from bytes to verdict without the host reading its contents. The host checks pointer and length, copies each proof
 * into the pinned chunk (`threads` bounds the copying threads only) and puts the verdict codes into the host verifier's words.
 * Verdicts, reasons, return value and err are unchanged: qpgpu_verifier_verify is the specification for both heads. All other
 * rules are those of qpgpu_verifier_verify_many_device; an unknown flag is QPGPU_EINVAL. Meant for callers with few host
 * threads to spare; a proof's transcript is a chain of about 120 dependent permutations, so a small batch may well be slower
 * than with the host head. Its timings have not been measured yet (profiles/verify_device_head.txt). Default off. */
#define QPGPU_VERIFY_HEAD_ON_DEVICE 1u
int qpgpu_verifier_verify_many_device_ex(const qpgpu_verifier *v, struct qpgpu_ctx *ctx, const uint8_t *const *proofs, const size_t *lens,
                                         size_t count, unsigned threads, unsigned flags, int *results, char *reasons, char *err);

/*
 * fri::verifier::verify_fri_proof on its own: the counterpart of qpgpu.h's qpgpu_fri_prove and step entries for a caller who
 * keeps the verifier's head (transcript, constraints at zeta) in its own code and hands over the rest, i.e. all the hashing of a
 * verification. It does not depend on a circuit: an instance is the oracles' shapes, the opening batches and the FRI
 * parameters. A qpgpu_fri_verifier is made once per instance and hasher, shared and thread-safe.
 *
 *   fri::verifier::verify_fri_proof   -> qpgpu_fri_verify, qpgpu_fri_verify_many_device
 *   Challenger::fri_challenges        -> qpgpu_fri_verifier_challenges
 */
typedef struct { uint32_t num_polys; uint32_t blinded; } qpgpu_fri_oracle_shape;   /* blinded: rows end in 4 salt words, hashed, not opened */
typedef struct {
    uint32_t degree_bits;
    uint32_t num_oracles;  const qpgpu_fri_oracle_shape *oracles;
    uint32_t num_batches;  const qpgpu_fri_batch *batches;     /* ranges as in qpgpu_fri_prove; `point` is not read here */
    qpgpu_fri_params params;
} qpgpu_fri_instance;
typedef struct qpgpu_fri_verifier qpgpu_fri_verifier;

/* Validates what qpgpu_fri_prove validates, in its words under the prefix "fri_verifier_create:" (ranges inside their oracle,
 * 1..8 ranges per batch, rounds of 1..8 bits, the schedule against degree and cap height, proof_of_work_bits <= 40, the LDE
 * within 2^23), and takes at most 255 oracles. The verifier keeps a copy of the instance that owns its arrays. hasher_kind / params as qpgpu_verifier_create. */
int    qpgpu_fri_verifier_create(const qpgpu_fri_instance *inst, int hasher_kind, const uint64_t *hasher_params, size_t n_params,
                                 qpgpu_fri_verifier **out, char *err);
void   qpgpu_fri_verifier_free(qpgpu_fri_verifier *v);
size_t qpgpu_fri_verifier_proof_size(const qpgpu_fri_verifier *v);   /* == qpgpu_fri_proof_size for oracles of these shapes */
size_t qpgpu_fri_verifier_num_openings(const qpgpu_fri_verifier *v); /* sum over batches and ranges of count */

/* Challenger::fri_challenges, the order qpgpu_fri_prove uses: alpha = two draws; per round observe(cap), beta = two draws;
 * observe(final polynomial); observe(nonce); one draw = the proof-of-work response; num_query_rounds draws mod the LDE size.
 * Host only; *c (the transcript after the openings were observed) is advanced in place. betas: [rounds][2]; indices:
 * [num_query_rounds]. A caller with other transcript rules computes the four itself. */
int qpgpu_fri_verifier_challenges(const qpgpu_fri_verifier *v, qpgpu_challenger *c, const uint8_t *proof, size_t len,
                                  uint64_t alpha[2], uint64_t *betas, uint64_t *pow_response, uint64_t *indices, char *err);

/* verify_fri_proof for one proof, on the host. caps: [num_oracles] pointers to 4 << cap_height words; points: [num_batches][2];
 * openings: [num_openings][2], batch by batch, range by range. Returns 0, or QPGPU_EVERIFY with the first failing check in err,
 * in this order: length; a non-canonical element anywhere in the proof; the proof-of-work response (leading zero bits); then
 * per query round the checks and texts of qpgpu_verifier_verify's query rounds. What the caller itself supplies is not judged:
 * a non-canonical cap word, point, opening or challenge, or an index >= the LDE size, is QPGPU_EINVAL. Thread-safe. */
int qpgpu_fri_verify(const qpgpu_fri_verifier *v, const uint64_t *const *caps, const uint64_t *points, const uint64_t *openings,
                     const uint64_t alpha[2], const uint64_t *betas, uint64_t pow_response, const uint64_t *indices,
                     const uint8_t *proof, size_t len, char *err);

/* The same for `count` proofs with the query rounds on ctx's GPU. cap_counts[o]: 1 = caps[o] holds one cap shared by all proofs,
 * count = one cap per proof, back to back; anything else is QPGPU_EINVAL naming the oracle. points: [num_batches][count][2];
 * openings [count][num_openings][2]; alphas [count][2]; betas [count][rounds][2]; pow_responses [count]; indices
 * [count][num_query_rounds]. results[i], reasons row i (QPGPU_VERIFY_ERR_CAP bytes, "" when accepted; reasons may be NULL), the
 * return value and err ("proof i: ...") are what `count` calls of qpgpu_fri_verify give. The verifier's hasher must equal the
 * context's, else QPGPU_EINVAL. count == 0 returns 0. A HIP error returns QPGPU_EDEVICE and the proofs not decided by then get
 * QPGPU_EDEVICE (no host fallback). Synchronous on the ctx stream. Instances of more than 16 oracles, 16 rounds or 8 batches
 * are QPGPU_EINVAL here (the host entry takes them). */
int qpgpu_fri_verify_many_device(const qpgpu_fri_verifier *v, struct qpgpu_ctx *ctx, size_t count,
                                 const uint64_t *const *caps, const uint32_t *cap_counts,
                                 const uint64_t *points, const uint64_t *openings,
                                 const uint64_t *alphas, const uint64_t *betas, const uint64_t *pow_responses, const uint64_t *indices,
                                 const uint8_t *const *proofs, const size_t *lens, int *results, char *reasons, char *err);

#ifdef __cplusplus
}
#endif
#endif
