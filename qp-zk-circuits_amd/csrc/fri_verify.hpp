// fri_verify.hpp — fri::verifier::verify_fri_proof over any FRI instance, on the host: the query-round half of verification as one
// function with two callers, the whole-proof verifier (verifier.cpp: four oracles, openings at zeta and g zeta) and the
// stage-level verifier (fri_verify.cpp: qpgpu_fri_verify, any list of oracles and opening batches). query_rounds, query_reason and
// reduced_openings are defined in verifier.cpp, prepare in fri_verify.cpp. No HIP header: both build with a plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "gl64.hpp"
#include "poseidon.hpp"
#include "proof_layout.hpp"

// first failing check of a query round, in the host verifier's order: code = kind << 8 | oracle or round; 0 = accepted
enum : uint32_t { VQ_ORACLE_PLEN = 1, VQ_ORACLE_PATH = 2, VQ_ROUND_PLEN = 3, VQ_ROUND_CONT = 4, VQ_ROUND_PATH = 5, VQ_FINAL = 6 };

namespace friv {

struct Range { uint32_t oracle, first, count; };       // FriPolynomialInfo::from_range

// FriInstanceInfo and FriParams as the query rounds need them
struct Instance {
    unsigned degree_bits = 0, rate_bits = 0, cap_height = 0, pow_bits = 0;
    std::vector<size_t> widths, polys;                 // per initial oracle: leaf words (salt included), opened polynomials
    std::vector<std::vector<Range>> batches;           // FriBatchInfo::polynomials, one list per opening point
    std::vector<uint64_t> arity_bits;
    proof_layout::Fri lay;                             // set by finish()
    void finish(size_t num_query_rounds) { lay = proof_layout::fri_part(degree_bits, rate_bits, cap_height, arity_bits, num_query_rounds, widths); }
    size_t cap_words() const { return (size_t)4 << cap_height; }
    size_t batch_count(size_t b) const { size_t n = 0; for (const Range &r : batches[b]) n += r.count; return n; }
    size_t num_openings() const { size_t n = 0; for (size_t b = 0; b < batches.size(); b++) n += batch_count(b); return n; }
};

// what the query rounds are checked against; every element canonical, every index below the LDE size
struct QueryInput {
    const gl::u64 *const *caps;          // [initial oracles] -> cap_words
    const gl::u64 *round_caps;           // [rounds][cap_words]
    const gl::e2 *points, *reduced;      // per batch: the opening point, the reduced openings sum_j opening_j alpha^j
    gl::e2 alpha;
    const gl::e2 *betas;                 // [rounds]
    const gl::e2 *final_poly;            // [lay.final_len]
    const uint64_t *indices;             // [lay.num_query_rounds]
};

// PrecomputedReducedOpenings: openings batch by batch, range by range; out: one element per batch
void reduced_openings(const Instance &in, const gl::e2 *openings, gl::e2 alpha, gl::e2 *out);

// The query rounds at `queries` (lay.queries_bytes() bytes). 0, or the first failing check as kind << 8 | oracle or round
// (VQ_* above) with its query round in *query.
uint32_t query_rounds(const hasher::Config &h, const Instance &in, const QueryInput &q, const uint8_t *queries, size_t *query);

// the verifier's words for a verdict of query_rounds, into QPGPU_VERIFY_ERR_CAP bytes
void query_reason(char *out, size_t query, uint32_t code);

// Everything qpgpu_fri_verify looks at before the query rounds (fri_verify.cpp), for its two callers: the caller's own values
// (QPGPU_EINVAL: a non-canonical cap word, point, opening or challenge, an index outside the LDE), then the proof's length, its
// elements and the proof-of-work response (QPGPU_EVERIFY). On 0 `p` holds what QueryInput points to.
struct Prepared {
    std::vector<gl::u64> round_caps;
    std::vector<gl::e2> points, reduced, betas, final_poly;
    gl::e2 alpha;
};
}  // namespace friv

struct qpgpu_fri_verifier {
    friv::Instance in;
    hasher::Config hash;
    size_t n_openings = 0;
};

namespace friv {
// caps: [oracles] pointers of this proof; points: batch b's point at points + b * point_stride (words)
int prepare(const qpgpu_fri_verifier *v, const gl::u64 *const *caps, const uint64_t *points, size_t point_stride, const uint64_t *openings,
            const uint64_t *alpha, const uint64_t *betas, uint64_t pow_response, const uint64_t *indices, const uint8_t *proof, size_t len,
            char *err, Prepared &p);
}  // namespace friv
