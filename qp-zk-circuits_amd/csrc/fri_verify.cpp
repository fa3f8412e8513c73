// fri_verify.cpp — verification of FRI opening proofs on the host (include/qpgpu_verify.h: qpgpu_fri_verifier_*,
// qpgpu_fri_verify): plonky2's fri::verifier::verify_fri_proof and Challenger::fri_challenges over any instance, the counterpart
// of the stage-level prover (fri_api.cpp). The query loop itself, friv::query_rounds, is the one every host verification in the
// library runs and lives with the whole-proof verifier (verifier.cpp). Pure host code: no HIP header is needed to build it.
#include "../../include/qpgpu.h"
#include "../../include/qpgpu_verify.h"
#include <algorithm>
#include <cstring>
#include <new>
#include "challenger.hpp"
#include "fri_verify.hpp"
#include "verifier.hpp"

using gl::e2;
using gl::u64;
using verify::fail;

namespace {

inline u64 word_at(const uint8_t *p) { u64 v; std::memcpy(&v, p, 8); return v; }

}  // namespace

namespace friv {

int prepare(const qpgpu_fri_verifier *v, const u64 *const *caps, const uint64_t *points, size_t point_stride, const uint64_t *openings,
            const uint64_t *alpha, const uint64_t *betas, uint64_t pow_response, const uint64_t *indices, const uint8_t *proof, size_t len,
            char *err, Prepared &p) {
    const Instance &in = v->in;
    const proof_layout::Fri &lay = in.lay;
    const size_t n_oracles = in.widths.size(), n_rounds = in.arity_bits.size(), n_batches = in.batches.size(), cap_words = in.cap_words();
    // ---- the caller's own values: not judged, refused ----
    for (size_t o = 0; o < n_oracles; o++) {
        if (!caps[o]) return fail(err, QPGPU_EINVAL, "fri_verify: null argument");
        for (size_t i = 0; i < cap_words; i++)
            if (caps[o][i] >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: word %zu of the cap of oracle %zu is not canonical", i, o);
    }
    p.points.resize(n_batches);
    for (size_t b = 0; b < n_batches; b++) {
        const uint64_t *pt = points + b * point_stride;
        if (pt[0] >= gl::P || pt[1] >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: the point of batch %zu is not canonical", b);
        p.points[b] = gl::e2_make(pt[0], pt[1]);
    }
    for (size_t i = 0; i < 2 * v->n_openings; i++)
        if (openings[i] >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: opening %zu is not canonical", i / 2);
    if (alpha[0] >= gl::P || alpha[1] >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: alpha is not canonical");
    p.alpha = gl::e2_make(alpha[0], alpha[1]);
    p.betas.resize(n_rounds);
    for (size_t r = 0; r < n_rounds; r++) {
        if (betas[2 * r] >= gl::P || betas[2 * r + 1] >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: beta %zu is not canonical", r);
        p.betas[r] = gl::e2_make(betas[2 * r], betas[2 * r + 1]);
    }
    if (pow_response >= gl::P) return fail(err, QPGPU_EINVAL, "fri_verify: the proof-of-work response is not canonical");
    for (size_t q = 0; q < lay.num_query_rounds; q++)
        if (indices[q] >> (in.degree_bits + in.rate_bits))
            return fail(err, QPGPU_EINVAL, "fri_verify: indices[%zu] = %llu is not below 2^%u", q, (unsigned long long)indices[q], in.degree_bits + in.rate_bits);
    // ---- the proof ----
    if (len != lay.total) return fail(err, QPGPU_EVERIFY, "FRI proof has %zu bytes, this instance's proofs have %zu", len, lay.total);
    bool noncanonical = false;
    auto scan = [&](const uint8_t *at, size_t n) { for (size_t i = 0; i < n; i++) noncanonical |= word_at(at + 8 * i) >= gl::P; };
    const size_t queries_pos = n_rounds * lay.cap_bytes, final_pos = queries_pos + lay.queries_bytes();
    scan(proof, n_rounds * cap_words);
    for (size_t q = 0; q < lay.num_query_rounds; q++)
        for (const proof_layout::Opening &o : lay.op) {
            const uint8_t *at = proof + queries_pos + q * lay.round_bytes + o.off;
            scan(at, o.row_words);
            scan(at + 8 * o.row_words + 1, 4 * o.path_len);
        }
    scan(proof + final_pos, 2 * lay.final_len + 1);
    if (noncanonical) return fail(err, QPGPU_EVERIFY, "proof holds a non-canonical field element");
    if (in.pow_bits && (pow_response >> (64 - in.pow_bits)) != 0)
        return fail(err, QPGPU_EVERIFY, "proof-of-work response has fewer than %llu leading zero bits", (unsigned long long)in.pow_bits);
    p.round_caps.assign(n_rounds * cap_words, 0);
    if (n_rounds) std::memcpy(p.round_caps.data(), proof, n_rounds * cap_words * 8);
    p.final_poly.resize(lay.final_len);
    std::memcpy((void *)p.final_poly.data(), proof + final_pos, lay.final_len * 16);
    p.reduced.resize(n_batches);
    reduced_openings(in, (const e2 *)openings, p.alpha, p.reduced.data());
    return QPGPU_OK;
}

}  // namespace friv

extern "C" {

int qpgpu_fri_verifier_create(const qpgpu_fri_instance *inst, int hasher_kind, const uint64_t *hasher_params, size_t n_params,
                              qpgpu_fri_verifier **out, char *err) {
    if (!inst || !out) return fail(err, QPGPU_EINVAL, "fri_verifier_create: null argument");
    *out = nullptr;
    if (!inst->batches || inst->num_batches == 0) return fail(err, QPGPU_EINVAL, "fri_verifier_create: null argument");
    const qpgpu_fri_params &prm = inst->params;
    // qpgpu_fri_prove's checks of oracles and parameters, in its order and words (fri_api.cpp: fri_setup, fri_call; oracle_api.cpp)
    const char *bad = "fri_verifier_create: bad oracles or FRI parameters";
    if (!inst->oracles || inst->num_oracles == 0 || prm.num_reduction_rounds > 16) return fail(err, QPGPU_EINVAL, "%s", bad);
    // a verdict names its oracle or round in eight bits (fri_verify.hpp: kind << 8 | oracle or round)
    if (inst->num_oracles > 255) return fail(err, QPGPU_EINVAL, "fri_verifier_create: more than 255 oracles");
    unsigned tot = 0;
    for (uint32_t r = 0; r < prm.num_reduction_rounds; r++) {
        const unsigned a = prm.reduction_arity_bits[r];
        if (a == 0 || a > 8) return fail(err, QPGPU_EINVAL, "%s", bad);
        tot += a;
    }
    if (tot > inst->degree_bits || (uint64_t)inst->degree_bits + prm.rate_bits < (uint64_t)tot + prm.cap_height || prm.proof_of_work_bits > 40 ||
        prm.num_query_rounds == 0 || prm.num_query_rounds > 4096)
        return fail(err, QPGPU_EINVAL, "%s", bad);
    if ((uint64_t)inst->degree_bits + prm.rate_bits > 23 || inst->degree_bits < 1)
        return fail(err, QPGPU_EINVAL, "fri_verifier_create: LDE sizes up to 2^23 supported");
    qpgpu_fri_verifier *v = new (std::nothrow) qpgpu_fri_verifier();
    if (!v) return fail(err, QPGPU_ENOMEM, "out of memory");
    friv::Instance &in = v->in;
    in.degree_bits = inst->degree_bits; in.rate_bits = prm.rate_bits; in.cap_height = prm.cap_height; in.pow_bits = prm.proof_of_work_bits;
    in.arity_bits.assign(prm.reduction_arity_bits, prm.reduction_arity_bits + prm.num_reduction_rounds);
    for (uint32_t o = 0; o < inst->num_oracles; o++) {
        const qpgpu_fri_oracle_shape &s = inst->oracles[o];
        if (s.num_polys == 0 || s.num_polys > (1u << 20)) { delete v; return fail(err, QPGPU_EINVAL, "%s", bad); }
        in.polys.push_back(s.num_polys);
        in.widths.push_back((size_t)s.num_polys + (s.blinded ? 4 : 0));
    }
    for (uint32_t b = 0; b < inst->num_batches; b++) {
        const qpgpu_fri_batch &fb = inst->batches[b];
        if (fb.num_ranges == 0 || fb.num_ranges > 8) { delete v; return fail(err, QPGPU_EINVAL, "fri_verifier_create: a batch needs 1..8 polynomial ranges"); }
        in.batches.emplace_back();
        for (uint32_t r = 0; r < fb.num_ranges; r++) {
            const qpgpu_fri_range &rg = fb.ranges[r];
            if (rg.oracle >= inst->num_oracles || (size_t)rg.first + rg.count > in.polys[rg.oracle] || rg.count == 0) {
                delete v;
                return fail(err, QPGPU_EINVAL, "fri_verifier_create: polynomial range outside its oracle");
            }
            in.batches.back().push_back({rg.oracle, rg.first, rg.count});
        }
    }
    if (int rc = verify::parse_hasher(hasher_kind, hasher_params, n_params, v->hash, err)) { delete v; return rc; }
    in.finish(prm.num_query_rounds);
    v->n_openings = in.num_openings();
    *out = v;
    return QPGPU_OK;
}

void qpgpu_fri_verifier_free(qpgpu_fri_verifier *v) { delete v; }
size_t qpgpu_fri_verifier_proof_size(const qpgpu_fri_verifier *v) { return v ? v->in.lay.total : 0; }
size_t qpgpu_fri_verifier_num_openings(const qpgpu_fri_verifier *v) { return v ? v->n_openings : 0; }

int qpgpu_fri_verifier_challenges(const qpgpu_fri_verifier *v, qpgpu_challenger *c, const uint8_t *proof, size_t len,
                                  uint64_t alpha[2], uint64_t *betas, uint64_t *pow_response, uint64_t *indices, char *err) {
    if (!v || !c || !proof || !alpha || !pow_response || !indices) return fail(err, QPGPU_EINVAL, "fri_verifier_challenges: null argument");
    const friv::Instance &in = v->in;
    const proof_layout::Fri &lay = in.lay;
    const size_t n_rounds = in.arity_bits.size(), cap_words = in.cap_words();
    if (n_rounds && !betas) return fail(err, QPGPU_EINVAL, "fri_verifier_challenges: null argument");
    if (len != lay.total) return fail(err, QPGPU_EINVAL, "fri_verifier_challenges: FRI proof has %zu bytes, this instance's proofs have %zu", len, lay.total);
    Challenger ch(v->hash);
    if (!challenger_to_host(c, ch)) return fail(err, QPGPU_EINVAL, "fri_verifier_challenges: invalid challenger state (input_len must be < 8, output_len <= 8)");
    std::vector<u64> buf(std::max(cap_words, 2 * lay.final_len + 1));
    alpha[0] = ch.get(); alpha[1] = ch.get();
    for (size_t r = 0; r < n_rounds; r++) {
        std::memcpy(buf.data(), proof + r * lay.cap_bytes, cap_words * 8);
        ch.observe(buf.data(), cap_words);
        betas[2 * r] = ch.get(); betas[2 * r + 1] = ch.get();
    }
    std::memcpy(buf.data(), proof + n_rounds * lay.cap_bytes + lay.queries_bytes(), (2 * lay.final_len + 1) * 8);
    ch.observe(buf.data(), 2 * lay.final_len);
    ch.observe(buf.data() + 2 * lay.final_len, 1);          // the proof-of-work witness
    *pow_response = ch.get();
    const u64 lde_n = 1ull << (in.degree_bits + in.rate_bits);
    for (size_t q = 0; q < lay.num_query_rounds; q++) indices[q] = ch.get() % lde_n;
    challenger_from_host(ch, c);
    return QPGPU_OK;
}

int qpgpu_fri_verify(const qpgpu_fri_verifier *v, const uint64_t *const *caps, const uint64_t *points, const uint64_t *openings,
                     const uint64_t alpha[2], const uint64_t *betas, uint64_t pow_response, const uint64_t *indices,
                     const uint8_t *proof, size_t len, char *err) {
    if (!v || !caps || !points || !openings || !alpha || !indices || !proof || (!betas && !v->in.arity_bits.empty()))
        return fail(err, QPGPU_EINVAL, "fri_verify: null argument");
    friv::Prepared p;
    if (int rc = friv::prepare(v, caps, points, 2, openings, alpha, betas, pow_response, indices, proof, len, err, p)) return rc;
    const friv::QueryInput q{caps, p.round_caps.data(), p.points.data(), p.reduced.data(), p.alpha, p.betas.data(), p.final_poly.data(), indices};
    size_t qi = 0;
    const uint32_t code = friv::query_rounds(v->hash, v->in, q, proof + v->in.arity_bits.size() * v->in.lay.cap_bytes, &qi);
    if (!code) return QPGPU_OK;
    friv::query_reason(err, qi, code);
    return QPGPU_EVERIFY;
}

}  // extern "C"
