// fri_api.cpp — stage-level C ABI, the FRI opening proof (include/qpgpu.h): PolynomialBatch::prove_openings as one call
// (qpgpu_fri_prove) and one step at a time (qpgpu_fri_session, qpgpu_fri_grind), for a caller who keeps the transcript and the
// rules around it — the order of observations, the proof-of-work rule, how query indices are drawn — in its own code. Both go
// through the step functions of fri_prover.hpp; the order of a session's calls is FriSteps's (fri_steps.hpp).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include "fri_prover.hpp"
#include "oracle_handle.hpp"

using gl::e2;
using gl::u64;

namespace {
// what the two entries that start a proof share: parameters, oracles and batches checked and converted
struct FriCall {
    FriParams fp;
    std::vector<size_t> widths;
    std::vector<FriBatch> bs;
    std::vector<const PolyOracle *> os;
    size_t max_count = 0;
};

int fri_setup(qpgpu_oracle *const *oracles, uint32_t n, const qpgpu_fri_params *params, FriParams &fp, std::vector<size_t> &widths) {
    if (!oracles || n == 0 || !params || params->num_reduction_rounds > 16) return QPGPU_EINVAL;
    for (uint32_t i = 0; i < n; i++) if (!oracles[i] || oracles[i]->ctx != oracles[0]->ctx) return QPGPU_EINVAL;
    fp.degree_bits = oracles[0]->o.log_n; fp.rate_bits = params->rate_bits; fp.cap_h = params->cap_height;
    fp.pow_bits = params->proof_of_work_bits; fp.num_queries = params->num_query_rounds;
    fp.arity_bits.assign(params->reduction_arity_bits, params->reduction_arity_bits + params->num_reduction_rounds);
    unsigned tot = 0;
    for (unsigned a : fp.arity_bits) { if (a == 0 || a > 8) return QPGPU_EINVAL; tot += a; }
    if (tot > fp.degree_bits || fp.degree_bits + fp.rate_bits < tot + fp.cap_h || fp.pow_bits > 40 || fp.num_queries == 0 || fp.num_queries > 4096) return QPGPU_EINVAL;
    widths.clear();
    for (uint32_t i = 0; i < n; i++) widths.push_back(oracles[i]->o.ncols + (oracles[i]->o.salt ? 4 : 0));
    return QPGPU_OK;
}

int fri_call(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
             const qpgpu_fri_params *params, FriCall &c) {
    if (fri_setup(oracles, num_oracles, params, c.fp, c.widths) != QPGPU_OK || oracles[0]->ctx != ctx)
        return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    c.bs.assign(num_batches, FriBatch());
    for (uint32_t b = 0; b < num_batches; b++) {
        if (batches[b].num_ranges == 0 || batches[b].num_ranges > 8) return ctx->fail(QPGPU_EINVAL, "fri_prove: a batch needs 1..8 polynomial ranges");
        c.bs[b].points = {gl::e2_make(gl::canon(batches[b].point[0]), gl::canon(batches[b].point[1]))};
        size_t cnt = 0;
        for (uint32_t r = 0; r < batches[b].num_ranges; r++) {
            const qpgpu_fri_range &rg = batches[b].ranges[r];
            c.bs[b].ranges.push_back({rg.oracle, rg.first, rg.count});
            cnt += rg.count;
        }
        c.max_count = std::max(c.max_count, cnt);
    }
    for (uint32_t i = 0; i < num_oracles; i++) c.os.push_back(&oracles[i]->o);
    return QPGPU_OK;
}

// workspace of one proof: one device allocation and one pinned staging block
struct FriSpace {
    void *dv = nullptr, *hv = nullptr;
    size_t work_words = 0;
    Stager stage;
    FriWork work;
    int alloc(qpgpu_ctx *ctx, const FriCall &c) {
        work_words = FriWork::words(c.fp, c.widths, c.max_count, 1);
        QP_HIP(ctx, hipMalloc(&dv, work_words * 8));
        stage.words = FriWork::stage_words(c.fp, c.max_count, 1);
        hipError_t e = hipHostMalloc(&hv, stage.words * 8, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipFree(dv); dv = nullptr; return ctx->hip_fail(e, "hipHostMalloc(fri stage)"); }
        stage.h = (u64 *)hv;
        work.bind((u64 *)dv, c.fp, c.widths, c.max_count, 1);
        return QPGPU_OK;
    }
    // the workspace holds alpha-combinations of the committed (possibly secret) polynomials: clear it before release
    void release(qpgpu_ctx *ctx) {
        if (!dv) return;
        (void)hipMemsetAsync(dv, 0, work_words * 8, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(dv); (void)hipHostFree(hv);
        dv = hv = nullptr;
    }
};

const uint32_t kOpenChunk = 32;   // indices one gather of a session takes (FriParams::num_queries of its workspace)
}  // namespace

struct qpgpu_fri_session {
    qpgpu_ctx *ctx = nullptr;
    FriSpace space;
    FriState st;                  // points into space: a session is never copied
    bool opened = false;
    size_t open_pos = 0;          // staging position the query indices of every qpgpu_fri_open start from
};

extern "C" {

size_t qpgpu_fri_proof_size(qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_params *params) {
    FriParams fp; std::vector<size_t> widths;
    if (fri_setup(oracles, num_oracles, params, fp, widths) != QPGPU_OK) return 0;
    return fri_proof_bytes(fp, widths);
}

int qpgpu_fri_prove(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, qpgpu_challenger *challenger,
                    uint8_t *out, size_t out_cap, size_t *out_len) {
    if (!ctx) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (!batches || num_batches == 0 || !challenger || !out) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    FriCall c;
    if (fri_setup(oracles, num_oracles, params, c.fp, c.widths) != QPGPU_OK || oracles[0]->ctx != ctx)
        return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    if (challenger->input_len >= 8 || challenger->output_len > 8) return ctx->fail(QPGPU_EINVAL, "fri_prove: invalid challenger state (input_len must be < 8, output_len <= 8)");
    QP_TRY(fri_call(ctx, oracles, num_oracles, batches, num_batches, params, c));
    FriSpace sp;
    QP_TRY(sp.alloc(ctx, c));
    Challenger ch(ctx->hasher); (void)challenger_to_host(challenger, ch);
    ByteWriter w{out, out_cap};
    int rc = fri_prove(ctx, c.fp, c.os.data(), c.os.size(), c.bs, 1, &ch, sp.work, sp.stage, &w);
    sp.release(ctx);
    if (rc != QPGPU_OK) return rc;
    challenger_from_host(ch, challenger);
    if (out_len) *out_len = w.len;
    if (w.overflow) return ctx->fail(QPGPU_EBUFSIZE, "fri_prove: output buffer too small");
    return QPGPU_OK;
}

// ---- the same, one step at a time ----
int qpgpu_fri_begin(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, const uint64_t alpha[2], qpgpu_fri_session **out) {
    if (!ctx || !out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    *out = nullptr;
    if (!batches || num_batches == 0 || !alpha) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    if (!params) return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    qpgpu_fri_params prm = *params;
    prm.proof_of_work_bits = 0; prm.num_query_rounds = kOpenChunk;    // not the session's business: neither is read
    FriCall c;
    QP_TRY(fri_call(ctx, oracles, num_oracles, batches, num_batches, &prm, c));
    qpgpu_fri_session *s = new qpgpu_fri_session();
    s->ctx = ctx;
    int rc = s->space.alloc(ctx, c);
    if (rc == QPGPU_OK) {
        const e2 a = gl::e2_make(gl::canon(alpha[0]), gl::canon(alpha[1]));
        rc = fri_begin(ctx, c.fp, c.os.data(), c.os.size(), c.bs, 1, &a, s->space.work, s->space.stage, false, s->st);
    }
    if (rc != QPGPU_OK) { s->space.release(ctx); delete s; return rc; }
    *out = s;
    return QPGPU_OK;
}

void qpgpu_fri_session_free(qpgpu_fri_session *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    s->space.release(s->ctx);
    delete s;
}

// a call out of order is refused before anything else is looked at or done; the session stays where it was
#define QP_FRI_ORDER(s, call) do { const std::string _why = (s)->st.steps.refuse(call); if (!_why.empty()) return (s)->ctx->fail(QPGPU_EINVAL, _why); } while (0)

int qpgpu_fri_round_commit(qpgpu_fri_session *s, uint64_t *cap_out, size_t cap_words) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!cap_out) return ctx->fail(QPGPU_EINVAL, "fri_round_commit: cap_out is NULL");
    if (cap_words != s->st.cap_words())
        return ctx->fail(QPGPU_EINVAL, "fri_round_commit: cap_words is " + std::to_string(cap_words) + ", the cap has " + std::to_string(s->st.cap_words()) + " words");
    QP_FRI_ORDER(s, FriSteps::COMMIT);
    QP_TRY(fri_round_commit(s->st));
    std::memcpy(cap_out, s->st.caps.back().data(), cap_words * 8);
    return QPGPU_OK;
}

int qpgpu_fri_round_fold(qpgpu_fri_session *s, const uint64_t beta[2]) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!beta) return ctx->fail(QPGPU_EINVAL, "fri_round_fold: beta is NULL");
    QP_FRI_ORDER(s, FriSteps::FOLD);
    const e2 b = gl::e2_make(gl::canon(beta[0]), gl::canon(beta[1]));
    return fri_round_fold(s->st, &b);
}

int qpgpu_fri_final_poly(qpgpu_fri_session *s, uint64_t *out, size_t out_words, size_t *num_coeffs) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!out) return ctx->fail(QPGPU_EINVAL, "fri_final_poly: out is NULL");
    const size_t len = s->st.w->proof.final_len;
    if (out_words != 2 * len)
        return ctx->fail(QPGPU_EINVAL, "fri_final_poly: out_words is " + std::to_string(out_words) + ", the final polynomial has " + std::to_string(2 * len) + " words");
    QP_FRI_ORDER(s, FriSteps::FINAL_POLY);
    std::vector<u64> fc;
    QP_TRY(fri_final_poly(s->st, fc));
    for (size_t i = 0; i < len; i++) { out[2 * i] = fc[i]; out[2 * i + 1] = fc[len + i]; }
    if (num_coeffs) *num_coeffs = len;
    return QPGPU_OK;
}

size_t qpgpu_fri_query_size(const qpgpu_fri_session *s) { return s ? s->st.w->proof.round_bytes : 0; }

int qpgpu_fri_open(qpgpu_fri_session *s, const uint64_t *indices, size_t n, uint8_t *out, size_t out_cap, size_t *out_len) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    QP_FRI_ORDER(s, FriSteps::OPEN);
    if (n == 0) { if (out_len) *out_len = 0; return QPGPU_OK; }
    if (!indices) return ctx->fail(QPGPU_EINVAL, "fri_open: indices is NULL");
    if (!out) return ctx->fail(QPGPU_EINVAL, "fri_open: out is NULL");
    const size_t qs = qpgpu_fri_query_size(s);
    if (out_cap / qs < n)
        return ctx->fail(QPGPU_EINVAL, "fri_open: out_cap is " + std::to_string(out_cap) + ", " + std::to_string(n) + " query rounds take " + std::to_string(n) + " x " + std::to_string(qs) + " bytes");
    const unsigned L = s->st.p.degree_bits + s->st.p.rate_bits;
    for (size_t i = 0; i < n; i++)
        if (indices[i] >> L)
            return ctx->fail(QPGPU_EINVAL, "fri_open: indices[" + std::to_string(i) + "] = " + std::to_string(indices[i]) + " is not below 2^" + std::to_string(L));
    Stager &stage = s->space.stage;
    if (!s->opened) { s->opened = true; s->open_pos = stage.pos; }
    ByteWriter w{out, out_cap};
    for (size_t at = 0; at < n; at += kOpenChunk) {
        stage.pos = s->open_pos;      // the previous gather has been read back: its indices' slot is free again
        QP_TRY(fri_gather(s->st, indices + at, (uint32_t)std::min<size_t>(kOpenChunk, n - at), &w));
    }
    if (out_len) *out_len = w.len;
    return QPGPU_OK;
}

int qpgpu_fri_grind(qpgpu_ctx *ctx, const qpgpu_challenger *c, unsigned proof_of_work_bits, uint64_t *nonce_out) {
    if (!ctx || !c || !nonce_out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (proof_of_work_bits > 40) return ctx->fail(QPGPU_EINVAL, "fri_grind: proof_of_work_bits above 40");
    Challenger ch(ctx->hasher);
    if (!challenger_to_host(c, ch)) return ctx->fail(QPGPU_EINVAL, "fri_grind: invalid challenger state (input_len must be < 8, output_len <= 8)");
    if (proof_of_work_bits == 0) { *nonce_out = 0; return QPGPU_OK; }
    ctx->hasher_in_use = true;
    QP_TRY(merkle_ensure_constants(ctx));
    QP_TRY(ctx->ensure_scratch(16 * 8));          // the search's three small tables; nothing else runs on the context meanwhile
    Stager bounce;                                // no ring: the two uploads go through the context's pinned buffer
    u64 nonce = 0;
    QP_TRY(fri_grind(ctx, &ch, 1, proof_of_work_bits, PowTables{ctx->scratch, ctx->scratch + 12, ctx->scratch + 13}, bounce, &nonce));
    *nonce_out = nonce;
    return QPGPU_OK;
}

}  // extern "C"
