// fri_api.cpp — stage-level C ABI, the FRI opening proof (include/qpgpu.h): PolynomialBatch::prove_openings as one call
// (qpgpu_fri_prove) and one step at a time (qpgpu_fri_session, qpgpu_fri_grind), for a caller who keeps the transcript and the
// rules around it — the order of observations, the proof-of-work rule, how query indices are drawn — in its own code. Both go
// through the step functions of fri_prover.hpp; the order of a session's calls is FriSteps's (fri_steps.hpp). Every entry exists for
// one proof and for a lockstep batch (the _batch entries; a session remembers its batch): the single-proof ones are the batch of one.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
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
    uint32_t nb = 1;
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
    for (uint32_t i = 0; i < n; i++) widths.push_back(oracles[i]->o.ncols + (oracles[i]->o.salted() ? 4 : 0));
    return QPGPU_OK;
}

// sharded oracles: the call's context is their home context (the FRI arithmetic reads the coefficients there), and the lockstep
// entries do not take them yet. `ctx` is non-NULL; oracles may be anything (fri_setup checks it afterwards).
int fri_sharded_check(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t n, bool lockstep) {
    if (!oracles) return QPGPU_OK;
    for (uint32_t i = 0; i < n; i++) {
        if (!oracles[i] || !oracles[i]->sh) continue;
        if (lockstep) return ctx->fail(QPGPU_EINVAL, "fri_prove_batch: oracle " + std::to_string(i) + " is sharded; sharded oracles are not taken here yet, use qpgpu_fri_prove or qpgpu_fri_begin");
        if (oracles[i]->ctx != ctx) return ctx->fail(QPGPU_EINVAL, "fri_prove: ctx is not the home context (ctxs[0] of qpgpu_oracle_commit_sharded) of sharded oracle " + std::to_string(i));
    }
    return QPGPU_OK;
}

// points: NULL for the single-proof entries (each batch's own `point` field), else [num_batches][nb][2]: proof p's point of batch k
int fri_call(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
             const uint64_t *points, uint32_t nb, const qpgpu_fri_params *params, FriCall &c) {
    if (fri_setup(oracles, num_oracles, params, c.fp, c.widths) != QPGPU_OK || oracles[0]->ctx != ctx)
        return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    c.nb = nb;
    // an oracle holds the batch's proofs, or one proof shared by all of them (constants/sigmas: strides 0)
    for (uint32_t i = 0; i < num_oracles; i++)
        if (oracles[i]->o.nb != nb && oracles[i]->o.nb != 1)
            return ctx->fail(QPGPU_EINVAL, "fri_prove: oracle " + std::to_string(i) + " holds " + std::to_string(oracles[i]->o.nb) + " proofs, the call is for a batch of " + std::to_string(nb) +
                                               (points ? "" : " (use the _batch entries for batched oracles)"));
    c.bs.assign(num_batches, FriBatch());
    for (uint32_t b = 0; b < num_batches; b++) {
        if (batches[b].num_ranges == 0 || batches[b].num_ranges > 8) return ctx->fail(QPGPU_EINVAL, "fri_prove: a batch needs 1..8 polynomial ranges");
        if (!points) c.bs[b].points = {gl::e2_make(gl::canon(batches[b].point[0]), gl::canon(batches[b].point[1]))};
        else for (uint32_t q = 0; q < nb; q++) {
            const uint64_t *pt = points + 2 * ((size_t)b * nb + q);
            c.bs[b].points.push_back(gl::e2_make(gl::canon(pt[0]), gl::canon(pt[1])));
        }
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

// workspace of one call's lockstep batch: one device allocation and one pinned staging block
struct FriSpace {
    void *dv = nullptr, *hv = nullptr;
    size_t work_words = 0;
    Stager stage;
    FriWork work;
    int alloc(qpgpu_ctx *ctx, const FriCall &c) {
        work_words = FriWork::words(c.fp, c.widths, c.max_count, c.nb);
        QP_HIP(ctx, ctx->track_malloc(&dv, work_words * 8, residue::FRI_SESSION));
        stage.words = FriWork::stage_words(c.fp, c.max_count, c.nb);
        hipError_t e = ctx->track_host_malloc(&hv, stage.words * 8, residue::FRI_SESSION);
        if (e != hipSuccess) { ctx->track_free(dv); dv = nullptr; return ctx->hip_fail(e, "hipHostMalloc(fri stage)"); }
        stage.h = (u64 *)hv;
        work.bind((u64 *)dv, c.fp, c.widths, c.max_count, c.nb);
        return QPGPU_OK;
    }
    // the workspace holds alpha-combinations of the committed (possibly secret) polynomials: clear it before release
    void release(qpgpu_ctx *ctx) {
        if (!dv) return;
        (void)hipMemsetAsync(dv, 0, work_words * 8, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (hv) std::memset(hv, 0, stage.words * 8);      // the pinned ring held challenges and query indices
        ctx->track_free(dv); ctx->track_free(hv);
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

// qpgpu_fri_prove / qpgpu_fri_prove_batch: nb transcripts, nb output buffers; points as fri_call's
static int prove_impl(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
                      const uint64_t *points, uint32_t nb, const qpgpu_fri_params *params, qpgpu_challenger *challengers,
                      uint8_t *const *outs, size_t out_cap, size_t *out_lens) {
    FriCall c;
    QP_TRY(fri_sharded_check(ctx, oracles, num_oracles, points != nullptr));
    if (fri_setup(oracles, num_oracles, params, c.fp, c.widths) != QPGPU_OK || oracles[0]->ctx != ctx)
        return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    for (uint32_t b = 0; b < nb; b++)
        if (challengers[b].input_len >= 8 || challengers[b].output_len > 8) return ctx->fail(QPGPU_EINVAL, "fri_prove: invalid challenger state (input_len must be < 8, output_len <= 8)");
    QP_TRY(fri_call(ctx, oracles, num_oracles, batches, num_batches, points, nb, params, c));
    FriSpace sp;
    QP_TRY(sp.alloc(ctx, c));
    std::vector<Challenger> chs(nb, Challenger(ctx->hasher));
    std::vector<ByteWriter> ws;
    for (uint32_t b = 0; b < nb; b++) { (void)challenger_to_host(&challengers[b], chs[b]); ws.push_back(ByteWriter{outs[b], out_cap}); }
    int rc = fri_prove(ctx, c.fp, c.os.data(), c.os.size(), c.bs, nb, chs.data(), sp.work, sp.stage, ws.data());
    sp.release(ctx);
    if (rc != QPGPU_OK) return rc;
    bool overflow = false;
    for (uint32_t b = 0; b < nb; b++) {
        challenger_from_host(chs[b], &challengers[b]);
        if (out_lens) out_lens[b] = ws[b].len;
        overflow = overflow || ws[b].overflow;
    }
    if (overflow) return ctx->fail(QPGPU_EBUFSIZE, "fri_prove: output buffer too small");
    return QPGPU_OK;
}

int qpgpu_fri_prove(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, qpgpu_challenger *challenger,
                    uint8_t *out, size_t out_cap, size_t *out_len) {
    if (!ctx) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (!batches || num_batches == 0 || !challenger || !out) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    return prove_impl(ctx, oracles, num_oracles, batches, num_batches, nullptr, 1, params, challenger, &out, out_cap, out_len);
}

int qpgpu_fri_prove_batch(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
                          const uint64_t *points, uint32_t batch, const qpgpu_fri_params *params, qpgpu_challenger *challengers,
                          uint8_t *const *outs, size_t out_cap, size_t *out_lens) {
    if (!ctx) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (!batches || num_batches == 0 || !points || !challengers || !outs) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    if (batch == 0 || batch > 1024) return ctx->fail(QPGPU_EINVAL, "fri_prove_batch: batch must be 1..1024");
    for (uint32_t b = 0; b < batch; b++) if (!outs[b]) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    return prove_impl(ctx, oracles, num_oracles, batches, num_batches, points, batch, params, challengers, outs, out_cap, out_lens);
}

// ---- the same, one step at a time ----
static int begin_impl(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
                      const uint64_t *points, uint32_t nb, const qpgpu_fri_params *params, const uint64_t *alphas, qpgpu_fri_session **out) {
    if (!params) return ctx->fail(QPGPU_EINVAL, "fri_prove: bad oracles or FRI parameters");
    qpgpu_fri_params prm = *params;
    prm.proof_of_work_bits = 0; prm.num_query_rounds = kOpenChunk;    // not the session's business: neither is read
    FriCall c;
    QP_TRY(fri_sharded_check(ctx, oracles, num_oracles, points != nullptr));
    QP_TRY(fri_call(ctx, oracles, num_oracles, batches, num_batches, points, nb, &prm, c));
    qpgpu_fri_session *s = new qpgpu_fri_session();
    s->ctx = ctx;
    int rc = s->space.alloc(ctx, c);
    if (rc == QPGPU_OK) {
        std::vector<e2> a(nb);
        for (uint32_t b = 0; b < nb; b++) a[b] = gl::e2_make(gl::canon(alphas[2 * b]), gl::canon(alphas[2 * b + 1]));
        rc = fri_begin(ctx, c.fp, c.os.data(), c.os.size(), c.bs, nb, a.data(), s->space.work, s->space.stage, false, s->st);
    }
    if (rc != QPGPU_OK) { s->space.release(ctx); delete s; return rc; }
    *out = s;
    return QPGPU_OK;
}

int qpgpu_fri_begin(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, const uint64_t alpha[2], qpgpu_fri_session **out) {
    if (!ctx || !out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    *out = nullptr;
    if (!batches || num_batches == 0 || !alpha) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    return begin_impl(ctx, oracles, num_oracles, batches, num_batches, nullptr, 1, params, alpha, out);
}

int qpgpu_fri_begin_batch(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches, uint32_t num_batches,
                          const uint64_t *points, uint32_t batch, const qpgpu_fri_params *params, const uint64_t *alphas, qpgpu_fri_session **out) {
    if (!ctx || !out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    *out = nullptr;
    if (!batches || num_batches == 0 || !points || !alphas) return ctx->fail(QPGPU_EINVAL, "fri_prove: null argument");
    if (batch == 0 || batch > 1024) return ctx->fail(QPGPU_EINVAL, "fri_begin_batch: batch must be 1..1024");
    return begin_impl(ctx, oracles, num_oracles, batches, num_batches, points, batch, params, alphas, out);
}

uint32_t qpgpu_fri_session_batch(const qpgpu_fri_session *s) { return s ? s->st.nb : 0; }

void qpgpu_fri_session_free(qpgpu_fri_session *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    s->space.release(s->ctx);
    delete s;
}

// a call out of order is refused before anything else is looked at or done; the session stays where it was
#define QP_FRI_ORDER(s, call) do { const std::string _why = (s)->st.steps.refuse(call); if (!_why.empty()) return (s)->ctx->fail(QPGPU_EINVAL, _why); } while (0)

// The array arguments of the step entries hold the session's nb proofs back to back; at nb = 1 the sizes and messages are the
// single-proof ones.
int qpgpu_fri_round_commit(qpgpu_fri_session *s, uint64_t *cap_out, size_t cap_words) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!cap_out) return ctx->fail(QPGPU_EINVAL, "fri_round_commit: cap_out is NULL");
    const size_t want = s->st.nb * s->st.cap_words();
    if (cap_words != want)
        return ctx->fail(QPGPU_EINVAL, "fri_round_commit: cap_words is " + std::to_string(cap_words) + ", the cap has " + std::to_string(want) + " words" +
                                           (s->st.nb > 1 ? " for the session's " + std::to_string(s->st.nb) + " proofs" : ""));
    QP_FRI_ORDER(s, FriSteps::COMMIT);
    QP_TRY(fri_round_commit(s->st));
    std::memcpy(cap_out, s->st.caps.back().data(), cap_words * 8);
    return QPGPU_OK;
}

int qpgpu_fri_round_fold(qpgpu_fri_session *s, const uint64_t *beta) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!beta) return ctx->fail(QPGPU_EINVAL, "fri_round_fold: beta is NULL");
    QP_FRI_ORDER(s, FriSteps::FOLD);
    std::vector<e2> b(s->st.nb);
    for (uint32_t i = 0; i < s->st.nb; i++) b[i] = gl::e2_make(gl::canon(beta[2 * i]), gl::canon(beta[2 * i + 1]));
    return fri_round_fold(s->st, b.data());
}

int qpgpu_fri_final_poly(qpgpu_fri_session *s, uint64_t *out, size_t out_words, size_t *num_coeffs) {
    if (!s) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = s->ctx;
    QP_DEV(ctx);
    if (!out) return ctx->fail(QPGPU_EINVAL, "fri_final_poly: out is NULL");
    const size_t len = s->st.w->proof.final_len, nb = s->st.nb;
    if (out_words != nb * 2 * len)
        return ctx->fail(QPGPU_EINVAL, "fri_final_poly: out_words is " + std::to_string(out_words) + ", the final polynomial has " + std::to_string(nb * 2 * len) + " words" +
                                           (nb > 1 ? " for the session's " + std::to_string(nb) + " proofs" : ""));
    QP_FRI_ORDER(s, FriSteps::FINAL_POLY);
    std::vector<u64> fc;
    QP_TRY(fri_final_poly(s->st, fc));
    for (size_t b = 0; b < nb; b++)
        for (size_t i = 0; i < len; i++) { out[2 * (b * len + i)] = fc[2 * b * len + i]; out[2 * (b * len + i) + 1] = fc[2 * b * len + len + i]; }
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
    const size_t qs = qpgpu_fri_query_size(s), nb = s->st.nb;
    if (out_cap / qs / nb < n)
        return ctx->fail(QPGPU_EINVAL, "fri_open: out_cap is " + std::to_string(out_cap) + ", " + std::to_string(n) + " query rounds take " +
                                           (nb > 1 ? std::to_string(nb) + " x " : "") + std::to_string(n) + " x " + std::to_string(qs) + " bytes");
    const unsigned L = s->st.p.degree_bits + s->st.p.rate_bits;
    for (size_t b = 0; b < nb; b++)
        for (size_t i = 0; i < n; i++)
            if (indices[b * n + i] >> L)
                return ctx->fail(QPGPU_EINVAL, "fri_open: indices[" + (nb > 1 ? std::to_string(b) + "][" : "") + std::to_string(i) + "] = " + std::to_string(indices[b * n + i]) +
                                                   " is not below 2^" + std::to_string(L));
    Stager &stage = s->space.stage;
    if (!s->opened) { s->opened = true; s->open_pos = stage.pos; }
    std::vector<ByteWriter> ws;
    for (size_t b = 0; b < nb; b++) ws.push_back(ByteWriter{out + b * n * qs, n * qs});
    std::vector<u64> idx;
    for (size_t at = 0; at < n; at += kOpenChunk) {
        stage.pos = s->open_pos;      // the previous gather has been read back: its indices' slot is free again
        const uint32_t m = (uint32_t)std::min<size_t>(kOpenChunk, n - at);
        idx.resize(nb * m);
        for (size_t b = 0; b < nb; b++) std::memcpy(idx.data() + b * m, indices + b * n + at, (size_t)m * 8);
        QP_TRY(fri_gather(s->st, idx.data(), m, ws.data()));
    }
    if (out_len) *out_len = nb * n * qs;
    return QPGPU_OK;
}

// qpgpu_fri_grind / qpgpu_fri_grind_batch: nb transcripts in lockstep, one search
static int grind_impl(qpgpu_ctx *ctx, const qpgpu_challenger *cs, uint32_t nb, unsigned proof_of_work_bits, uint64_t *nonces_out) {
    if (proof_of_work_bits > 40) return ctx->fail(QPGPU_EINVAL, "fri_grind: proof_of_work_bits above 40");
    std::vector<Challenger> chs(nb, Challenger(ctx->hasher));
    for (uint32_t b = 0; b < nb; b++) {
        if (!challenger_to_host(&cs[b], chs[b])) return ctx->fail(QPGPU_EINVAL, "fri_grind: invalid challenger state (input_len must be < 8, output_len <= 8)");
        if (chs[b].n_in != chs[0].n_in) return ctx->fail(QPGPU_EINVAL, "fri_grind: challengers[" + std::to_string(b) + "] holds another number of pending inputs than challengers[0]: the transcripts of a batch advance together");
    }
    if (proof_of_work_bits == 0) { for (uint32_t b = 0; b < nb; b++) nonces_out[b] = 0; return QPGPU_OK; }
    ctx->hasher_in_use = true;
    QP_TRY(merkle_ensure_constants(ctx));
    QP_TRY(ctx->ensure_scratch((size_t)nb * 16 * 8));   // the search's three small tables; nothing else runs on the context meanwhile
    Stager bounce;                                // no ring: the two uploads go through the context's pinned buffer
    std::vector<u64> nonces(nb, 0);
    u64 *t = ctx->scratch;
    QP_TRY(fri_grind(ctx, chs.data(), nb, proof_of_work_bits, PowTables{t, t + 12 * (size_t)nb, t + 13 * (size_t)nb}, bounce, nonces.data()));
    for (uint32_t b = 0; b < nb; b++) nonces_out[b] = nonces[b];
    return QPGPU_OK;
}

int qpgpu_fri_grind(qpgpu_ctx *ctx, const qpgpu_challenger *c, unsigned proof_of_work_bits, uint64_t *nonce_out) {
    if (!ctx || !c || !nonce_out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    return grind_impl(ctx, c, 1, proof_of_work_bits, nonce_out);
}

int qpgpu_fri_grind_batch(qpgpu_ctx *ctx, const qpgpu_challenger *cs, uint32_t batch, unsigned proof_of_work_bits, uint64_t *nonces_out) {
    if (!ctx || !cs || !nonces_out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (batch == 0 || batch > 1024) return ctx->fail(QPGPU_EINVAL, "fri_grind_batch: batch must be 1..1024");
    return grind_impl(ctx, cs, batch, proof_of_work_bits, nonces_out);
}

}  // extern "C"
