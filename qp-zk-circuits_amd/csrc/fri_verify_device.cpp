// fri_verify_device.cpp — qpgpu_fri_verify_many_device (include/qpgpu_verify.h): qpgpu_fri_verify for many proofs of one
// instance with the query rounds on the context's GPU. Per chunk of proofs, as verify_device.cpp does for whole proofs:
//   1. on host threads, everything qpgpu_fri_verify looks at before the query rounds (fri_verify.cpp: friv::prepare — the
//      caller's values, length, canonical elements, proof of work); a proof that passes is copied into the pinned staging buffer
//      with its record and its caps
//   2. one host-to-device copy of the chunk, the query-round kernels (fri_verify_kernels.hip), the per-query verdicts read back
//   3. per proof, the first failing query's verdict in the host verifier's words
// The proof length is fixed by the instance before upload, the indices are range-checked in step 1: the kernels take no length
// and no offset from proof bytes. The workspace is the context's verification workspace (ctx.hpp: vd_pin, vd_dev).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>
#include "../../include/qpgpu.h"
#include "../../include/qpgpu_verify.h"
#include "ctx.hpp"
#include "fri_verify.hpp"
#include "fri_verify_kernels.hpp"
#include "verifier.hpp"

using gl::u64;

namespace {

// the instance as the kernels read it; cap offsets are filled per call (they depend on which caps are shared)
bool make_layout(const friv::Instance &in, FvLayout &lay) {
    const proof_layout::Fri &p = in.lay;
    const size_t n_oracles = in.widths.size(), n_rounds = in.arity_bits.size();
    if (n_oracles > (size_t)FV_MAX_ORACLES || n_rounds > (size_t)FV_MAX_ROUNDS || in.batches.size() > (size_t)FV_MAX_BATCHES || p.total >= ((size_t)1 << 31))
        return false;
    memset(&lay, 0, sizeof lay);
    lay.nq = (uint32_t)p.num_query_rounds;
    lay.n_oracles = (uint32_t)n_oracles; lay.n_rounds = (uint32_t)n_rounds; lay.n_batches = (uint32_t)in.batches.size();
    lay.queries_pos = (uint32_t)(n_rounds * p.cap_bytes);
    lay.q_bytes = (uint32_t)p.round_bytes;
    lay.final_off = (uint32_t)(lay.queries_pos + p.queries_bytes());
    lay.final_n = (uint32_t)p.final_len;
    lay.stride_words = (uint32_t)((p.total + 7) / 8 + 1);
    lay.rec_words = frec_words(lay.n_batches, lay.n_rounds, lay.nq);
    lay.log_lde = in.degree_bits + in.rate_bits;
    for (size_t r = 0; r < n_rounds; r++) lay.arity_bits[r] = (uint32_t)in.arity_bits[r];
    for (size_t i = 0; i < n_oracles + n_rounds; i++) {
        const proof_layout::Opening &o = p.op[i];
        lay.op[i] = {(uint32_t)o.off, (uint32_t)o.row_words, (uint32_t)o.path_len, (uint32_t)o.shift, 0, 0};
        if (i >= n_oracles) { lay.op[i].cap_off = (uint32_t)((i - n_oracles) * in.cap_words()); lay.op[i].cap_stride = FV_CAP_IN_PROOF; }
    }
    for (size_t b = 0; b < in.batches.size(); b++) {
        if (in.batches[b].size() > (size_t)FV_MAX_RANGES) return false;
        lay.batch[b].num_ranges = (uint32_t)in.batches[b].size();
        for (size_t k = 0; k < in.batches[b].size(); k++) {
            const friv::Range &rg = in.batches[b][k];
            lay.batch[b].ranges[k] = {(uint32_t)(p.op[rg.oracle].off + 8 * (size_t)rg.first), rg.count};
        }
    }
    return true;
}

constexpr size_t CHUNK_PROOFS = 1024;
constexpr size_t CHUNK_BYTES = (size_t)256 << 20;

}  // namespace

extern "C" int qpgpu_fri_verify_many_device(const qpgpu_fri_verifier *v, qpgpu_ctx *ctx, size_t count, const uint64_t *const *caps,
                                            const uint32_t *cap_counts, const uint64_t *points, const uint64_t *openings, const uint64_t *alphas,
                                            const uint64_t *betas, const uint64_t *pow_responses, const uint64_t *indices,
                                            const uint8_t *const *proofs, const size_t *lens, int *results, char *reasons, char *err) {
    if (!v || !ctx) return verify::fail(err, QPGPU_EINVAL, "null argument");
    if (count == 0) return QPGPU_OK;
    const friv::Instance &in = v->in;
    const size_t n_oracles = in.widths.size(), n_rounds = in.arity_bits.size(), n_batches = in.batches.size(), cap_words = in.cap_words();
    if (!caps || !cap_counts || !points || !openings || !alphas || !pow_responses || !indices || !proofs || !lens || !results || (n_rounds && !betas))
        return verify::fail(err, QPGPU_EINVAL, "null argument");
    if (!verify::same_hasher(v->hash, ctx->hasher)) {
        ctx->fail(QPGPU_EINVAL, "fri_verify_many_device: the verifier's hasher is not the context's (qpgpu_ctx_set_hasher)");
        return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
    }
    for (size_t o = 0; o < n_oracles; o++) {
        if (cap_counts[o] != 1 && cap_counts[o] != count) {
            ctx->fail(QPGPU_EINVAL, "fri_verify_many_device: oracle " + std::to_string(o) + " holds " + std::to_string(cap_counts[o]) +
                                        " caps, the call is for a batch of " + std::to_string(count));
            return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
        }
        if (!caps[o]) return verify::fail(err, QPGPU_EINVAL, "null argument");
    }
    FvLayout lay;
    if (!make_layout(in, lay)) {
        ctx->fail(QPGPU_EINVAL, "fri_verify_many_device: instance outside the supported range (16 oracles, 16 rounds, 8 batches)");
        return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
    }
    const unsigned threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    const size_t SW = lay.stride_words, RW = lay.rec_words, nq = lay.nq, n_open = n_oracles + n_rounds, n_openings = v->n_openings;
    const size_t chunk = std::max<size_t>(1, std::min(std::min(CHUNK_PROOFS, count), CHUNK_BYTES / (SW * 8)));
    // chunk layout, host and device alike: the cap area (an oracle's cap once, or one per proof of a full chunk), the chunk's
    // proofs (SW words each), its records (RW words each)
    size_t cap_area = 0;
    for (size_t o = 0; o < n_oracles; o++) {
        const bool shared = cap_counts[o] == 1 && count != 1;
        lay.op[o].cap_off = (uint32_t)cap_area;
        lay.op[o].cap_stride = shared ? 0 : (uint32_t)cap_words;
        cap_area += shared ? cap_words : chunk * cap_words;
    }
    const size_t pin_bytes = (cap_area + chunk * (SW + RW)) * 8;
    const size_t mcode_off = (pin_bytes + 255) & ~(size_t)255, qcode_off = (mcode_off + chunk * nq * n_open + 255) & ~(size_t)255;
    const size_t dev_bytes = qcode_off + chunk * nq * 4;
    std::vector<uint32_t> qcodes(chunk * nq);
    std::vector<char> own_reasons;          // the caller's rows, or rows of our own for err
    if (!reasons) own_reasons.assign(count * QPGPU_VERIFY_ERR_CAP, 0);
    char *const rows = reasons ? reasons : own_reasons.data();
    auto reason_row = [&](size_t i) { return rows + i * QPGPU_VERIFY_ERR_CAP; };

    // a HIP failure: the proofs not yet decided get QPGPU_EDEVICE; err carries the context's message. Proofs below `headed`
    // whose result is not EDEVICE were decided on the host.
    size_t chunk_from = 0, headed = 0;
    auto device_fail = [&](int rc) {
        for (size_t i = chunk_from; i < count; i++)
            if (i >= headed || results[i] == QPGPU_EDEVICE) { results[i] = QPGPU_EDEVICE; reason_row(i)[0] = 0; }
        return verify::fail(err, rc, "%s", ctx->err.c_str());
    };
    {
        const hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "hipSetDevice"));
    }
    if (int rc = merkle_ensure_constants(ctx)) return device_fail(rc);
    if (pin_bytes > ctx->vd_pin_bytes) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && ctx->vd_pin) { ctx->track_free(ctx->vd_pin); ctx->vd_pin = nullptr; ctx->vd_pin_bytes = 0; }
        if (e == hipSuccess) e = ctx->track_host_malloc(&ctx->vd_pin, pin_bytes, residue::VERIFY_STAGING);
        if (e != hipSuccess) { ctx->vd_pin = nullptr; return device_fail(ctx->hip_fail(e, "hipHostMalloc (verification staging)")); }
        ctx->vd_pin_bytes = pin_bytes;
    }
    if (dev_bytes > ctx->vd_dev_bytes) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && ctx->vd_dev) { ctx->track_free(ctx->vd_dev); ctx->vd_dev = nullptr; ctx->vd_dev_bytes = 0; }
        if (e == hipSuccess) e = ctx->track_malloc(&ctx->vd_dev, dev_bytes, residue::VERIFY_STAGING);
        if (e != hipSuccess) { ctx->vd_dev = nullptr; return device_fail(ctx->hip_fail(e, "hipMalloc (verification workspace)")); }
        ctx->vd_dev_bytes = dev_bytes;
    }
    uint8_t *const dev = (uint8_t *)ctx->vd_dev;
    u64 *const pin = (u64 *)ctx->vd_pin;
    std::memset(pin, 0, cap_area * 8);      // the slots of proofs that are not staged are uploaded with their chunk

    for (size_t c0 = 0; c0 < count; c0 += chunk) {
        const size_t n = std::min(chunk, count - c0);
        chunk_from = headed = c0;
        u64 *const h_caps = pin, *const h_proofs = pin + cap_area, *const h_recs = h_proofs + n * SW;
        for (size_t o = 0; o < n_oracles; o++)
            if (lay.op[o].cap_stride == 0) std::memcpy(h_caps + lay.op[o].cap_off, caps[o], cap_words * 8);

        // ---- phase 1: what comes before the query rounds, on host threads; the survivors staged ----
        std::atomic<size_t> next{0};
        auto work = [&] {
            char local[QPGPU_VERIFY_ERR_CAP];
            friv::Prepared p;
            std::vector<const u64 *> own(n_oracles);
            for (size_t k = next.fetch_add(1); k < n; k = next.fetch_add(1)) {
                const size_t i = c0 + k;
                u64 *rec = h_recs + k * RW;
                rec[FREC_LIVE] = 0;
                char *row = reason_row(i);
                row[0] = 0;
                if (!proofs[i]) { results[i] = verify::fail(row, QPGPU_EINVAL, "fri_verify: null argument"); continue; }
                for (size_t o = 0; o < n_oracles; o++) own[o] = caps[o] + (cap_counts[o] == 1 ? 0 : i * cap_words);
                local[0] = 0;
                const int rc = friv::prepare(v, own.data(), points + 2 * i, 2 * count, openings + 2 * n_openings * i, alphas + 2 * i,
                                             betas ? betas + 2 * n_rounds * i : nullptr, pow_responses[i], indices + nq * i, proofs[i], lens[i], local, p);
                if (rc != QPGPU_OK) { results[i] = rc; std::memcpy(row, local, QPGPU_VERIFY_ERR_CAP); continue; }
                u64 *dst = h_proofs + k * SW;
                dst[SW - 2] = 0; dst[SW - 1] = 0;          // the partial last word and the padding word
                std::memcpy(dst, proofs[i], lens[i]);
                for (size_t o = 0; o < n_oracles; o++)
                    if (lay.op[o].cap_stride) std::memcpy(h_caps + lay.op[o].cap_off + k * cap_words, own[o], cap_words * 8);
                rec[FREC_ALPHA] = p.alpha.a; rec[FREC_ALPHA + 1] = p.alpha.b;
                for (size_t b = 0; b < n_batches; b++) {
                    const gl::e2 shift = gl::e2_pow(p.alpha, in.batch_count(b)), ex[3] = {p.points[b], p.reduced[b], shift};
                    for (int e = 0; e < 3; e++) { rec[FREC_BATCHES + FREC_BATCH_WORDS * b + 2 * e] = ex[e].a; rec[FREC_BATCHES + FREC_BATCH_WORDS * b + 2 * e + 1] = ex[e].b; }
                }
                u64 *rb = rec + frec_betas((uint32_t)n_batches);
                for (size_t r = 0; r < n_rounds; r++) { rb[2 * r] = p.betas[r].a; rb[2 * r + 1] = p.betas[r].b; }
                for (size_t q = 0; q < nq; q++) rb[2 * n_rounds + q] = indices[nq * i + q];
                rec[FREC_LIVE] = 1;
                results[i] = QPGPU_EDEVICE;                 // until the device has decided
            }
        };
        const unsigned nt = (unsigned)std::min<size_t>(threads, n);
        std::vector<std::thread> pool;
        try {
            for (unsigned t = 1; t < nt; t++) pool.emplace_back(work);
        } catch (...) {}                 // no more threads to be had: the ones that started (and this one) drain the queue
        work();
        for (auto &t : pool) t.join();
        headed = c0 + n;
        bool any = false;
        for (size_t k = 0; k < n && !any; k++) any = h_recs[k * RW + FREC_LIVE] != 0;
        if (!any) continue;

        // ---- phase 2: one copy of the chunk, the query-round kernels, the verdicts back ----
        const size_t bytes = (cap_area + n * (SW + RW)) * 8;
        hipError_t e = hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "hipMemcpyAsync (proofs of the chunk)"));
        const u64 *d_caps = (const u64 *)dev, *d_proofs = d_caps + cap_area, *d_recs = d_proofs + n * SW;
        uint8_t *d_mcodes = dev + mcode_off;
        uint32_t *d_qcodes = (uint32_t *)(dev + qcode_off);
        ctx->prof_begin("fri_verify_many_device.query");
        e = fri_verify_query_rounds(lay, d_proofs, d_recs, d_caps, (uint32_t)n, d_mcodes, d_qcodes, ctx->hasher_dev(), ctx->stream);
        ctx->prof_end();
        if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "fri_verify_query_rounds"));
        if (int rc = ctx->read_back(qcodes.data(), d_qcodes, n * nq * 4)) return device_fail(rc);

        // ---- phase 3: the first failing check of each proof, in the host verifier's words ----
        for (size_t k = 0; k < n; k++) {
            if (h_recs[k * RW + FREC_LIVE] == 0) continue;
            const size_t i = c0 + k;
            results[i] = QPGPU_OK;
            for (size_t q = 0; q < nq; q++) {
                const uint32_t code = qcodes[k * nq + q];
                if (!code) continue;
                results[i] = QPGPU_EVERIFY;
                friv::query_reason(reason_row(i), q, code);
                break;
            }
        }
    }
    for (size_t i = 0; i < count; i++)
        if (results[i]) return verify::fail(err, results[i], "proof %zu: %.170s", i, reason_row(i));
    return QPGPU_OK;
}
