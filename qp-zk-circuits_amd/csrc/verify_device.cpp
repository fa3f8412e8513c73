// verify_device.cpp — qpgpu_verifier_verify_many_device (include/qpgpu_verify.h): verify_many with the query rounds of every
// proof on the context's GPU. Three phases per chunk of proofs:
//   1. on host threads, the head of verification (verifier.cpp: verify_head — parse, transcript, proof of work, quotient
//      identity, query indices); a proof that passes is copied into the pinned staging buffer with its record (VerifyLayout)
//   2. one host-to-device copy of the chunk, the query-round kernels (verify_kernels.hip), the per-query verdicts read back
//      through the context's pinned read-back
//   3. per proof, the first failing query's verdict written out in the host verifier's words
// The verdict and reason of every proof are the host verifier's (qpgpu_verifier_verify); the host query loop is the specification.
//
// qpgpu_verifier_verify_many_device_ex with QPGPU_VERIFY_HEAD_ON_DEVICE moves phase 1 to the device as well
// (verify_head_kernels.hip): the host checks pointer and length, copies the proof into the pinned chunk and, once per call,
// states the layout and asks verify_math.hpp whether the pack's gate table is consistent; the transcript, the proof of work and
// the quotient identity are kernels, and a proof goes from bytes to verdict without the host reading its contents.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../include/qpgpu.h"
#include "../../include/qpgpu_verify.h"
#include "ctx.hpp"
#include "verifier.hpp"
#include "verify_kernels.hpp"
#include "verify_math.hpp"

using gl::u64;

namespace {

// the proof layout (proof_layout.hpp) as the kernels read it, and the strides of the device buffer
bool make_layout(const CircuitPack &c, const proof_layout::Proof &p, VerifyLayout &lay) {
    const size_t n_rounds = c.arity_bits.size();
    if (n_rounds > (size_t)VERIFY_MAX_ROUNDS || p.total >= ((size_t)1 << 31)) return false;
    memset(&lay, 0, sizeof lay);
    for (size_t i = 0; i < 4 + n_rounds; i++) {
        const proof_layout::Opening &o = p.fri.op[i];
        // the cap an opening leads to: the verifier's own, a cap at the head of the proof, the FRI round's
        const size_t cap_off = i == 0 ? VERIFY_CAP_VERIFIER : i < 4 ? (i - 1) * p.cap_bytes : p.fri_caps_pos + (i - 4) * p.cap_bytes;
        lay.op[i] = {(uint32_t)o.off, (uint32_t)o.row_words, (uint32_t)o.path_len, (uint32_t)o.shift, (uint32_t)cap_off};
    }
    for (int o = 0; o < 4; o++) lay.polys[o] = (uint32_t)p.polys[o];
    for (size_t r = 0; r < n_rounds; r++) lay.arity_bits[r] = (uint32_t)c.arity_bits[r];
    lay.nq = (uint32_t)c.num_query_rounds;
    lay.n_open = (uint32_t)(4 + n_rounds);
    lay.queries_pos = (uint32_t)p.queries_pos;
    lay.q_bytes = (uint32_t)p.fri.round_bytes;
    lay.final_off = (uint32_t)p.final_pos;
    lay.final_n = (uint32_t)p.fri.final_len;
    lay.stride_words = (uint32_t)((p.total + 7) / 8 + 1);
    lay.rec_words = vrec_words((uint32_t)n_rounds, lay.nq);
    lay.log_lde = (uint32_t)(c.degree_bits + c.rate_bits);
    lay.nch = (uint32_t)c.num_challenges;
    return true;
}

// what the head kernels read, beyond VerifyLayout; false: a gate beyond the bounds of the device code's local arrays
bool make_head_layout(const qpgpu_verifier *v, const VerifyLayout &lay, HeadLayout &hl, std::string &pack_why) {
    const CircuitPack &c = v->pack;
    const proof_layout::Proof &p = v->layout;
    if (c.num_challenges > 4 || c.gates.size() > 60000) return false;
    for (const GateInfo &g : c.gates)
        if (g.type == GATE_RANDOM_ACCESS && g.param0 > vmath::MAX_RANDOM_ACCESS_BITS) return false;
    hl = HeadLayout();
    hl.cap_words = (uint32_t)(p.cap_bytes / 8);
    hl.n_rounds = (uint32_t)c.arity_bits.size();
    for (int i = 0; i < 7; i++) { hl.open_pos[i] = (uint32_t)p.openings[i].pos; hl.open_cnt[i] = (uint32_t)p.openings[i].count; }
    hl.fri_caps_pos = (uint32_t)p.fri_caps_pos; hl.final_pos = (uint32_t)p.final_pos; hl.pow_pos = (uint32_t)p.pow_pos;
    hl.pis_pos = (uint32_t)p.pis_pos; hl.n_pis = (uint32_t)c.num_public_inputs; hl.total = (uint32_t)p.total;
    hl.degree_bits = (uint32_t)c.degree_bits; hl.pow_bits = (uint32_t)c.proof_of_work_bits;
    hl.num_selectors = (uint32_t)c.num_selectors; hl.num_constants = (uint32_t)c.num_constants; hl.num_routed = (uint32_t)c.num_routed_wires;
    hl.num_pp = (uint32_t)c.num_partial_products; hl.qdf = (uint32_t)c.quotient_degree_factor;
    hl.n_gates = (uint32_t)c.gates.size(); hl.n_slots = hl.n_gates + 2;
    hl.gate_term0 = (uint32_t)(c.num_challenges * (2 + c.num_partial_products));
    hl.hrec_words = HREC_WORDS;
    std::memcpy(hl.digest, c.circuit_digest, sizeof hl.digest);
    hl.p2 = c.p2_layout;
    pack_why = v->pack_why;      // vanishing_at_zeta's check of the gate table, asked once when the verifier was created
    hl.pack_bad = pack_why.empty() ? 0 : 1;
    return true;
}

// the host verifier's words for a head verdict (verifier.cpp: verify_head)
void head_reason(char *out, uint32_t code, const CircuitPack &c, const std::string &pack_why) {
    switch (code >> 8) {
    case VH_NONCANONICAL: verify::fail(out, 0, "proof holds a non-canonical field element"); break;
    case VH_POW: verify::fail(out, 0, "proof-of-work response has fewer than %llu leading zero bits", (unsigned long long)c.proof_of_work_bits); break;
    case VH_PACK: verify::fail(out, 0, "%s", pack_why.c_str()); break;
    default: verify::fail(out, 0, "quotient identity fails at zeta (challenge %zu): the openings do not satisfy the circuit", (size_t)(code & 0xff)); break;
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void host_stat(qpgpu_ctx *ctx, const char *name, double ms) {
    if (!ctx->profiling) return;
    ctx->kstats[name].ms += ms;
    ctx->kstats[name].launches++;
}

constexpr size_t CHUNK_PROOFS = 1024;
constexpr size_t CHUNK_BYTES = (size_t)256 << 20;

}  // namespace

extern "C" int qpgpu_verifier_verify_many_device(const qpgpu_verifier *v, qpgpu_ctx *ctx, const uint8_t *const *proofs, const size_t *lens,
                                                 size_t count, unsigned threads, int *results, char *reasons, char *err) {
    return qpgpu_verifier_verify_many_device_ex(v, ctx, proofs, lens, count, threads, 0, results, reasons, err);
}

extern "C" int qpgpu_verifier_verify_many_device_ex(const qpgpu_verifier *v, qpgpu_ctx *ctx, const uint8_t *const *proofs, const size_t *lens,
                                                    size_t count, unsigned threads, unsigned flags, int *results, char *reasons, char *err) {
    if (!v || !ctx) return verify::fail(err, QPGPU_EINVAL, "null argument");
    if (flags & ~(unsigned)QPGPU_VERIFY_HEAD_ON_DEVICE) return verify::fail(err, QPGPU_EINVAL, "verify_many_device: unknown flag");
    const bool device_head = (flags & QPGPU_VERIFY_HEAD_ON_DEVICE) != 0;
    if (count == 0) return QPGPU_OK;
    if (!proofs || !lens || !results) return verify::fail(err, QPGPU_EINVAL, "null argument");
    if (!verify::same_hasher(v->hash, ctx->hasher)) {
        ctx->fail(QPGPU_EINVAL, "verify_many_device: the verifier's hasher is not the context's (qpgpu_ctx_set_hasher)");
        return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
    }
    VerifyLayout lay;
    if (!make_layout(v->pack, v->layout, lay)) {
        ctx->fail(QPGPU_EINVAL, "verify_many_device: circuit outside the supported range");
        return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
    }
    HeadLayout hl;
    std::string pack_why;
    if (device_head && !make_head_layout(v, lay, hl, pack_why)) {
        ctx->fail(QPGPU_EINVAL, "verify_many_device: circuit outside the supported range");
        return verify::fail(err, QPGPU_EINVAL, "%s", ctx->err.c_str());
    }
    if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
    const size_t cap_words = v->cs_cap.size(), SW = lay.stride_words, RW = lay.rec_words, nq = lay.nq;
    // device head: the gate table (GateInfo, 8 words each) and k_is travel behind the cap
    const size_t table_words = device_head ? 8 * v->pack.gates.size() + v->pack.k_is.size() : 0;
    const size_t chunk = std::max<size_t>(1, std::min(CHUNK_PROOFS, CHUNK_BYTES / (SW * 8)));
    const size_t pin_bytes = (chunk * (SW + RW) + cap_words + table_words) * 8;
    const size_t mcode_off = (pin_bytes + 255) & ~(size_t)255, qcode_off = (mcode_off + chunk * nq * lay.n_open + 255) & ~(size_t)255;
    // the head verdicts sit right behind the query verdicts of the chunk's proofs (one read-back); head records and slots follow
    const size_t hrec_off = (qcode_off + chunk * (nq + 1) * 4 + 255) & ~(size_t)255;
    const size_t part_off = hrec_off + (device_head ? chunk * HREC_WORDS * 8 : 0);
    const size_t dev_bytes = part_off + (device_head ? chunk * hl.n_slots * VERIFY_PARTIAL_WORDS * 8 : 0);
    std::vector<uint32_t> qcodes(chunk * (nq + 1));
    std::vector<uint8_t> staged(device_head ? chunk : 0);
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

    for (size_t c0 = 0; c0 < count; c0 += chunk) {
        const size_t n = std::min(chunk, count - c0);
        chunk_from = headed = c0;
        // chunk layout, host and device alike: n proofs (SW words each), n records (RW words each), the constants/sigmas cap
        u64 *const h_proofs = pin, *const h_recs = pin + n * SW, *const h_cap = h_recs + n * RW;
        std::memcpy(h_cap, v->cs_cap.data(), cap_words * 8);
        if (device_head) {
            u64 *h_table = h_cap + cap_words;
            std::memcpy(h_table, v->pack.gates.data(), 8 * v->pack.gates.size() * 8);
            std::memcpy(h_table + 8 * v->pack.gates.size(), v->pack.k_is.data(), v->pack.k_is.size() * 8);
        }

        // ---- phase 1: the head of every proof on host threads; the survivors staged ----
        auto t0 = std::chrono::steady_clock::now();
        std::atomic<size_t> next{0};
        // device head: pointer and length are all the host looks at; the proof is copied, its head is the device's
        auto stage = [&] {
            for (size_t k = next.fetch_add(1); k < n; k = next.fetch_add(1)) {
                const size_t i = c0 + k;
                u64 *rec = h_recs + k * RW;
                rec[VREC_LIVE] = 0;
                staged[k] = 0;
                char *row = reason_row(i);
                row[0] = 0;
                if (!proofs[i]) { results[i] = QPGPU_EINVAL; continue; }
                if (lens[i] != v->layout.total) {
                    results[i] = verify::fail(row, QPGPU_EVERIFY, "proof has %zu bytes, this circuit's proofs have %zu", lens[i], v->layout.total);
                    continue;
                }
                u64 *dst = h_proofs + k * SW;
                dst[SW - 2] = 0; dst[SW - 1] = 0;
                std::memcpy(dst, proofs[i], lens[i]);
                rec[VREC_LIVE] = 1;
                staged[k] = 1;
                results[i] = QPGPU_EDEVICE;
            }
        };
        auto head_work = [&] {
            char local[QPGPU_VERIFY_ERR_CAP];
            VerifyHead h;
            for (size_t k = next.fetch_add(1); k < n; k = next.fetch_add(1)) {
                const size_t i = c0 + k;
                u64 *rec = h_recs + k * RW;
                rec[VREC_LIVE] = 0;
                char *row = reason_row(i);
                row[0] = 0;
                if (!proofs[i]) { results[i] = QPGPU_EINVAL; continue; }
                local[0] = 0;
                const int rc = verify_head(v, proofs[i], lens[i], local, h);
                if (rc != QPGPU_OK) { results[i] = rc; std::memcpy(row, local, QPGPU_VERIFY_ERR_CAP); continue; }
                u64 *dst = h_proofs + k * SW;
                dst[SW - 2] = 0; dst[SW - 1] = 0;          // the partial last word and the padding word
                std::memcpy(dst, proofs[i], lens[i]);
                const gl::e2 ex[6] = {h.zeta, h.g_zeta, h.fri_alpha, h.alpha_nch, h.red0, h.red1};
                for (int e = 0; e < 6; e++) { rec[1 + 2 * e] = ex[e].a; rec[2 + 2 * e] = ex[e].b; }
                for (size_t r = 0; r < h.fri_betas.size(); r++) { rec[VREC_BETAS + 2 * r] = h.fri_betas[r].a; rec[VREC_BETAS + 2 * r + 1] = h.fri_betas[r].b; }
                for (size_t q = 0; q < nq; q++) rec[VREC_BETAS + 2 * h.fri_betas.size() + q] = h.x_indices[q];
                rec[VREC_LIVE] = 1;
                results[i] = QPGPU_EDEVICE;                 // until the device has decided
            }
        };
        auto work = [&] { if (device_head) stage(); else head_work(); };
        const unsigned nt = (unsigned)std::min<size_t>(threads, n);
        std::vector<std::thread> pool;
        try {
            for (unsigned t = 1; t < nt; t++) pool.emplace_back(work);
        } catch (...) {}                 // no more threads to be had: the ones that started (and this one) drain the queue
        work();
        for (auto &t : pool) t.join();
        headed = c0 + n;
        host_stat(ctx, device_head ? "verify_many_device.copy" : "verify_many_device.head", ms_since(t0));
        bool any = false;
        for (size_t k = 0; k < n && !any; k++) any = h_recs[k * RW + VREC_LIVE] != 0;
        if (!any) continue;

        // ---- phase 2: one copy of the chunk, the query-round kernels, the verdicts back ----
        t0 = std::chrono::steady_clock::now();
        const size_t bytes = (n * (SW + RW) + cap_words + table_words) * 8;
        hipError_t e = hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "hipMemcpyAsync (proofs of the chunk)"));
        if (ctx->profiling) {
            if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return device_fail(ctx->hip_fail(e, "hipStreamSynchronize"));
            host_stat(ctx, "verify_many_device.upload", ms_since(t0));
            t0 = std::chrono::steady_clock::now();
        }
        const u64 *d_proofs = (const u64 *)dev, *d_cap = d_proofs + n * (SW + RW);
        u64 *d_recs = (u64 *)dev + n * SW;
        uint8_t *d_mcodes = dev + mcode_off;
        uint32_t *d_qcodes = (uint32_t *)(dev + qcode_off), *d_hcodes = d_qcodes + n * nq;
        if (device_head) {     // the records are the device's: transcript, identity slots, verdict; a rejected proof leaves not live
            u64 *d_hrecs = (u64 *)(dev + hrec_off), *d_parts = (u64 *)(dev + part_off);
            ctx->prof_begin("verify_many_device.transcript");
            e = verify_head_transcript(lay, hl, d_proofs, d_recs, d_hrecs, (uint32_t)n, ctx->hasher_dev(), ctx->stream);
            ctx->prof_end();
            if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "verify_head_transcript"));
            ctx->prof_begin("verify_many_device.identity");
            e = verify_head_identity(lay, hl, d_proofs, d_recs, d_hrecs, d_cap + cap_words, d_parts, (uint32_t)n, ctx->stream);
            if (e == hipSuccess) e = verify_head_verdict(lay, hl, d_recs, d_hrecs, d_parts, d_hcodes, (uint32_t)n, ctx->stream);
            ctx->prof_end();
            if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "verify_head_identity"));
        }
        ctx->prof_begin("verify_many_device.query");
        e = verify_query_rounds(lay, d_proofs, d_recs, d_cap, (uint32_t)n, d_mcodes, d_qcodes, ctx->hasher_dev(), ctx->stream);
        ctx->prof_end();
        if (e != hipSuccess) return device_fail(ctx->hip_fail(e, "verify_query_rounds"));
        if (int rc = ctx->read_back(qcodes.data(), d_qcodes, n * (nq + (device_head ? 1 : 0)) * 4)) return device_fail(rc);
        host_stat(ctx, "verify_many_device.kernels", ms_since(t0));

        // ---- phase 3: the first failing check of each proof, in the host verifier's words ----
        t0 = std::chrono::steady_clock::now();
        for (size_t k = 0; k < n; k++) {
            if (!(device_head ? staged[k] != 0 : h_recs[k * RW + VREC_LIVE] != 0)) continue;
            const size_t i = c0 + k;
            if (device_head && qcodes[n * nq + k]) {
                results[i] = QPGPU_EVERIFY;
                head_reason(reason_row(i), qcodes[n * nq + k], v->pack, pack_why);
                continue;
            }
            results[i] = QPGPU_OK;
            for (size_t q = 0; q < nq; q++) {
                const uint32_t code = qcodes[k * nq + q];
                if (!code) continue;
                results[i] = QPGPU_EVERIFY;
                friv::query_reason(reason_row(i), q, code);
                break;
            }
        }
        host_stat(ctx, "verify_many_device.reasons", ms_since(t0));
    }
    for (size_t i = 0; i < count; i++)
        if (results[i]) return verify::fail(err, QPGPU_EVERIFY, "proof %zu: %.170s", i, reason_row(i));
    return QPGPU_OK;
}
