// oracle_api.cpp — stage-level C ABI: polynomial-batch commitments, their opening evaluations and Merkle openings, and the
// challenger as separate calls (include/qpgpu.h, "stage-level entry points"; the FRI opening proof is fri_api.cpp). These are the
// circuit-independent parts of qp-plonky2's prove(); a patched prover can keep its gate evaluation in Rust and use these for the rest.
// An oracle holds one proof's batch of polynomials (qpgpu_oracle_commit) or those of the proofs of a lockstep batch, as dense
// [batch][...] arrays (qpgpu_oracle_commit_batch; the _batch entries read them with one launch for all proofs).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include "merkle.hpp"
#include "oracle_handle.hpp"
#include "prover_host.hpp"
#include "prover_kernels.hpp"

using gl::e2;
using gl::u64;

extern "C" void qpgpu_oracle_free(qpgpu_oracle *h) {
    if (!h) return;
    if (h->sh) { oracle_sharded_free(h); return; }
    (void)hipSetDevice(h->ctx->device);
    if (h->block) {
        // committed columns can hold the witness (reference wormhole/circuit/src/sensitive.rs:36-44): scrub before release
        (void)hipMemsetAsync(h->block, 0, h->block_words * 8, h->ctx->stream);
        (void)hipStreamSynchronize(h->ctx->stream);
        h->ctx->track_free(h->block);
    }
    delete h;
}

namespace {

// what qpgpu_oracle_commit and qpgpu_oracle_commit_batch share: `batch` proofs' matrices into one dense [batch][...] oracle
int commit_impl(qpgpu_ctx *ctx, const uint64_t *const *polys, uint32_t batch, uint32_t num_polys, unsigned degree_bits, unsigned rate_bits,
                unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream, qpgpu_oracle **out) {
    if (degree_bits + rate_bits > 23 || degree_bits < 1)
        return ctx->fail(QPGPU_EINVAL, "oracle_commit: LDE sizes up to 2^23 supported");
    if (cap_height > degree_bits + rate_bits) return ctx->fail(QPGPU_EINVAL, "oracle_commit: cap_height exceeds the tree height");
    if (flags & ~7u) return ctx->fail(QPGPU_EINVAL, "oracle_commit: unknown flags");
    ctx->hasher_in_use = true;
    QP_TRY(merkle_ensure_constants(ctx));
    const bool blinding = (flags & QPGPU_ORACLE_BLINDING) != 0, from_coeffs = (flags & QPGPU_ORACLE_COEFFS) != 0;
    const u64 n = 1ull << degree_bits, lde_n = n << rate_bits;
    const unsigned L = degree_bits + rate_bits;
    const size_t B = batch;
    qpgpu_oracle *h = new qpgpu_oracle();
    h->ctx = ctx;
    PolyOracle &o = h->o;
    o.ncols = num_polys; o.log_n = degree_bits; o.rate_bits = rate_bits; o.cap_h = cap_height; o.oracle_index = blinding_stream;
    // per proof; the areas are [batch][...] arrays, the evaluation scratch and the salt keys grow with the batch too
    const size_t w_coeffs = (size_t)num_polys * n, w_lde = (size_t)num_polys * lde_n, w_dig = digest_words(L, cap_height),
                 w_salt = blinding ? (size_t)4 * lde_n : 0, w_eval = 2 + 2 * (size_t)num_polys;
    h->block_words = B * (w_coeffs + w_lde + w_dig + w_salt + w_eval + 4);
    void *v = nullptr;
    hipError_t e = ctx->track_malloc(&v, h->block_words * 8, residue::ORACLE);
    if (e != hipSuccess) { delete h; return ctx->hip_fail(e, "hipMalloc(oracle)"); }
    h->block = (u64 *)v;
    o.coeffs = h->block; o.lde = o.coeffs + B * w_coeffs; o.digests = o.lde + B * w_lde;
    o.salt = blinding ? o.digests + B * w_dig : nullptr;
    h->d_point = (e2 *)(o.digests + B * (w_dig + w_salt)); h->d_eval = h->d_point + B;
    h->d_key = (uint32_t *)(o.digests + B * (w_dig + w_salt + w_eval));
    o.set_batch(batch, batch == 1);
    int rc = QPGPU_OK;
    if (blinding) {
        // blinding_seed 0: 256 fresh bits per proof from the OS entropy source (the reference: thread_rng); otherwise proof b's key
        // is derived from seed + b (qpgpu_circuit_set_blinding_seed's rule for a batch), which makes the commitment reproducible (tests)
        std::vector<uint32_t> keys(8 * B);
        for (size_t b = 0; b < B && rc == QPGPU_OK; b++) {
            if (blinding_seed) salt_key_from_seed(blinding_seed + b, keys.data() + 8 * b);
            else if (salt_key_random(keys.data() + 8 * b) != QPGPU_OK) rc = ctx->fail(QPGPU_EDEVICE, "oracle_commit: the OS entropy source failed");
        }
        if (rc == QPGPU_OK) {
            e = hipMemcpyAsync(h->d_key, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) rc = ctx->hip_fail(e, "oracle_commit: key upload");
        }
        volatile uint32_t *kz = keys.data();          // the keys are secrets: the host copy goes as soon as the device has them
        for (size_t i = 0; i < keys.size(); i++) kz[i] = 0;
    }
    bool dense = true;
    for (size_t b = 0; b < B; b++) dense = dense && polys[b] == polys[0] + b * w_coeffs;
    const u64 *src = polys[0];
    if (rc == QPGPU_OK && !(flags & QPGPU_ORACLE_DEVICE_INPUT)) {
        // stage through the LDE area (large enough, overwritten afterwards); a coefficient input goes straight to its place
        u64 *dst = from_coeffs ? o.coeffs : o.lde;
        e = hipSuccess;
        if (dense) e = hipMemcpyAsync(dst, polys[0], B * w_coeffs * 8, hipMemcpyHostToDevice, ctx->stream);
        else for (size_t b = 0; b < B && e == hipSuccess; b++) e = hipMemcpyAsync(dst + b * w_coeffs, polys[b], w_coeffs * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { rc = ctx->hip_fail(e, "oracle_commit: upload"); }
        src = dst;
    } else if (rc == QPGPU_OK && (from_coeffs || !dense)) {
        // device matrices: coefficients are copied to their place; values that do not lie back to back are gathered in the LDE area
        u64 *dst = from_coeffs ? o.coeffs : o.lde;
        e = hipSuccess;
        if (dense) e = hipMemcpyAsync(dst, polys[0], B * w_coeffs * 8, hipMemcpyDeviceToDevice, ctx->stream);
        else for (size_t b = 0; b < B && e == hipSuccess; b++) e = hipMemcpyAsync(dst + b * w_coeffs, polys[b], w_coeffs * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) rc = ctx->hip_fail(e, "oracle_commit: copy");
        src = dst;
    }
    if (rc == QPGPU_OK) rc = from_coeffs ? oracle_commit_coeffs(ctx, o, h->d_key) : oracle_commit_values(ctx, src, o, h->d_key);
    if (rc != QPGPU_OK) { qpgpu_oracle_free(h); return rc; }
    *out = h;
    return QPGPU_OK;
}

// the single-proof read entries do not silently serve proof 0 of a batched oracle
int refuse_batched(const qpgpu_oracle *h, const char *entry) {
    return h->ctx->fail(QPGPU_EINVAL, std::string(entry) + ": the oracle holds a batch of " + std::to_string(h->o.nb) + " proofs, use qpgpu_" + entry + "_batch");
}

}  // namespace

extern "C" {

int qpgpu_oracle_commit(qpgpu_ctx *ctx, const uint64_t *polys, uint32_t num_polys, unsigned degree_bits, unsigned rate_bits,
                        unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream, qpgpu_oracle **out) {
    if (!ctx || !out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    *out = nullptr;
    if (!polys || num_polys == 0) return ctx->fail(QPGPU_EINVAL, "oracle_commit: no polynomials");
    return commit_impl(ctx, &polys, 1, num_polys, degree_bits, rate_bits, cap_height, flags, blinding_seed, blinding_stream, out);
}

int qpgpu_oracle_commit_batch(qpgpu_ctx *ctx, const uint64_t *const *polys, uint32_t batch, uint32_t num_polys, unsigned degree_bits,
                              unsigned rate_bits, unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream,
                              qpgpu_oracle **out) {
    if (!ctx || !out) return QPGPU_EINVAL;
    QP_DEV(ctx);
    *out = nullptr;
    if (batch == 0 || batch > 1024) return ctx->fail(QPGPU_EINVAL, "oracle_commit_batch: batch must be 1..1024");
    if (!polys || num_polys == 0) return ctx->fail(QPGPU_EINVAL, "oracle_commit: no polynomials");
    for (uint32_t b = 0; b < batch; b++)
        if (!polys[b]) return ctx->fail(QPGPU_EINVAL, "oracle_commit_batch: polys[" + std::to_string(b) + "] is NULL");
    return commit_impl(ctx, polys, batch, num_polys, degree_bits, rate_bits, cap_height, flags, blinding_seed, blinding_stream, out);
}

uint32_t qpgpu_oracle_batch(const qpgpu_oracle *h) { return h ? h->o.nb : 0; }

int qpgpu_oracle_strides(const qpgpu_oracle *h, uint64_t *coeffs, uint64_t *lde, uint64_t *digests) {
    if (!h) return QPGPU_EINVAL;
    if (coeffs) *coeffs = h->o.ps_coeffs;
    if (lde) *lde = h->o.ps_lde;
    if (digests) *digests = h->o.ps_digests;
    return QPGPU_OK;
}

int qpgpu_oracle_cap(const qpgpu_oracle *h, uint64_t *out, size_t out_words) {
    if (!h || !out || out_words < h->o.cap.size()) return QPGPU_EINVAL;
    std::memcpy(out, h->o.cap.data(), h->o.cap.size() * 8);
    return QPGPU_OK;
}

int qpgpu_oracle_eval(qpgpu_oracle *h, const uint64_t point[2], uint32_t first, uint32_t count, uint64_t *out) {
    if (!h) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = h->ctx;
    QP_DEV(ctx);
    if (h->o.nb > 1) return refuse_batched(h, "oracle_eval");
    if (!point || !out || count == 0 || (size_t)first + count > h->o.ncols) return ctx->fail(QPGPU_EINVAL, "oracle_eval: bad range");
    const e2 z = gl::e2_make(gl::canon(point[0]), gl::canon(point[1]));
    QP_HIP(ctx, hipMemcpyAsync(h->d_point, &z, sizeof z, hipMemcpyHostToDevice, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const u64 n = 1ull << h->o.log_n;
    QP_HIP(ctx, pk_poly_eval(h->o.coeffs + (size_t)first * n, n, count, h->d_point, 1, h->d_eval, 1, 0, 0, 0, ctx->stream));
    QP_HIP(ctx, hipMemcpyAsync(out, h->d_eval, (size_t)count * sizeof(e2), hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QPGPU_OK;
}

int qpgpu_oracle_read(qpgpu_oracle *h, unsigned what, uint32_t first, uint32_t count, uint64_t *out) {
    if (!h) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = h->ctx;
    QP_DEV(ctx);
    if (h->o.nb > 1) return ctx->fail(QPGPU_EINVAL, "oracle_read: the oracle holds a batch of " + std::to_string(h->o.nb) + " proofs, use qpgpu_oracle_device_ptrs and qpgpu_oracle_strides");
    if (!out || count == 0 || (size_t)first + count > h->o.ncols || what > QPGPU_ORACLE_READ_LDE) return ctx->fail(QPGPU_EINVAL, "oracle_read: bad range");
    if (h->sh && what == QPGPU_ORACLE_READ_LDE) return oracle_sharded_read_lde(h, first, count, out);
    const u64 len = what == QPGPU_ORACLE_READ_LDE ? h->o.lde_n() : 1ull << h->o.log_n;
    const u64 *src = (what == QPGPU_ORACLE_READ_LDE ? h->o.lde : h->o.coeffs) + (size_t)first * len;
    QP_HIP(ctx, hipMemcpyAsync(out, src, (size_t)count * len * 8, hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QPGPU_OK;
}

int qpgpu_oracle_device_ptrs(const qpgpu_oracle *h, const uint64_t **d_coeffs, const uint64_t **d_lde, const uint64_t **d_digests) {
    if (!h) return QPGPU_EINVAL;
    if (h->sh) return h->ctx->fail(QPGPU_EINVAL, "oracle_device_ptrs: the oracle is sharded over " + std::to_string(h->sh->s.size()) + " contexts, use qpgpu_oracle_shard_device_ptrs");
    if (d_coeffs) *d_coeffs = h->o.coeffs;
    if (d_lde) *d_lde = h->o.lde;
    if (d_digests) *d_digests = h->o.digests;
    return QPGPU_OK;
}

size_t qpgpu_oracle_leaf_width(const qpgpu_oracle *h) { return h ? (size_t)h->o.ncols + (h->o.salted() ? 4 : 0) : 0; }

int qpgpu_oracle_open(qpgpu_oracle *h, const uint64_t *indices, size_t n, uint64_t *rows_out, uint64_t *paths_out) {
    if (!h) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = h->ctx;
    QP_DEV(ctx);
    if (h->o.nb > 1) return refuse_batched(h, "oracle_open");
    if (n == 0) return QPGPU_OK;
    if (!indices) return ctx->fail(QPGPU_EINVAL, "oracle_open: indices is NULL");
    const PolyOracle &o = h->o;
    const u64 lde_n = o.lde_n();
    for (size_t i = 0; i < n; i++)
        if (indices[i] >= lde_n)
            return ctx->fail(QPGPU_EINVAL, "oracle_open: indices[" + std::to_string(i) + "] = " + std::to_string(indices[i]) + " is not below 2^" + std::to_string(o.log_lde()));
    if (h->sh) return oracle_sharded_open(o, indices, n, rows_out, paths_out);
    const uint32_t plen = o.log_lde() - o.cap_h;
    const size_t width = qpgpu_oracle_leaf_width(h), per = 1 + (rows_out ? width : 0) + (paths_out ? (size_t)plen * 4 : 0);
    if (per == 1) return QPGPU_OK;
    const size_t chunk = 256;                       // indices per pass: the gathers go through the context's scratch buffer
    QP_TRY(ctx->ensure_scratch(std::min(n, chunk) * per * 8));
    std::vector<u64> got;
    for (size_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - at);
        u64 *d_idx = ctx->scratch, *d_rows = d_idx + m, *d_salt = d_rows + (rows_out ? (size_t)o.ncols * m : 0),
            *d_paths = d_idx + m + (rows_out ? width * m : 0);
        QP_HIP(ctx, hipMemcpyAsync(d_idx, indices + at, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
        if (rows_out) {
            QP_HIP(ctx, pk_gather_rows(o.lde, lde_n, o.ncols, d_idx, m, d_rows, 1, 0, 0, ctx->stream));
            if (o.salt) QP_HIP(ctx, pk_gather_rows(o.salt, lde_n, 4, d_idx, m, d_salt, 1, 0, 0, ctx->stream));
        }
        if (paths_out) QP_HIP(ctx, pk_gather_paths(o.digests, lde_n, plen, d_idx, 0, m, d_paths, 1, 0, 0, ctx->stream));
        got.resize((size_t)m * (per - 1));
        QP_TRY(ctx->read_back(got.data(), d_rows, got.size() * 8));
        if (rows_out)
            for (uint32_t q = 0; q < m; q++) {      // the leaf as the proof carries it: the columns, then the salt
                std::memcpy(rows_out + (at + q) * width, got.data() + (size_t)q * o.ncols, (size_t)o.ncols * 8);
                if (o.salt) std::memcpy(rows_out + (at + q) * width + o.ncols, got.data() + (size_t)o.ncols * m + (size_t)q * 4, 32);
            }
        if (paths_out && plen) std::memcpy(paths_out + at * plen * 4, got.data() + (rows_out ? width * m : 0), (size_t)m * plen * 32);
    }
    return QPGPU_OK;
}

// ---- the same for the proofs of a batched oracle: one upload, one launch per gather, one read-back for all of them ----
int qpgpu_oracle_eval_batch(qpgpu_oracle *h, const uint64_t *points, uint32_t first, uint32_t count, uint64_t *out) {
    if (!h) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = h->ctx;
    QP_DEV(ctx);
    if (h->sh) return refuse_sharded(h, "oracle_eval_batch");
    if (!points || !out || count == 0 || (size_t)first + count > h->o.ncols) return ctx->fail(QPGPU_EINVAL, "oracle_eval_batch: bad range");
    const PolyOracle &o = h->o;
    const uint32_t nb = o.nb;
    std::vector<e2> z(nb);
    for (uint32_t b = 0; b < nb; b++) z[b] = gl::e2_make(gl::canon(points[2 * b]), gl::canon(points[2 * b + 1]));
    QP_HIP(ctx, hipMemcpyAsync(h->d_point, z.data(), nb * sizeof(e2), hipMemcpyHostToDevice, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const u64 n = 1ull << o.log_n;
    QP_HIP(ctx, pk_poly_eval(o.coeffs + (size_t)first * n, n, count, h->d_point, 1, h->d_eval, nb, o.ps_coeffs, 1, count, ctx->stream));
    QP_HIP(ctx, hipMemcpyAsync(out, h->d_eval, (size_t)nb * count * sizeof(e2), hipMemcpyDeviceToHost, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QPGPU_OK;
}

int qpgpu_oracle_open_batch(qpgpu_oracle *h, const uint64_t *indices, size_t n, uint64_t *rows_out, uint64_t *paths_out) {
    if (!h) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = h->ctx;
    QP_DEV(ctx);
    if (h->sh) return refuse_sharded(h, "oracle_open_batch");
    if (n == 0) return QPGPU_OK;
    if (!indices) return ctx->fail(QPGPU_EINVAL, "oracle_open_batch: indices is NULL");
    const PolyOracle &o = h->o;
    const size_t nb = o.nb;
    const u64 lde_n = o.lde_n();
    for (size_t b = 0; b < nb; b++)
        for (size_t i = 0; i < n; i++)
            if (indices[b * n + i] >= lde_n)
                return ctx->fail(QPGPU_EINVAL, "oracle_open_batch: indices[" + std::to_string(b) + "][" + std::to_string(i) + "] = " + std::to_string(indices[b * n + i]) +
                                                   " is not below 2^" + std::to_string(o.log_lde()));
    const uint32_t plen = o.log_lde() - o.cap_h;
    const size_t width = qpgpu_oracle_leaf_width(h), got_w = (rows_out ? width : 0) + (paths_out ? (size_t)plen * 4 : 0);
    if (got_w == 0) return QPGPU_OK;
    const size_t chunk = 256;                       // indices per proof and pass: the gathers go through the context's scratch buffer
    QP_TRY(ctx->ensure_scratch(nb * std::min(n, chunk) * (1 + got_w) * 8));
    std::vector<u64> got, idx;
    for (size_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - at);
        const size_t ps = got_w * m;                // one proof's gathered words: rows | salt | paths
        u64 *d_idx = ctx->scratch, *d_rows = d_idx + nb * m, *d_salt = d_rows + (rows_out ? (size_t)o.ncols * m : 0),
            *d_paths = d_rows + (rows_out ? width * m : 0);
        idx.resize(nb * m);
        for (size_t b = 0; b < nb; b++) std::memcpy(idx.data() + b * m, indices + b * n + at, (size_t)m * 8);
        QP_HIP(ctx, hipMemcpyAsync(d_idx, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        QP_HIP(ctx, hipStreamSynchronize(ctx->stream));     // idx is reused by the next pass
        if (rows_out) {
            QP_HIP(ctx, pk_gather_rows(o.lde, lde_n, o.ncols, d_idx, m, d_rows, (uint32_t)nb, o.ps_lde, ps, ctx->stream));
            if (o.salt) QP_HIP(ctx, pk_gather_rows(o.salt, lde_n, 4, d_idx, m, d_salt, (uint32_t)nb, o.ps_salt, ps, ctx->stream));
        }
        if (paths_out) QP_HIP(ctx, pk_gather_paths(o.digests, lde_n, plen, d_idx, 0, m, d_paths, (uint32_t)nb, o.ps_digests, ps, ctx->stream));
        got.resize(nb * ps);
        QP_TRY(ctx->read_back(got.data(), d_rows, got.size() * 8));
        for (size_t b = 0; b < nb; b++) {
            const u64 *g = got.data() + b * ps;
            if (rows_out)
                for (uint32_t q = 0; q < m; q++) {  // the leaf as the proof carries it: the columns, then the salt
                    u64 *row = rows_out + (b * n + at + q) * width;
                    std::memcpy(row, g + (size_t)q * o.ncols, (size_t)o.ncols * 8);
                    if (o.salt) std::memcpy(row + o.ncols, g + (size_t)o.ncols * m + (size_t)q * 4, 32);
                }
            if (paths_out && plen) std::memcpy(paths_out + (b * n + at) * plen * 4, g + (rows_out ? width * m : 0), (size_t)m * plen * 32);
        }
    }
    return QPGPU_OK;
}

// ---- challenger (host only) ----
void qpgpu_challenger_init(qpgpu_challenger *c) { if (c) std::memset(c, 0, sizeof *c); }
static int challenger_observe(const hasher::Config &h, qpgpu_challenger *c, const uint64_t *elements, size_t n) {
    if (!c || (!elements && n)) return QPGPU_EINVAL;
    Challenger ch(h);
    if (!challenger_to_host(c, ch)) return QPGPU_EINVAL;
    ch.observe(elements, n);
    challenger_from_host(ch, c);
    return QPGPU_OK;
}
static int challenger_get(const hasher::Config &h, qpgpu_challenger *c, uint64_t *out) {
    if (!c || !out) return QPGPU_EINVAL;
    Challenger ch(h);
    if (!challenger_to_host(c, ch)) return QPGPU_EINVAL;
    *out = ch.get();
    challenger_from_host(ch, c);
    return QPGPU_OK;
}
// under the context's hasher
int qpgpu_ctx_challenger_observe(const qpgpu_ctx *ctx, qpgpu_challenger *c, const uint64_t *elements, size_t n) {
    return ctx ? challenger_observe(ctx->hasher, c, elements, n) : QPGPU_EINVAL;
}
int qpgpu_ctx_challenger_get(const qpgpu_ctx *ctx, qpgpu_challenger *c, uint64_t *out) {
    return ctx ? challenger_get(ctx->hasher, c, out) : QPGPU_EINVAL;
}
// under the process-default hasher (first ABI; an invalid state leaves the challenger untouched and get returns 0)
void qpgpu_challenger_observe(qpgpu_challenger *c, const uint64_t *elements, size_t n) { (void)challenger_observe(hasher::process_default(), c, elements, n); }
uint64_t qpgpu_challenger_get(qpgpu_challenger *c) {
    uint64_t v = 0;
    (void)challenger_get(hasher::process_default(), c, &v);
    return v;
}

}  // extern "C"
