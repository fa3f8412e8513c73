// oracle_sharded.cpp — one polynomial commitment across several contexts (include/qpgpu.h: qpgpu_oracle_commit_sharded). The cut is
// by cosets (oracle_shard_map.hpp): shard g of G owns the leaves [g N/G, (g + 1) N/G), which are whole cosets and a whole subtree, and
// its values are the LDE of the same coefficients at rate 2^r / G on the shift g_mult w_(d+r)^brev(g). So a shard needs the
// coefficients once (1/2^r of the LDE) and then transforms, salts, hashes and reduces its leaves with the launches every oracle uses,
// at its own size, without talking to anyone; what comes back is max(1, 2^cap_h / G) digests. The home context (ctxs[0], which is
// also shard 0's) keeps the coefficients for qpgpu_oracle_eval and the FRI arithmetic and hashes the levels above the shards' roots
// when G > 2^cap_h. The calling thread drives every context's stream and has synchronised them all when an entry returns.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "merkle.hpp"
#include "oracle_handle.hpp"
#include "prover_kernels.hpp"

using gl::u64;

namespace {
bool same_hasher(const qpgpu_ctx *a, const qpgpu_ctx *b) {
    if (a->hasher.kind != b->hasher.kind) return false;
    return a->hasher.kind != hasher::POSEIDON2 || std::memcmp(&a->hasher.p2, &b->hasher.p2, sizeof(poseidon2::Params)) == 0;
}

// everything after the handle exists; a failure leaves the handle to the caller to free (every stream is synchronised there)
int commit_shards(qpgpu_oracle *h, const uint64_t *polys, unsigned flags, uint64_t blinding_seed, hipEvent_t ready) {
    qpgpu_ctx *home = h->ctx;
    OracleShards &sh = *h->sh;
    PolyOracle &o = h->o;
    const shard_map::Map &m = sh.map;
    const uint32_t G = m.shards();
    const bool from_coeffs = (flags & QPGPU_ORACLE_COEFFS) != 0;
    const u64 n = 1ull << m.d, Nl = m.local_leaves();
    const size_t w_coeffs = (size_t)o.ncols * n;

    if (sh.blinded) {
        // one key for the whole oracle: every shard draws its leaves' salts from the same stream, at the global leaf index
        uint32_t key[8];
        int rc = QPGPU_OK;
        if (blinding_seed) salt_key_from_seed(blinding_seed, key);
        else if (salt_key_random(key) != QPGPU_OK) rc = home->fail(QPGPU_EDEVICE, "oracle_commit_sharded: the OS entropy source failed");
        for (uint32_t g = 0; g < G && rc == QPGPU_OK; g++) {
            qpgpu_ctx *c = sh.s[g].ctx;
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipMemcpyAsync(sh.s[g].d_key, key, sizeof key, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = shard_fail(home, g, c, c->hip_fail(e, "oracle_commit_sharded: key upload"));
        }
        volatile uint32_t *kz = key;                  // the key is a secret: the host copy goes as soon as the devices have it
        for (int i = 0; i < 8; i++) kz[i] = 0;
        QP_TRY(rc);
    }

    // ---- home: the coefficients ----
    QP_DEV(home);
    const u64 *src = polys;
    if (!(flags & QPGPU_ORACLE_DEVICE_INPUT)) {
        // values are staged through shard 0's LDE area (N/G >= n words per column, overwritten afterwards)
        u64 *dst = from_coeffs ? o.coeffs : sh.s[0].lde;
        QP_HIP(home, hipMemcpyAsync(dst, polys, w_coeffs * 8, hipMemcpyHostToDevice, home->stream));
        QP_HIP(home, hipStreamSynchronize(home->stream));
        src = dst;
    } else if (from_coeffs) {
        QP_HIP(home, hipMemcpyAsync(o.coeffs, polys, w_coeffs * 8, hipMemcpyDeviceToDevice, home->stream));
    }
    if (!from_coeffs) QP_TRY(ntt_run(home, src, o.coeffs, m.d, m.d, o.ncols, true, false, 0));
    QP_HIP(home, hipEventRecord(ready, home->stream));

    // ---- every shard: its copy of the coefficients, then LDE, salts, leaves and subtree on its own stream ----
    const u64 wL = gl::root_of_unity(m.log_leaves());
    for (uint32_t g = 0; g < G; g++) {
        OracleShard &s = sh.s[g];
        qpgpu_ctx *c = s.ctx;
        QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
        if (g > 0) {
            QP_SHARD_HIP(home, g, c, hipStreamWaitEvent(c->stream, ready, 0));
            if (c->device == home->device) QP_SHARD_HIP(home, g, c, hipMemcpyAsync(s.coeffs, o.coeffs, w_coeffs * 8, hipMemcpyDeviceToDevice, c->stream));
            else QP_SHARD_HIP(home, g, c, hipMemcpyPeerAsync(s.coeffs, c->device, o.coeffs, home->device, w_coeffs * 8, c->stream));
        }
        c->hasher_in_use = true;
        QP_SHARD(home, g, c, merkle_ensure_constants(c));
        const u64 shift = gl::mul(gl::MULT_GEN, gl::pow(wL, m.shift_exponent(g)));
        QP_SHARD(home, g, c, ntt_run(c, s.coeffs, s.lde, m.d, m.local_log_leaves(), o.ncols, false, true, shift));
        MerkleLeafArgs a{};
        a.src0 = s.lde; a.stride0 = Nl; a.ncols0 = o.ncols; a.n_leaves = Nl; a.digests = s.digests; a.batch = 1;
        if (sh.blinded) {
            QP_SHARD_HIP(home, g, c, pk_salt_slice(s.d_key, o.oracle_index, m.first_leaf(g), Nl, s.salt, c->stream));
            a.src1 = s.salt; a.stride1 = Nl; a.ncols1 = 4;
        }
        QP_SHARD(home, g, c, merkle_build(c, a, m.local_log_leaves(), m.local_cap_h(), s.digests));
    }

    // ---- the shards' roots: cap entries as they are, or the leaves of the home context's merge levels ----
    const size_t total_l = digest_words(m.local_log_leaves(), m.local_cap_h()), rw = (size_t)4 << m.local_cap_h();
    std::vector<u64> roots(rw * G);
    for (uint32_t g = 0; g < G; g++) {
        qpgpu_ctx *c = sh.s[g].ctx;
        QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
        QP_SHARD(home, g, c, c->read_back(roots.data() + rw * g, sh.s[g].digests + total_l - rw, rw * 8));   // synchronises the shard's stream
    }
    QP_DEV(home);
    if (m.merge_levels() == 0) { o.cap = roots; return QPGPU_OK; }
    u64 *d_merge = o.coeffs + w_coeffs;
    const size_t mw = (size_t)m.merge_digests() * 4;
    QP_HIP(home, hipMemcpyAsync(d_merge, roots.data(), roots.size() * 8, hipMemcpyHostToDevice, home->stream));
    QP_HIP(home, hipStreamSynchronize(home->stream));
    home->prof_begin("merkle_nodes");
    hipError_t e = merkle_reduce_to_cap(d_merge, G, 1ull << m.cap_h, 1, 0, home->hasher_dev(), home->stream);
    home->prof_end();
    QP_HIP(home, e);
    sh.merge.resize(mw);
    QP_TRY(home->read_back(sh.merge.data(), d_merge, mw * 8));
    o.cap.assign(sh.merge.end() - o.cap_words(), sh.merge.end());
    return QPGPU_OK;
}
}  // namespace

int refuse_sharded(const qpgpu_oracle *h, const char *entry) {
    return h->ctx->fail(QPGPU_EINVAL, std::string(entry) + ": sharded oracles are not taken here yet (the oracle has " + std::to_string(h->sh->s.size()) +
                                          " shards; commit it with qpgpu_oracle_commit for this entry)");
}

void oracle_sharded_free(qpgpu_oracle *h) {
    // committed columns can hold the witness: every shard is scrubbed on the context that owns it before release
    for (OracleShard &s : h->sh->s) {
        if (!s.block) continue;
        (void)hipSetDevice(s.ctx->device);
        (void)hipMemsetAsync(s.block, 0, s.block_words * 8, s.ctx->stream);
        (void)hipStreamSynchronize(s.ctx->stream);
        s.ctx->track_free(s.block);
    }
    (void)hipSetDevice(h->ctx->device);
    if (h->block) {
        (void)hipMemsetAsync(h->block, 0, h->block_words * 8, h->ctx->stream);
        (void)hipStreamSynchronize(h->ctx->stream);
        h->ctx->track_free(h->block);
    }
    std::fill(h->sh->merge.begin(), h->sh->merge.end(), 0);
    delete h;
}

// columns [first, first + count) of the LDE: the shards' blocks side by side in leaf order
int oracle_sharded_read_lde(qpgpu_oracle *h, uint32_t first, uint32_t count, uint64_t *out) {
    qpgpu_ctx *home = h->ctx;
    const OracleShards &sh = *h->sh;
    const u64 N = h->o.lde_n(), Nl = sh.map.local_leaves();
    for (uint32_t g = 0; g < sh.s.size(); g++) {
        qpgpu_ctx *c = sh.s[g].ctx;
        QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
        QP_SHARD_HIP(home, g, c, hipMemcpy2DAsync(out + g * Nl, N * 8, sh.s[g].lde + (size_t)first * Nl, Nl * 8, Nl * 8, count, hipMemcpyDeviceToHost, c->stream));
    }
    for (uint32_t g = 0; g < sh.s.size(); g++) {
        qpgpu_ctx *c = sh.s[g].ctx;
        QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
        QP_SHARD_HIP(home, g, c, hipStreamSynchronize(c->stream));
    }
    QP_DEV(home);
    return QPGPU_OK;
}

int oracle_sharded_open(const PolyOracle &o, const u64 *indices, size_t n, u64 *rows_out, u64 *paths_out) {
    const OracleShards &sh = *o.sh;
    qpgpu_ctx *home = sh.home;
    const shard_map::Map &m = sh.map;
    const uint32_t G = m.shards(), pl = m.local_path_len(), ml = m.merge_levels(), plen = m.path_len();
    const u64 Nl = m.local_leaves();
    const size_t width = (size_t)o.ncols + (sh.blinded ? 4 : 0), pw = (size_t)pl * 4;
    const size_t per = (rows_out ? width : 0) + (paths_out ? pw : 0);     // gathered words per index on a shard
    if (n == 0 || (!rows_out && !paths_out)) return QPGPU_OK;
    const size_t chunk = 256;                         // indices per pass: the gathers go through the shards' scratch buffers
    std::vector<std::vector<u64>> local(G);           // a shard's local indices of this pass, and where each goes in the caller's order
    std::vector<std::vector<size_t>> where(G);
    std::vector<u64> got;
    for (size_t at = 0; at < n; at += chunk) {
        const size_t cnt = std::min(chunk, n - at);
        for (uint32_t g = 0; g < G; g++) { local[g].clear(); where[g].clear(); }
        for (size_t i = at; i < at + cnt; i++) {
            const uint32_t g = m.shard_of(indices[i]);
            local[g].push_back(m.local_of(indices[i]));
            where[g].push_back(i);
        }
        // one gather per shard on that shard's stream, all of them queued before the first is waited for
        for (uint32_t g = 0; g < G && per; g++) {
            const uint32_t mg = (uint32_t)local[g].size();
            if (!mg) continue;
            const OracleShard &s = sh.s[g];
            qpgpu_ctx *c = s.ctx;
            QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
            QP_SHARD(home, g, c, c->ensure_scratch((size_t)mg * (1 + per) * 8));
            u64 *d_idx = c->scratch, *d_rows = d_idx + mg, *d_salt = d_rows + (rows_out ? (size_t)o.ncols * mg : 0),
                *d_paths = d_rows + (rows_out ? width * mg : 0);
            QP_SHARD_HIP(home, g, c, hipMemcpyAsync(d_idx, local[g].data(), (size_t)mg * 8, hipMemcpyHostToDevice, c->stream));
            if (rows_out) {
                QP_SHARD_HIP(home, g, c, pk_gather_rows(s.lde, Nl, o.ncols, d_idx, mg, d_rows, 1, 0, 0, c->stream));
                if (sh.blinded) QP_SHARD_HIP(home, g, c, pk_gather_rows(s.salt, Nl, 4, d_idx, mg, d_salt, 1, 0, 0, c->stream));
            }
            if (paths_out) QP_SHARD_HIP(home, g, c, pk_gather_paths(s.digests, Nl, pl, d_idx, 0, mg, d_paths, 1, 0, 0, c->stream));
        }
        for (uint32_t g = 0; g < G; g++) {
            const uint32_t mg = (uint32_t)local[g].size();
            if (!mg) continue;
            qpgpu_ctx *c = sh.s[g].ctx;
            got.resize((size_t)mg * per);
            if (per) {
                QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
                QP_SHARD(home, g, c, c->read_back(got.data(), c->scratch + mg, got.size() * 8));
            }
            const u64 *g_rows = got.data(), *g_salt = g_rows + (size_t)o.ncols * mg, *g_paths = got.data() + (rows_out ? width * mg : 0);
            for (uint32_t q = 0; q < mg; q++) {
                const size_t i = where[g][q];
                if (rows_out) {                       // the leaf as the proof carries it: the columns, then the salt
                    std::memcpy(rows_out + i * width, g_rows + (size_t)q * o.ncols, (size_t)o.ncols * 8);
                    if (sh.blinded) std::memcpy(rows_out + i * width + o.ncols, g_salt + (size_t)q * 4, 32);
                }
                if (paths_out) {
                    u64 *path = paths_out + i * plen * 4;
                    if (pw) std::memcpy(path, g_paths + (size_t)q * pw, pw * 8);
                    for (unsigned t = 0; t < ml; t++)     // above the shard's root: the home context's merge levels
                        std::memcpy(path + pw + 4 * t, sh.merge.data() + 4 * (m.merge_level_offset(t) + m.merge_sibling(g, t)), 32);
                }
            }
        }
    }
    QP_DEV(home);
    return QPGPU_OK;
}

extern "C" {

int qpgpu_oracle_commit_sharded(qpgpu_ctx *const *ctxs, uint32_t n_ctx, const uint64_t *polys, uint32_t num_polys, unsigned degree_bits,
                                unsigned rate_bits, unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream,
                                qpgpu_oracle **out) {
    if (!ctxs || !out || n_ctx == 0) return QPGPU_EINVAL;
    for (uint32_t i = 0; i < n_ctx; i++) if (!ctxs[i]) return QPGPU_EINVAL;
    qpgpu_ctx *home = ctxs[0];
    QP_DEV(home);
    *out = nullptr;
    if (!polys || num_polys == 0) return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: no polynomials");
    if (n_ctx == 1) return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: one context is no sharded oracle, use qpgpu_oracle_commit");
    if (degree_bits + rate_bits > 23 || degree_bits < 1) return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: LDE sizes up to 2^23 supported");
    if (cap_height > degree_bits + rate_bits) return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: cap_height exceeds the tree height");
    if (flags & ~7u) return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: unknown flags");
    const int lg = shard_map::log2_shards(n_ctx, rate_bits);
    if (lg < 0)
        return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: n_ctx = " + std::to_string(n_ctx) + " is not a power of two from 2 to 2^rate_bits = " + std::to_string(1ull << rate_bits));
    for (uint32_t i = 0; i < n_ctx; i++) {
        for (uint32_t j = 0; j < i; j++)
            if (ctxs[i] == ctxs[j])
                return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: ctxs[" + std::to_string(j) + "] and ctxs[" + std::to_string(i) + "] are the same context; every shard runs on a context of its own");
        if (!same_hasher(home, ctxs[i]))
            return home->fail(QPGPU_EINVAL, "oracle_commit_sharded: ctxs[" + std::to_string(i) + "] has another hasher than ctxs[0]");
    }
    home->hasher_in_use = true;
    QP_TRY(merkle_ensure_constants(home));

    qpgpu_oracle *h = new qpgpu_oracle();
    h->ctx = home;
    h->sh.reset(new OracleShards());
    OracleShards &sh = *h->sh;
    sh.home = home;
    sh.map.d = degree_bits; sh.map.r = rate_bits; sh.map.cap_h = cap_height; sh.map.lg = (unsigned)lg;
    sh.blinded = (flags & QPGPU_ORACLE_BLINDING) != 0;
    sh.s.resize(n_ctx);
    PolyOracle &o = h->o;
    o.ncols = num_polys; o.log_n = degree_bits; o.rate_bits = rate_bits; o.cap_h = cap_height; o.oracle_index = blinding_stream;
    o.sh = &sh; o.blinded = sh.blinded;
    o.set_batch(1, true);
    const shard_map::Map &m = sh.map;
    const u64 n = 1ull << degree_bits, Nl = m.local_leaves();
    const size_t w_coeffs = (size_t)num_polys * n, w_merge = (size_t)m.merge_digests() * 4, w_eval = 2 + 2 * (size_t)num_polys;
    const size_t w_lde = (size_t)num_polys * Nl, w_dig = digest_words(m.local_log_leaves(), m.local_cap_h()), w_salt = sh.blinded ? (size_t)4 * Nl : 0;
    int rc = QPGPU_OK;
    {
        h->block_words = w_coeffs + w_merge + w_eval;
        void *v = nullptr;
        hipError_t e = home->track_malloc(&v, h->block_words * 8, residue::ORACLE);
        if (e != hipSuccess) rc = home->hip_fail(e, "hipMalloc(oracle)");
        h->block = (u64 *)v;
        o.coeffs = h->block;
        h->d_point = (gl::e2 *)(h->block + w_coeffs + w_merge); h->d_eval = h->d_point + 1;
    }
    for (uint32_t g = 0; g < n_ctx && rc == QPGPU_OK; g++) {
        OracleShard &s = sh.s[g];
        s.ctx = ctxs[g];
        hipError_t e = hipSetDevice(s.ctx->device);
        const size_t w_copy = g ? w_coeffs : 0;
        s.block_words = w_copy + w_lde + w_dig + w_salt + 4;
        void *v = nullptr;
        if (e == hipSuccess) e = s.ctx->track_malloc(&v, s.block_words * 8, residue::ORACLE);
        if (e != hipSuccess) { rc = shard_fail(home, g, s.ctx, s.ctx->hip_fail(e, "hipMalloc(oracle shard)")); break; }
        s.block = (u64 *)v;
        s.coeffs = g ? s.block : o.coeffs;
        s.lde = s.block + w_copy; s.digests = s.lde + w_lde;
        s.salt = sh.blinded ? s.digests + w_dig : nullptr;
        s.d_key = (uint32_t *)(s.digests + w_dig + w_salt);
    }
    hipEvent_t ready = nullptr;
    if (rc == QPGPU_OK) {
        hipError_t e = hipSetDevice(home->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
        if (e != hipSuccess) rc = home->hip_fail(e, "hipEventCreate");
    }
    if (rc == QPGPU_OK) rc = commit_shards(h, polys, flags, blinding_seed, ready);
    if (rc != QPGPU_OK) {
        const std::string why = home->err;
        oracle_sharded_free(h);                       // waits for every stream, so nothing still waits on the event
        if (ready) (void)hipEventDestroy(ready);
        home->err = why;
        return rc;
    }
    (void)hipSetDevice(home->device);
    (void)hipEventDestroy(ready);
    *out = h;
    return QPGPU_OK;
}

uint32_t qpgpu_oracle_shards(const qpgpu_oracle *h) { return h ? (h->sh ? (uint32_t)h->sh->s.size() : 1) : 0; }

int qpgpu_oracle_shard_range(const qpgpu_oracle *h, uint32_t shard, uint64_t *first_leaf, uint64_t *num_leaves) {
    if (!h || shard >= qpgpu_oracle_shards(h)) return QPGPU_EINVAL;
    if (first_leaf) *first_leaf = h->sh ? h->sh->map.first_leaf(shard) : 0;
    if (num_leaves) *num_leaves = h->sh ? h->sh->map.local_leaves() : h->o.lde_n();
    return QPGPU_OK;
}

int qpgpu_oracle_shard_device_ptrs(const qpgpu_oracle *h, uint32_t shard, const uint64_t **d_lde, const uint64_t **d_digests) {
    if (!h || shard >= qpgpu_oracle_shards(h)) return QPGPU_EINVAL;
    if (d_lde) *d_lde = h->sh ? h->sh->s[shard].lde : h->o.lde;
    if (d_digests) *d_digests = h->sh ? h->sh->s[shard].digests : h->o.digests;
    return QPGPU_OK;
}

}  // extern "C"
