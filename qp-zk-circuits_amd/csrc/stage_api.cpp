// stage_api.cpp — stage-level C ABI for the two gate-dependent stages of qp-plonky2's prove(): partial products (s5,
// `all_wires_permutation_partial_products`) and the quotient (s6, `compute_quotient_polys`), for a caller that runs the stage
// flow of oracle_api.cpp (include/qpgpu.h, "stage-level entry points"). A qpgpu_stage_plan holds what the two stages need and
// what does not depend on a witness: the tables a circuit handle prepares at load, built from the pack's header and the
// caller's constants/sigmas oracle. The launch sequences are the all-in-one prover's (prover_stages.cpp), for a lockstep batch of
// up to the plan's max_batch proofs (the single-proof entries are the batch of one), reading the caller's oracles in place: no
// LDE leaves the device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include "oracle_handle.hpp"
#include "prover_stages.hpp"

using gl::u64;

struct qpgpu_stage_plan {
    qpgpu_ctx *ctx = nullptr;
    uint32_t max_batch = 1;
    CircuitPack pack;                // header only: the constants/sigmas values are not kept
    const qpgpu_oracle *cs = nullptr;   // the caller's; must outlive the plan
    StageTables tab;
    StageWork work;
    Stager stage;
    u64 *d_cs_values = nullptr;      // [num_cs_cols][n]: the oracle's polynomials on the subgroup
    u64 *d_wires_vals = nullptr;     // [max_batch][num_wires][n]: host or scattered witnesses of s5; the wire values the witness check of s6 reads
    std::vector<u64> small;          // host copy of the small tables, [max_batch][tab.small_words]
    std::vector<void *> allocs;
    std::vector<std::pair<void *, size_t>> secret_allocs;

    int alloc(u64 **p, size_t count, bool secret) {
        void *v = nullptr;
        const size_t bytes = std::max<size_t>(count * 8, 8);
        hipError_t e = ctx->track_malloc(&v, bytes, secret ? residue::STAGE_PLAN : residue::CIRCUIT_SETUP);
        if (e == hipErrorOutOfMemory) return ctx->fail(QPGPU_ENOMEM, "hipMalloc(stage plan): out of device memory");
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMalloc(stage plan)");
        allocs.push_back(v);
        if (secret) secret_allocs.push_back({v, bytes});
        *p = (u64 *)v;
        return QPGPU_OK;
    }
    // overwrite everything that held witness-derived values: workspace, the host table (challenges) and the pinned ring
    void scrub() {
        for (auto &r : secret_allocs) (void)hipMemsetAsync(r.first, 0, r.second, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (stage.h) std::memset(stage.h, 0, stage.words * 8);
        volatile u64 *s = small.data();
        for (size_t i = 0; i < small.size(); i++) s[i] = 0;
    }
};

namespace {

int refuse(qpgpu_ctx *ctx, char *err, int code, const std::string &msg) {
    if (err) std::snprintf(err, QPGPU_STAGE_ERR_CAP, "%s", msg.c_str());
    if (ctx) ctx->err = msg;
    return code;
}

// an oracle argument against the plan's header; empty, or what disagrees
std::string oracle_mismatch(const qpgpu_stage_plan *pl, const qpgpu_oracle *o, size_t ncols, bool may_blind) {
    const CircuitPack &p = pl->pack;
    // its LDE lies in its shards, not behind o.lde: refused, never read as if shard 0 were the whole
    if (o->sh) return "is sharded over " + std::to_string(o->sh->s.size()) + " contexts: sharded oracles are not taken here yet";
    if (o->ctx != pl->ctx) return "belongs to another context";
    if (o->o.ncols != ncols) return "has " + std::to_string(o->o.ncols) + " polynomials, the circuit needs " + std::to_string(ncols);
    if (o->o.log_n != p.degree_bits) return "has degree_bits " + std::to_string(o->o.log_n) + ", the circuit " + std::to_string(p.degree_bits);
    if (o->o.rate_bits != p.rate_bits) return "has rate_bits " + std::to_string(o->o.rate_bits) + ", the circuit " + std::to_string(p.rate_bits);
    if (!may_blind && o->o.salt) return "is blinded: the constants/sigmas commitment carries no salt";
    return "";
}

// a failed call leaves nothing witness-derived behind (as qpgpu_oracle_free does for its block); the message survives the scrub
int fail_scrubbed(qpgpu_stage_plan *pl, int rc) {
    const std::string keep = pl->ctx->err;
    (void)hipStreamSynchronize(pl->ctx->stream);
    pl->scrub();
    pl->ctx->err = keep;
    return rc;
}

}  // namespace

extern "C" {

void qpgpu_stage_plan_free(qpgpu_stage_plan *pl) {
    if (!pl) return;
    (void)hipSetDevice(pl->ctx->device);
    (void)hipStreamSynchronize(pl->ctx->stream);
    pl->scrub();
    pl->ctx->track_free(pl->stage.h);
    for (void *p : pl->allocs) pl->ctx->track_free(p);
    delete pl;
}

int qpgpu_stage_plan_create_batch(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, uint32_t max_batch,
                                  qpgpu_stage_plan **out, char *err) {
    if (err) err[0] = 0;
    if (!out) return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: null plan pointer");
    *out = nullptr;
    if (!words) return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: null words");
    // the header is checked first: it needs no device, and a refusal reads the same whether or not a GPU is present
    CircuitPack pack;
    {
        std::string why = pack.parse_stage(words, n_words);
        if (why.empty()) why = stage_limits(pack);
        if (!why.empty()) return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: " + why);
    }
    if (max_batch == 0 || max_batch > 1024)
        return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: max_batch is " + std::to_string(max_batch) + ", it must be 1..1024");
    pack.constants_sigmas.clear(); pack.constants_sigmas.shrink_to_fit();   // the oracle holds them
    pack.header_only = true;
    if (!ctx) return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: null context");
    if (!cs_oracle) return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: null cs_oracle");
    QP_DEV(ctx);
    qpgpu_stage_plan *pl = new qpgpu_stage_plan();
    pl->ctx = ctx; pl->max_batch = max_batch; pl->pack = pack; pl->cs = cs_oracle;
    const CircuitPack &p = pl->pack;
    {
        std::string why = oracle_mismatch(pl, cs_oracle, p.num_cs_cols(), false);
        if (why.empty() && cs_oracle->o.nb != 1)
            why = "holds a batch of " + std::to_string(cs_oracle->o.nb) + " proofs: the constants/sigmas commitment is shared by all proofs";
        if (!why.empty()) { delete pl; return refuse(ctx, err, QPGPU_EINVAL, "stage_plan_create: cs_oracle " + why); }
    }
    const u64 n = p.n();
    const unsigned d = (unsigned)p.degree_bits;
    int rc = QPGPU_OK;
    auto fail = [&](int code) {
        const std::string keep = ctx->err;
        qpgpu_stage_plan_free(pl);
        return refuse(ctx, err, code, keep);
    };
#define CK(expr) do { rc = (expr); if (rc) return fail(rc); } while (0)
    const StageAlloc take = [pl](u64 **ptr, size_t count, bool secret) { return pl->alloc(ptr, count, secret); };
    // the constants/sigmas polynomials on the subgroup (the sigma columns of s5, the witness check's constants): forward NTT of
    // the oracle's coefficients
    CK(pl->alloc(&pl->d_cs_values, (size_t)p.num_cs_cols() * n, false));
    CK(ntt_run(ctx, cs_oracle->o.coeffs, pl->d_cs_values, d, d, (size_t)p.num_cs_cols(), false, false, 0));
    pl->tab.cs_values = pl->d_cs_values; pl->tab.cs_lde = cs_oracle->o.lde;
    CK(stage_tables_build(ctx, p, take, pl->tab));
    pl->work.stage = &pl->stage;
    CK(stage_work_alloc(p, pl->tab, take, max_batch, pl->work));
    CK(pl->alloc(&pl->d_wires_vals, (size_t)max_batch * p.num_wires * n, true));
    pl->small.assign((size_t)max_batch * pl->tab.small_words, 0);
    {
        pl->stage.words = 2 * stage_ring_words(pl->tab, max_batch) + 64;    // s6 puts the beta part again, then the alpha part and the check's seed
        void *hp = nullptr;
        const hipError_t e = ctx->track_host_malloc(&hp, pl->stage.words * 8, residue::STAGE_PLAN);
        if (e != hipSuccess) return fail(ctx->hip_fail(e, "hipHostMalloc(stage plan)"));
        pl->stage.h = (u64 *)hp;
    }
    CK(ctx->reserve_read_back((1u << 12) + (size_t)max_batch * 16));
    {   // asynchronous faults of the setup kernels surface here
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx->hip_fail(e, "stage_plan_create: hipStreamSynchronize"));
    }
#undef CK
    *out = pl;
    return QPGPU_OK;
}

int qpgpu_stage_plan_create(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, qpgpu_stage_plan **out, char *err) {
    return qpgpu_stage_plan_create_batch(ctx, words, n_words, cs_oracle, 1, out, err);
}

uint32_t qpgpu_stage_plan_max_batch(const qpgpu_stage_plan *pl) { return pl ? pl->max_batch : 0; }

int qpgpu_stage_plan_info(const qpgpu_stage_plan *pl, unsigned *degree_bits, unsigned *num_challenges, unsigned *num_partial_products,
                          unsigned *quotient_degree_factor, int *fused_selected) {
    if (!pl) return QPGPU_EINVAL;
    const CircuitPack &p = pl->pack;
    if (degree_bits) *degree_bits = (unsigned)p.degree_bits;
    if (num_challenges) *num_challenges = (unsigned)p.num_challenges;
    if (num_partial_products) *num_partial_products = (unsigned)p.num_partial_products;
    if (quotient_degree_factor) *quotient_degree_factor = (unsigned)p.quotient_degree_factor;
    if (fused_selected) *fused_selected = pl->tab.fused_selected(p) ? 1 : 0;
    return QPGPU_OK;
}

}  // extern "C"

namespace {

// s5 for a lockstep batch; `who` is the entry's name in messages. wires: nb matrices, on the host or on the device.
int partial_products_impl(qpgpu_stage_plan *pl, const char *who, const uint64_t *const *wires, uint32_t nb, int wires_on_device,
                          const uint64_t *betas, const uint64_t *gammas, uint64_t *d_out) {
    qpgpu_ctx *ctx = pl->ctx;
    const CircuitPack &p = pl->pack;
    const u64 n = p.n();
    const size_t mat = (size_t)p.num_wires * n, nch = p.num_challenges, SW = pl->tab.small_words;
    for (uint32_t b = 0; b < nb; b++) {
        u64 ch[8];
        for (size_t k = 0; k < nch; k++) { ch[k] = gl::canon(betas[b * nch + k]); ch[4 + k] = gl::canon(gammas[b * nch + k]); }
        stage_fill_betas(p, pl->small.data() + b * SW, ch, ch + 4);
    }
    pl->stage.pos = 0;
    bool dense = true;
    for (uint32_t b = 0; b < nb; b++) dense = dense && wires[b] == wires[0] + b * mat;
    const u64 *d_wires = wires[0];
    int rc = QPGPU_OK;
    if (!wires_on_device) {
        if (dense) rc = h2d_sync(ctx, pl->d_wires_vals, wires[0], nb * mat * 8);
        else for (uint32_t b = 0; b < nb && rc == QPGPU_OK; b++) rc = h2d_sync(ctx, pl->d_wires_vals + b * mat, wires[b], mat * 8);
        d_wires = pl->d_wires_vals;
    } else if (!dense) {   // witnesses scattered over the heap: gathered into the plan's wire area, as qpgpu_prove_batch_dev does
        for (uint32_t b = 0; b < nb && rc == QPGPU_OK; b++) {
            const hipError_t e = hipMemcpyAsync(pl->d_wires_vals + b * mat, wires[b], mat * 8, hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) rc = ctx->hip_fail(e, "stage_partial_products: gather");
        }
        d_wires = pl->d_wires_vals;
    }
    if (rc == QPGPU_OK) rc = stage_partial_products(ctx, p, pl->tab, pl->work, nb, pl->small.data(), d_wires, mat, d_out);
    if (rc == QPGPU_OK) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = ctx->hip_fail(e, (std::string(who) + ": hipStreamSynchronize").c_str());
    }
    return rc == QPGPU_OK ? rc : fail_scrubbed(pl, rc);
}

// s6 for a lockstep batch. The oracles hold nb proofs each (checked by the caller of this function for the batch entry).
int quotient_impl(qpgpu_stage_plan *pl, const char *who, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, uint32_t nb,
                  const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hashes, uint64_t *d_out) {
    qpgpu_ctx *ctx = pl->ctx;
    const CircuitPack &p = pl->pack;
    {
        std::string why = oracle_mismatch(pl, wires_oracle, p.num_wires, true);
        if (!why.empty()) return ctx->fail(QPGPU_EINVAL, std::string(who) + ": wires_oracle " + why);
        why = oracle_mismatch(pl, zs_pp_oracle, p.num_zs_pp_cols(), true);
        if (!why.empty()) return ctx->fail(QPGPU_EINVAL, std::string(who) + ": zs_pp_oracle " + why);
    }
    const u64 n = p.n();
    const unsigned d = (unsigned)p.degree_bits;
    const uint32_t nch = (uint32_t)p.num_challenges;
    const size_t SW = pl->tab.small_words;
    for (uint32_t b = 0; b < nb; b++) {
        u64 ch[12], pih[4];
        for (uint32_t k = 0; k < nch; k++) {
            ch[k] = gl::canon(betas[(size_t)b * nch + k]); ch[4 + k] = gl::canon(gammas[(size_t)b * nch + k]); ch[8 + k] = gl::canon(alphas[(size_t)b * nch + k]);
        }
        for (int i = 0; i < 4; i++) pih[i] = gl::canon(public_inputs_hashes[4 * (size_t)b + i]);
        stage_fill_betas(p, pl->small.data() + b * SW, ch, ch + 4);
        stage_fill_alphas(p, pl->small.data() + b * SW, ch + 8, pih);
    }
    pl->stage.pos = 0;
    auto run = [&]() -> int {
        QP_TRY(stage_put_betas(ctx, p, pl->tab, pl->work, nb, pl->small.data()));
        // The witness check of qpgpu_prove* (qpgpu_circuit_set_witness_check), always on here: the stage flow has no later point at
        // which an unsatisfied witness would show, the quotient of one is simply not a polynomial of the committed degree. It reads the
        // trace on the subgroup: wire and Z values from the oracles' coefficients (dense [nb][cols][n]: one transform over all the
        // proofs' wire columns; the Z columns are the first nch of each proof's Z/partial-products block), the row products of the
        // permutation argument from those wire values.
        QP_TRY(ntt_run(ctx, wires_oracle->o.coeffs, pl->d_wires_vals, d, d, (size_t)nb * p.num_wires, false, false, 0));
        QP_TRY(stage_pp_rows(ctx, p, pl->tab, pl->work, nb, pl->d_wires_vals, p.num_wires * n));
        NttProofs np; np.nproofs = nb; np.in_ps = zs_pp_oracle->o.ps_coeffs; np.out_ps = (u64)nch * n;
        QP_TRY(ntt_run(ctx, zs_pp_oracle->o.coeffs, pl->work.d_z, d, d, (size_t)nch, false, false, 0, np));
        // the oracles' LDE columns are the polynomial columns only, stride lde_n: the salt columns of a blinded oracle lie in a
        // region of their own behind the digests and are never touched
        QuotientViews v;
        v.wires_lde = wires_oracle->o.lde; v.ps_wires_lde = wires_oracle->o.ps_lde;
        v.zs_lde = zs_pp_oracle->o.lde; v.ps_zs_lde = zs_pp_oracle->o.ps_lde; v.out = d_out;
        v.check_wires = pl->d_wires_vals; v.ps_check_wires = p.num_wires * n;
        QP_TRY(stage_quotient(ctx, p, pl->tab, pl->work, nb, pl->small.data(), v));
        QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return QPGPU_OK;
    };
    const int rc = run();
    return rc == QPGPU_OK ? rc : fail_scrubbed(pl, rc);
}

}  // namespace

extern "C" {

int qpgpu_stage_partial_products(qpgpu_stage_plan *pl, const uint64_t *wires, int wires_on_device, const uint64_t *betas, const uint64_t *gammas,
                                 uint64_t *d_out) {
    if (!pl) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = pl->ctx;
    QP_DEV(ctx);
    if (!wires || !betas || !gammas || !d_out) return ctx->fail(QPGPU_EINVAL, "stage_partial_products: null argument");
    return partial_products_impl(pl, "stage_partial_products", &wires, 1, wires_on_device, betas, gammas, d_out);
}

int qpgpu_stage_partial_products_batch(qpgpu_stage_plan *pl, const uint64_t *const *wires, uint32_t batch, int wires_on_device,
                                       const uint64_t *betas, const uint64_t *gammas, uint64_t *d_out) {
    if (!pl) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = pl->ctx;
    QP_DEV(ctx);
    if (!wires || !betas || !gammas || !d_out) return ctx->fail(QPGPU_EINVAL, "stage_partial_products_batch: null argument");
    if (batch == 0 || batch > pl->max_batch)
        return ctx->fail(QPGPU_EINVAL, "stage_partial_products_batch: batch is " + std::to_string(batch) + ", the plan's max_batch is " + std::to_string(pl->max_batch));
    for (uint32_t b = 0; b < batch; b++)
        if (!wires[b]) return ctx->fail(QPGPU_EINVAL, "stage_partial_products_batch: wires[" + std::to_string(b) + "] is NULL");
    return partial_products_impl(pl, "stage_partial_products_batch", wires, batch, wires_on_device, betas, gammas, d_out);
}

int qpgpu_stage_quotient(qpgpu_stage_plan *pl, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, const uint64_t *betas,
                         const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hash, uint64_t *d_out) {
    if (!pl) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = pl->ctx;
    QP_DEV(ctx);
    if (!wires_oracle || !zs_pp_oracle || !betas || !gammas || !alphas || !public_inputs_hash || !d_out)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient: null argument");
    if (wires_oracle->o.nb != 1) return ctx->fail(QPGPU_EINVAL, "stage_quotient: wires_oracle holds a batch of " + std::to_string(wires_oracle->o.nb) + " proofs, use qpgpu_stage_quotient_batch");
    if (zs_pp_oracle->o.nb != 1) return ctx->fail(QPGPU_EINVAL, "stage_quotient: zs_pp_oracle holds a batch of " + std::to_string(zs_pp_oracle->o.nb) + " proofs, use qpgpu_stage_quotient_batch");
    return quotient_impl(pl, "stage_quotient", wires_oracle, zs_pp_oracle, 1, betas, gammas, alphas, public_inputs_hash, d_out);
}

int qpgpu_stage_quotient_batch(qpgpu_stage_plan *pl, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, uint32_t batch,
                               const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hashes,
                               uint64_t *d_out) {
    if (!pl) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = pl->ctx;
    QP_DEV(ctx);
    if (!wires_oracle || !zs_pp_oracle || !betas || !gammas || !alphas || !public_inputs_hashes || !d_out)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: null argument");
    if (batch == 0 || batch > pl->max_batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: batch is " + std::to_string(batch) + ", the plan's max_batch is " + std::to_string(pl->max_batch));
    if (wires_oracle->o.nb != batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: wires_oracle holds " + std::to_string(wires_oracle->o.nb) + " proofs, the call is for a batch of " + std::to_string(batch));
    if (zs_pp_oracle->o.nb != batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: zs_pp_oracle holds " + std::to_string(zs_pp_oracle->o.nb) + " proofs, the call is for a batch of " + std::to_string(batch));
    return quotient_impl(pl, "stage_quotient_batch", wires_oracle, zs_pp_oracle, batch, betas, gammas, alphas, public_inputs_hashes, d_out);
}

}  // extern "C"
