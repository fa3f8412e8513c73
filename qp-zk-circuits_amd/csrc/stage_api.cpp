// stage_api.cpp — stage-level C ABI for the two gate-dependent stages of qp-plonky2's prove(): partial products (s5,
// `all_wires_permutation_partial_products`) and the quotient (s6, `compute_quotient_polys`), for a caller that runs the stage
// flow of oracle_api.cpp (include/qpgpu.h, "stage-level entry points"). A qpgpu_stage_plan holds what the two stages need and
// what does not depend on a witness: the tables a circuit handle prepares at load, built from the pack's header and the
// caller's constants/sigmas oracle. The launch sequences are the all-in-one prover's (prover_stages.cpp), for a lockstep batch of
// up to the plan's max_batch proofs (the single-proof entries are the batch of one), reading the caller's oracles in place: no
// LDE leaves the device.
//
// A plan is a list of per-context parts (StagePart), one per context that evaluates quotient points (quotient_shard_map.hpp). A
// plan on one context has one: the home part, whose LDE is the circuit's own. A plan over a coset-sharded constants/sigmas oracle
// (qpgpu_stage_plan_create_sharded) has one per working shard: a shard's leaves are a whole LDE of their own, so part g runs the same
// launch sequence on its own context, over tables built for its shift and rate, and the home context turns the parts' coefficients
// into the chunks (pk_quotient_merge). s5 and the witness check stay on the home part, which keeps the coefficients. The calling
// thread drives every stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include "oracle_handle.hpp"
#include "prover_stages.hpp"

using gl::u64;

// the device allocations of a plan on one context, and which of them hold witness-derived values
struct StageMem {
    qpgpu_ctx *ctx = nullptr;
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
    // the context's device is selected; the stream is synchronised on return
    void scrub(Stager &stage) {
        for (auto &r : secret_allocs) (void)hipMemsetAsync(r.first, 0, r.second, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (stage.h) std::memset(stage.h, 0, stage.words * 8);
    }
    void release(Stager &stage) {
        ctx->track_free(stage.h);
        stage.h = nullptr;
        for (void *p : allocs) ctx->track_free(p);
        allocs.clear(); secret_allocs.clear();
    }
};

// What a plan keeps on one context: the tables of that context's LDE, the workspace of the kernels and the pinned staging of its
// copy of the small table. Part 0 is the home context's and serves s5, the witness check and shard 0 of s6; part g >= 1 is working
// shard g's, with the workspace of the quotient kernels alone.
struct StagePart {
    StageMem mem;
    StageTables tab;
    StageWork work;
    Stager stage;
    u64 *d_vals = nullptr;           // g >= 1: [nch][M] on another device than the home context's; on the same one the part writes its gather block in place
    hipEvent_t done = nullptr;       // g >= 1: recorded on the part's stream behind its block of the gather buffer
};

struct qpgpu_stage_plan {
    qpgpu_ctx *ctx = nullptr;
    uint32_t max_batch = 1;
    CircuitPack pack;                // header only: the constants/sigmas values are not kept
    const qpgpu_oracle *cs = nullptr;   // the caller's; must outlive the plan
    std::vector<std::unique_ptr<StagePart>> parts;   // qmap.working() of them once the plan stands; a plan on one context has the home part alone
    u64 *d_cs_values = nullptr;      // [num_cs_cols][n]: the oracle's polynomials on the subgroup
    u64 *d_wires_vals = nullptr;     // [max_batch][num_wires][n]: host or scattered witnesses of s5; the wire values the witness check of s6 reads
    std::vector<u64> small;          // host copy of the small tables, [max_batch][small_words]
    // the contexts of cs's shards in order (empty: a plan on one context), the arithmetic of who evaluates what (lg = 0 on one
    // context), and on the home context the gather buffer [Gq][nch][M] and the merge kernel's table, both only where Gq > 1
    std::vector<qpgpu_ctx *> shard_ctxs;
    shard_map::QuotientMap qmap;
    u64 *d_gather = nullptr, *d_merge_tab = nullptr;

    bool sharded() const { return !shard_ctxs.empty(); }
    StagePart &home() const { return *parts[0]; }
    // f on every part with its context's device selected: the other contexts' first, the home context's last, whose device stays selected
    template <class F> void each_part(F f) {
        for (size_t i = 1; i <= parts.size(); i++) {
            StagePart &s = *parts[i % parts.size()];
            (void)hipSetDevice(s.mem.ctx->device);
            f(s);
        }
    }
    // wait for every stream of the plan, then overwrite everything that held witness-derived values: the workspace on every
    // context, the pinned rings and the host table (challenges)
    void scrub() {
        each_part([](StagePart &s) {
            (void)hipStreamSynchronize(s.mem.ctx->stream);
            s.mem.scrub(s.stage);
        });
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

// An oracle argument against the plan; empty, or what disagrees. A plan on one context takes oracles of that context, a sharded
// plan oracles sharded as its constants/sigmas oracle is, context by context. new_sharded: the argument is the constants/sigmas
// oracle of a sharded plan in the making, whose shards will be the plan's.
std::string oracle_mismatch(const qpgpu_stage_plan *pl, const qpgpu_oracle *o, size_t ncols, bool may_blind, bool new_sharded = false) {
    const CircuitPack &p = pl->pack;
    const size_t G = pl->shard_ctxs.size();
    if (new_sharded) {
        if (!o->sh) return "is not sharded: qpgpu_stage_plan_create takes an oracle of one context";
        if (o->ctx != pl->ctx) return "has another home context than ctx: the plan lives on the home context of its oracles";
    } else if (!pl->sharded()) {
        // its LDE lies in its shards, not behind o.lde: refused, never read as if shard 0 were the whole
        if (o->sh) return "is sharded over " + std::to_string(o->sh->s.size()) + " contexts: sharded oracles are not taken here yet";
        if (o->ctx != pl->ctx) return "belongs to another context";
    } else {
        if (!o->sh) return "is not sharded: the plan's cs_oracle is sharded over " + std::to_string(G) + " contexts and takes oracles sharded over the same ones";
        if (o->sh->s.size() != G) return "is sharded over " + std::to_string(o->sh->s.size()) + " contexts, the plan's cs_oracle over " + std::to_string(G);
        if (o->ctx != pl->ctx) return "has another home context than the plan's cs_oracle";
        for (size_t i = 0; i < G; i++)
            if (o->sh->s[i].ctx != pl->shard_ctxs[i]) return "runs shard " + std::to_string(i) + " on another context than the plan's cs_oracle";
    }
    if (o->o.ncols != ncols) return "has " + std::to_string(o->o.ncols) + " polynomials, the circuit needs " + std::to_string(ncols);
    if (o->o.log_n != p.degree_bits) return "has degree_bits " + std::to_string(o->o.log_n) + ", the circuit " + std::to_string(p.degree_bits);
    if (o->o.rate_bits != p.rate_bits) return "has rate_bits " + std::to_string(o->o.rate_bits) + ", the circuit " + std::to_string(p.rate_bits);
    if (!may_blind && o->o.salted()) return "is blinded: the constants/sigmas commitment carries no salt";
    return "";
}

// the LDE of shard g of an oracle, as part g walks it: with the oracle's own ps_lde (a sharded oracle holds one proof, stride 0);
// an oracle of one context is its own shard 0
const u64 *shard_lde(const qpgpu_oracle *o, uint32_t g) { return o->sh ? o->sh->s[g].lde : o->o.lde; }

// Part g of a plan in the making, on its context: the tables of its LDE, the workspace, the pinned ring. The home part (g = 0)
// also gets what s5 and the witness check read and, where several parts work, what the merge reads.
int build_part(qpgpu_stage_plan *pl, const std::string &who, uint32_t g) {
    qpgpu_ctx *home = pl->ctx, *c = g ? pl->shard_ctxs[g] : home;
    const CircuitPack &p = pl->pack;
    const shard_map::QuotientMap &m = pl->qmap;
    const u64 n = p.n(), M = m.points();
    const uint32_t Gq = m.working(), nch = (uint32_t)p.num_challenges, max_batch = pl->max_batch;
    pl->parts.emplace_back(new StagePart());
    StagePart &s = *pl->parts[g];
    s.mem.ctx = c;
    QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
    const StageAlloc take = [&s](u64 **ptr, size_t count, bool secret) { return s.mem.alloc(ptr, count, secret); };
    if (g == 0) {
        // the constants/sigmas polynomials on the subgroup (the sigma columns of s5, the witness check's constants): forward NTT of
        // the oracle's coefficients
        QP_TRY(take(&pl->d_cs_values, (size_t)p.num_cs_cols() * n, false));
        QP_TRY(ntt_run(c, pl->cs->o.coeffs, pl->d_cs_values, m.d, m.d, (size_t)p.num_cs_cols(), false, false, 0));
        s.tab.cs_values = pl->d_cs_values;
    }
    s.tab.cs_lde = shard_lde(pl->cs, g);
    const StageGeom geom = stage_geom_of(m, g);
    QP_SHARD(home, g, c, stage_tables_build(c, p, take, s.tab, &geom));
    if (g) {   // fused / pair / folded: decided once, by the home part's tables, for all parts
        const StageTables &t0 = pl->home().tab;
        s.tab.quotient_fused = t0.quotient_fused; s.tab.quotient_plain_map = t0.quotient_plain_map; s.tab.quotient_pair = t0.quotient_pair;
        s.tab.fold_words = t0.fold_words;
    }
    s.work.stage = &s.stage;
    QP_SHARD(home, g, c, stage_work_alloc(p, s.tab, take, max_batch, s.work, g != 0));
    if (g == 0) {
        QP_TRY(take(&pl->d_wires_vals, (size_t)max_batch * p.num_wires * n, true));
        pl->small.assign((size_t)max_batch * s.tab.small_words, 0);
    } else if (c->device != home->device) {
        QP_SHARD(home, g, c, take(&s.d_vals, (size_t)nch * M, true));
    }
    {
        s.stage.words = 2 * stage_ring_words(s.tab, max_batch) + 64;    // s6 puts the beta part again, then the alpha part and the check's seed
        void *hp = nullptr;
        const hipError_t e = c->track_host_malloc(&hp, s.stage.words * 8, residue::STAGE_PLAN);
        if (e != hipSuccess) return shard_fail(home, g, c, c->hip_fail(e, "hipHostMalloc(stage plan)"));
        s.stage.h = (u64 *)hp;
    }
    if (g == 0) {
        QP_TRY(c->reserve_read_back((1u << 12) + (size_t)max_batch * 16));
        if (Gq > 1) {
            QP_TRY(take(&pl->d_gather, (size_t)Gq * nch * M, true));
            // the merge kernel's table: w_Gq^-k, then g_mult^(-cM) / Gq
            std::vector<u64> tab(2 * (size_t)Gq);
            const u64 winv = gl::inv(gl::root_of_unity(m.log_working())), sinv = gl::pow(gl::inv(gl::MULT_GEN), M);
            u64 a = 1, b = gl::inv(Gq);
            for (uint32_t k = 0; k < Gq; k++) { tab[k] = gl::canon(a); tab[Gq + k] = gl::canon(b); a = gl::mul(a, winv); b = gl::mul(b, sinv); }
            QP_TRY(take(&pl->d_merge_tab, tab.size(), false));
            QP_TRY(h2d_sync(c, pl->d_merge_tab, tab.data(), tab.size() * 8));
        }
    } else {
        QP_SHARD_HIP(home, g, c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    {   // asynchronous faults of the setup kernels surface here
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return shard_fail(home, g, c, c->hip_fail(e, (who + "hipStreamSynchronize").c_str()));
    }
    return QPGPU_OK;
}

// The three creation entries. who: the entry's prefix in messages; sharded: cs_oracle is a coset-sharded oracle and the plan gets a
// part per working shard, else an oracle of ctx and the plan the home part alone.
int plan_create(const std::string &who, bool sharded, qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle,
                uint32_t max_batch, qpgpu_stage_plan **out, char *err) {
    if (err) err[0] = 0;
    if (!out) return refuse(ctx, err, QPGPU_EINVAL, who + "null plan pointer");
    *out = nullptr;
    if (!words) return refuse(ctx, err, QPGPU_EINVAL, who + "null words");
    // the header is checked first: it needs no device, and a refusal reads the same whether or not a GPU is present
    CircuitPack pack;
    {
        std::string why = pack.parse_stage(words, n_words);
        if (why.empty()) why = stage_limits(pack);
        if (!why.empty()) return refuse(ctx, err, QPGPU_EINVAL, who + why);
    }
    if (max_batch == 0 || max_batch > 1024)
        return refuse(ctx, err, QPGPU_EINVAL, who + "max_batch is " + std::to_string(max_batch) + ", it must be 1..1024");
    pack.constants_sigmas.clear(); pack.constants_sigmas.shrink_to_fit();   // the oracle holds them
    pack.header_only = true;
    if (!ctx) return refuse(ctx, err, QPGPU_EINVAL, who + "null context");
    if (!cs_oracle) return refuse(ctx, err, QPGPU_EINVAL, who + "null cs_oracle");
    QP_DEV(ctx);
    qpgpu_stage_plan *pl = new qpgpu_stage_plan();
    pl->ctx = ctx; pl->max_batch = max_batch; pl->pack = pack; pl->cs = cs_oracle;
    const CircuitPack &p = pl->pack;
    {
        std::string why = oracle_mismatch(pl, cs_oracle, p.num_cs_cols(), false, sharded);
        if (why.empty() && cs_oracle->o.nb != 1)
            why = "holds a batch of " + std::to_string(cs_oracle->o.nb) + " proofs: the constants/sigmas commitment is shared by all proofs";
        if (!why.empty()) { delete pl; return refuse(ctx, err, QPGPU_EINVAL, who + "cs_oracle " + why); }
    }
    if (sharded) for (const OracleShard &s : cs_oracle->sh->s) pl->shard_ctxs.push_back(s.ctx);
    pl->qmap = shard_map::QuotientMap::of((unsigned)p.degree_bits, (unsigned)p.rate_bits, p.quotient_degree_factor, sharded ? cs_oracle->sh->map.lg : 0);
    int rc = QPGPU_OK;
    for (uint32_t g = 0; g < pl->qmap.working() && rc == QPGPU_OK; g++) rc = build_part(pl, who, g);
    if (rc) {
        const std::string keep = ctx->err;
        qpgpu_stage_plan_free(pl);
        return refuse(ctx, err, rc, keep);
    }
    (void)hipSetDevice(ctx->device);
    *out = pl;
    return QPGPU_OK;
}

// a failed call leaves nothing witness-derived behind (as qpgpu_oracle_free does for its block); the message survives the scrub
int fail_scrubbed(qpgpu_stage_plan *pl, int rc) {
    const std::string keep = pl->ctx->err;
    pl->scrub();
    pl->ctx->err = keep;
    return rc;
}

}  // namespace

extern "C" {

void qpgpu_stage_plan_free(qpgpu_stage_plan *pl) {
    if (!pl) return;
    pl->scrub();
    pl->each_part([](StagePart &s) {
        if (s.done) (void)hipEventDestroy(s.done);
        s.mem.release(s.stage);
    });
    delete pl;
}

int qpgpu_stage_plan_create_batch(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, uint32_t max_batch,
                                  qpgpu_stage_plan **out, char *err) {
    return plan_create("stage_plan_create: ", false, ctx, words, n_words, cs_oracle, max_batch, out, err);
}

int qpgpu_stage_plan_create(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, qpgpu_stage_plan **out, char *err) {
    return plan_create("stage_plan_create: ", false, ctx, words, n_words, cs_oracle, 1, out, err);
}

int qpgpu_stage_plan_create_sharded(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, qpgpu_stage_plan **out,
                                    char *err) {
    return plan_create("stage_plan_create_sharded: ", true, ctx, words, n_words, cs_oracle, 1, out, err);
}

uint32_t qpgpu_stage_plan_shards(const qpgpu_stage_plan *pl) { return pl ? (pl->sharded() ? (uint32_t)pl->shard_ctxs.size() : 1) : 0; }

uint32_t qpgpu_stage_plan_max_batch(const qpgpu_stage_plan *pl) { return pl ? pl->max_batch : 0; }

int qpgpu_stage_plan_info(const qpgpu_stage_plan *pl, unsigned *degree_bits, unsigned *num_challenges, unsigned *num_partial_products,
                          unsigned *quotient_degree_factor, int *fused_selected) {
    if (!pl) return QPGPU_EINVAL;
    const CircuitPack &p = pl->pack;
    if (degree_bits) *degree_bits = (unsigned)p.degree_bits;
    if (num_challenges) *num_challenges = (unsigned)p.num_challenges;
    if (num_partial_products) *num_partial_products = (unsigned)p.num_partial_products;
    if (quotient_degree_factor) *quotient_degree_factor = (unsigned)p.quotient_degree_factor;
    if (fused_selected) *fused_selected = pl->home().tab.fused_selected(p) ? 1 : 0;
    return QPGPU_OK;
}

}  // extern "C"

namespace {

// The host copy of the small tables of nb proofs from their challenges, canonical: the beta part, and with alphas (and the
// public-input hashes) the alpha part too
void fill_small(qpgpu_stage_plan *pl, uint32_t nb, const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas = nullptr,
                const uint64_t *public_inputs_hashes = nullptr) {
    const CircuitPack &p = pl->pack;
    const size_t nch = p.num_challenges, SW = pl->home().tab.small_words;
    for (uint32_t b = 0; b < nb; b++) {
        u64 ch[12], pih[4];
        for (size_t k = 0; k < nch; k++) {
            ch[k] = gl::canon(betas[b * nch + k]); ch[4 + k] = gl::canon(gammas[b * nch + k]);
            if (alphas) ch[8 + k] = gl::canon(alphas[b * nch + k]);
        }
        stage_fill_betas(p, pl->small.data() + b * SW, ch, ch + 4);
        if (!alphas) continue;
        for (int i = 0; i < 4; i++) pih[i] = gl::canon(public_inputs_hashes[4 * (size_t)b + i]);
        stage_fill_alphas(p, pl->small.data() + b * SW, ch + 8, pih);
    }
}

// s5 for a lockstep batch; `who` is the entry's name in messages. wires: nb matrices, on the host or on the device.
int partial_products_impl(qpgpu_stage_plan *pl, const char *who, const uint64_t *const *wires, uint32_t nb, int wires_on_device,
                          const uint64_t *betas, const uint64_t *gammas, uint64_t *d_out) {
    qpgpu_ctx *ctx = pl->ctx;
    const CircuitPack &p = pl->pack;
    StagePart &h = pl->home();
    const size_t mat = (size_t)p.num_wires * p.n();
    fill_small(pl, nb, betas, gammas);
    h.stage.pos = 0;
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
    if (rc == QPGPU_OK) rc = stage_partial_products(ctx, p, h.tab, h.work, nb, pl->small.data(), d_wires, mat, d_out);
    if (rc == QPGPU_OK) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = ctx->hip_fail(e, (std::string(who) + ": hipStreamSynchronize").c_str());
    }
    return rc == QPGPU_OK ? rc : fail_scrubbed(pl, rc);
}

// s6 for a lockstep batch over the plan's parts. The oracles hold nb proofs each (the entries check it; a sharded plan and its
// oracles hold one). Parts 1 .. Gq - 1 are queued first, each on its own stream; the home part then runs the witness check and its
// own points, waits for the others' blocks and merges. A plan on one context has the home part alone, which writes d_out itself.
// Every stream is synchronised before the function returns.
int quotient_impl(qpgpu_stage_plan *pl, const char *who, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, uint32_t nb,
                  const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hashes, uint64_t *d_out) {
    qpgpu_ctx *home = pl->ctx;
    const CircuitPack &p = pl->pack;
    {
        std::string why = oracle_mismatch(pl, wires_oracle, p.num_wires, true);
        if (!why.empty()) return home->fail(QPGPU_EINVAL, std::string(who) + ": wires_oracle " + why);
        why = oracle_mismatch(pl, zs_pp_oracle, p.num_zs_pp_cols(), true);
        if (!why.empty()) return home->fail(QPGPU_EINVAL, std::string(who) + ": zs_pp_oracle " + why);
    }
    const shard_map::QuotientMap &m = pl->qmap;
    const u64 n = p.n(), M = m.points();
    const unsigned d = (unsigned)p.degree_bits;
    const uint32_t nch = (uint32_t)p.num_challenges, Gq = m.working();
    fill_small(pl, nb, betas, gammas, alphas, public_inputs_hashes);
    // the oracles' LDE columns are the polynomial columns only, stride lde_n: the salt columns of a blinded oracle lie in a
    // region of their own behind the digests and are never touched
    auto views = [&](uint32_t g, u64 *out) {
        QuotientViews v;
        v.wires_lde = shard_lde(wires_oracle, g); v.ps_wires_lde = wires_oracle->o.ps_lde;
        v.zs_lde = shard_lde(zs_pp_oracle, g); v.ps_zs_lde = zs_pp_oracle->o.ps_lde; v.out = out;
        return v;
    };
    auto run = [&]() -> int {
        for (uint32_t g = 1; g < Gq; g++) {
            StagePart &s = *pl->parts[g];
            qpgpu_ctx *c = s.mem.ctx;
            QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
            s.stage.pos = 0;
            u64 *block = pl->d_gather + (size_t)g * nch * M;
            const QuotientViews v = views(g, s.d_vals ? s.d_vals : block);   // on the home context's device the part's coefficients are written where the merge reads them
            QP_SHARD(home, g, c, stage_put_betas(c, p, s.tab, s.work, nb, pl->small.data()));
            QP_SHARD(home, g, c, stage_quotient_prepare(c, p, s.tab, s.work, nb, pl->small.data(), v));
            QP_SHARD(home, g, c, stage_quotient_values(c, p, s.tab, s.work, nb, v));
            if (s.d_vals) QP_SHARD_HIP(home, g, c, hipMemcpyPeerAsync(block, home->device, s.d_vals, c->device, (size_t)nch * M * 8, c->stream));
            QP_SHARD_HIP(home, g, c, hipEventRecord(s.done, c->stream));
        }
        QP_DEV(home);
        StagePart &h = pl->home();
        h.stage.pos = 0;
        QP_TRY(stage_put_betas(home, p, h.tab, h.work, nb, pl->small.data()));
        // The witness check of qpgpu_prove* (qpgpu_circuit_set_witness_check), always on here: the stage flow has no later point at
        // which an unsatisfied witness would show, the quotient of one is simply not a polynomial of the committed degree. It reads the
        // trace on the subgroup: wire and Z values from the coefficients the home context keeps (dense [nb][cols][n]: one transform
        // over all the proofs' wire columns; the Z columns are the first nch of each proof's Z/partial-products block), the row
        // products of the permutation argument from those wire values.
        QP_TRY(ntt_run(home, wires_oracle->o.coeffs, pl->d_wires_vals, d, d, (size_t)nb * p.num_wires, false, false, 0));
        QP_TRY(stage_pp_rows(home, p, h.tab, h.work, nb, pl->d_wires_vals, p.num_wires * n));
        NttProofs np; np.nproofs = nb; np.in_ps = zs_pp_oracle->o.ps_coeffs; np.out_ps = (u64)nch * n;
        QP_TRY(ntt_run(home, zs_pp_oracle->o.coeffs, h.work.d_z, d, d, (size_t)nch, false, false, 0, np));
        QuotientViews v = views(0, Gq > 1 ? pl->d_gather : d_out);           // one working part holds the whole quotient domain: nothing to merge
        v.check_wires = pl->d_wires_vals; v.ps_check_wires = p.num_wires * n;
        QP_TRY(stage_quotient_prepare(home, p, h.tab, h.work, nb, pl->small.data(), v));
        QP_TRY(stage_quotient_values(home, p, h.tab, h.work, nb, v));
        if (Gq > 1) {
            for (uint32_t g = 1; g < Gq; g++) QP_HIP(home, hipStreamWaitEvent(home->stream, pl->parts[g]->done, 0));
            home->prof_begin("prove_quotient_merge");
            const hipError_t e = pk_quotient_merge(pl->d_gather, d_out, M, nch, m.log_working(), pl->d_merge_tab, home->stream);
            home->prof_end();
            QP_HIP(home, e);
        }
        QP_HIP(home, hipStreamSynchronize(home->stream));
        for (uint32_t g = 1; g < Gq; g++) {               // done already (the home stream waited for them): asynchronous faults surface here
            qpgpu_ctx *c = pl->parts[g]->mem.ctx;
            QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
            QP_SHARD_HIP(home, g, c, hipStreamSynchronize(c->stream));
        }
        QP_DEV(home);
        return QPGPU_OK;
    };
    const int rc = run();
    return rc == QPGPU_OK ? rc : fail_scrubbed(pl, rc);
}

int refuse_batch_on_sharded(qpgpu_stage_plan *pl, const char *who, const char *single) {
    return pl->ctx->fail(QPGPU_EINVAL, std::string(who) + ": the plan is sharded over " + std::to_string(pl->shard_ctxs.size()) +
                                           " contexts: a sharded plan takes one proof (" + single + ")");
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
    if (pl->sharded()) return refuse_batch_on_sharded(pl, "stage_partial_products_batch", "qpgpu_stage_partial_products");
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
    if (!pl->sharded()) {   // a sharded plan's oracles are sharded ones, which hold one proof: whatever else is refused as not sharded
        if (wires_oracle->o.nb != 1) return ctx->fail(QPGPU_EINVAL, "stage_quotient: wires_oracle holds a batch of " + std::to_string(wires_oracle->o.nb) + " proofs, use qpgpu_stage_quotient_batch");
        if (zs_pp_oracle->o.nb != 1) return ctx->fail(QPGPU_EINVAL, "stage_quotient: zs_pp_oracle holds a batch of " + std::to_string(zs_pp_oracle->o.nb) + " proofs, use qpgpu_stage_quotient_batch");
    }
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
    if (pl->sharded()) return refuse_batch_on_sharded(pl, "stage_quotient_batch", "qpgpu_stage_quotient");
    if (batch == 0 || batch > pl->max_batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: batch is " + std::to_string(batch) + ", the plan's max_batch is " + std::to_string(pl->max_batch));
    if (wires_oracle->o.nb != batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: wires_oracle holds " + std::to_string(wires_oracle->o.nb) + " proofs, the call is for a batch of " + std::to_string(batch));
    if (zs_pp_oracle->o.nb != batch)
        return ctx->fail(QPGPU_EINVAL, "stage_quotient_batch: zs_pp_oracle holds " + std::to_string(zs_pp_oracle->o.nb) + " proofs, the call is for a batch of " + std::to_string(batch));
    return quotient_impl(pl, "stage_quotient_batch", wires_oracle, zs_pp_oracle, batch, betas, gammas, alphas, public_inputs_hashes, d_out);
}

}  // extern "C"
