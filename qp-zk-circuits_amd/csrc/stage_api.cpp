// stage_api.cpp — stage-level C ABI for the two gate-dependent stages of qp-plonky2's prove(): partial products (s5,
// `all_wires_permutation_partial_products`) and the quotient (s6, `compute_quotient_polys`), for a caller that runs the stage
// flow of oracle_api.cpp (include/qpgpu.h, "stage-level entry points"). A qpgpu_stage_plan holds what the two stages need and
// what does not depend on a witness: the tables a circuit handle prepares at load, built from the pack's header and the
// caller's constants/sigmas oracle. The launch sequences are the all-in-one prover's (prover_stages.cpp), for a lockstep batch of
// up to the plan's max_batch proofs (the single-proof entries are the batch of one), reading the caller's oracles in place: no
// LDE leaves the device.
//
// A plan over a coset-sharded constants/sigmas oracle (qpgpu_stage_plan_create_sharded) runs s6 on the shards: a shard's leaves are a
// whole LDE of their own, so working shard g runs the same launch sequence on its own context, over tables built for its shift and
// rate (quotient_shard_map.hpp), and the home context turns the shards' coefficients into the chunks (pk_quotient_merge). s5 and the
// witness check stay on the home context, which keeps the coefficients. The calling thread drives every stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include "oracle_handle.hpp"
#include "prover_stages.hpp"
#include "quotient_shard_map.hpp"

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

// Working shard g >= 1 of a sharded plan, on its own context: the tables of its LDE, the workspace of the quotient kernels and the
// pinned staging of its copy of the small table. (Shard 0 is the home context's: the plan's own tables, built for shard 0's LDE.)
struct StageShard {
    StageMem mem;
    StageTables tab;
    StageWork work;
    Stager stage;
    u64 *d_vals = nullptr;           // [nch][M] on another device than the home context's; on the same one the shard writes its gather block in place
    hipEvent_t done = nullptr;       // recorded on the shard's stream behind its block of the gather buffer
};

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
    StageMem mem;
    // qpgpu_stage_plan_create_sharded: the contexts of cs's shards in order (empty: a plan on one context), the arithmetic of who
    // evaluates what, working shards 1 .. Gq - 1 (index 0 unused), and on the home context the gather buffer [Gq][nch][M] and the
    // merge kernel's table, both only where Gq > 1
    std::vector<qpgpu_ctx *> shard_ctxs;
    shard_map::QuotientMap qmap;
    std::vector<std::unique_ptr<StageShard>> shards;
    u64 *d_gather = nullptr, *d_merge_tab = nullptr;

    bool sharded() const { return !shard_ctxs.empty(); }
    int alloc(u64 **p, size_t count, bool secret) { return mem.alloc(p, count, secret); }
    // wait for every stream of the plan, then overwrite everything that held witness-derived values: the workspace on every shard
    // context, the host table (challenges) and the pinned rings. Leaves the home context's device selected.
    void scrub() {
        for (auto &s : shards) {
            if (!s) continue;
            (void)hipSetDevice(s->mem.ctx->device);
            (void)hipStreamSynchronize(s->mem.ctx->stream);
            s->mem.scrub(s->stage);
        }
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        mem.scrub(stage);
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

// the same for a sharded plan: the argument must be sharded as the plan's constants/sigmas oracle is, context by context
std::string sharded_mismatch(const qpgpu_stage_plan *pl, const qpgpu_oracle *o, size_t ncols) {
    const CircuitPack &p = pl->pack;
    const size_t G = pl->shard_ctxs.size();
    if (!o->sh) return "is not sharded: the plan's cs_oracle is sharded over " + std::to_string(G) + " contexts and takes oracles sharded over the same ones";
    if (o->sh->s.size() != G) return "is sharded over " + std::to_string(o->sh->s.size()) + " contexts, the plan's cs_oracle over " + std::to_string(G);
    if (o->ctx != pl->ctx) return "has another home context than the plan's cs_oracle";
    for (size_t i = 0; i < G; i++)
        if (o->sh->s[i].ctx != pl->shard_ctxs[i]) return "runs shard " + std::to_string(i) + " on another context than the plan's cs_oracle";
    if (o->o.ncols != ncols) return "has " + std::to_string(o->o.ncols) + " polynomials, the circuit needs " + std::to_string(ncols);
    if (o->o.log_n != p.degree_bits) return "has degree_bits " + std::to_string(o->o.log_n) + ", the circuit " + std::to_string(p.degree_bits);
    if (o->o.rate_bits != p.rate_bits) return "has rate_bits " + std::to_string(o->o.rate_bits) + ", the circuit " + std::to_string(p.rate_bits);
    return "";
}

// a failure on a shard's context is reported where the caller looks: on the home context
int shard_fail(qpgpu_ctx *home, uint32_t g, qpgpu_ctx *ctx, int rc) {
    if (ctx != home) home->err = "shard " + std::to_string(g) + ": " + ctx->err;
    return rc;
}
#define QP_SHARD(home, g, sctx, expr) do { int _rc = (expr); if (_rc) return shard_fail(home, g, sctx, _rc); } while (0)
#define QP_SHARD_HIP(home, g, sctx, call) do { hipError_t _e = (call); if (_e != hipSuccess) return shard_fail(home, g, sctx, (sctx)->hip_fail(_e, #call)); } while (0)

// the LDE of shard g of the plan's oracles, as the s6 kernels walk it
StageGeom shard_geom(const shard_map::QuotientMap &m, uint32_t g) {
    StageGeom geom;
    geom.shift = gl::canon(gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity(m.d + m.r), m.shift_exponent(g))));
    geom.log_lde = m.local_log_lde(); geom.rate_bits = m.local_rate_bits();
    geom.q_shift = m.local_q_shift(); geom.log_q = m.log_points();
    return geom;
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
    pl->scrub();                                      // every shard's workspace on its own context; ends on the home context's device
    for (auto &s : pl->shards) {
        if (!s) continue;
        (void)hipSetDevice(s->mem.ctx->device);
        if (s->done) (void)hipEventDestroy(s->done);
        s->mem.release(s->stage);
    }
    (void)hipSetDevice(pl->ctx->device);
    pl->mem.release(pl->stage);
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
    pl->ctx = ctx; pl->mem.ctx = ctx; pl->max_batch = max_batch; pl->pack = pack; pl->cs = cs_oracle;
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

int qpgpu_stage_plan_create_sharded(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle, qpgpu_stage_plan **out,
                                    char *err) {
    const std::string who = "stage_plan_create_sharded: ";
    if (err) err[0] = 0;
    if (!out) return refuse(ctx, err, QPGPU_EINVAL, who + "null plan pointer");
    *out = nullptr;
    if (!words) return refuse(ctx, err, QPGPU_EINVAL, who + "null words");
    CircuitPack pack;
    {
        std::string why = pack.parse_stage(words, n_words);
        if (why.empty()) why = stage_limits(pack);
        if (!why.empty()) return refuse(ctx, err, QPGPU_EINVAL, who + why);
    }
    pack.constants_sigmas.clear(); pack.constants_sigmas.shrink_to_fit();
    pack.header_only = true;
    if (!ctx) return refuse(ctx, err, QPGPU_EINVAL, who + "null context");
    if (!cs_oracle) return refuse(ctx, err, QPGPU_EINVAL, who + "null cs_oracle");
    QP_DEV(ctx);
    {
        const PolyOracle &o = cs_oracle->o;
        std::string why;
        if (!cs_oracle->sh) why = "is not sharded: qpgpu_stage_plan_create takes an oracle of one context";
        else if (cs_oracle->ctx != ctx) why = "has another home context than ctx: the plan lives on the home context of its oracles";
        else if (o.ncols != pack.num_cs_cols()) why = "has " + std::to_string(o.ncols) + " polynomials, the circuit needs " + std::to_string(pack.num_cs_cols());
        else if (o.log_n != pack.degree_bits) why = "has degree_bits " + std::to_string(o.log_n) + ", the circuit " + std::to_string(pack.degree_bits);
        else if (o.rate_bits != pack.rate_bits) why = "has rate_bits " + std::to_string(o.rate_bits) + ", the circuit " + std::to_string(pack.rate_bits);
        else if (o.salted()) why = "is blinded: the constants/sigmas commitment carries no salt";
        if (!why.empty()) return refuse(ctx, err, QPGPU_EINVAL, who + "cs_oracle " + why);
    }
    qpgpu_stage_plan *pl = new qpgpu_stage_plan();
    pl->ctx = ctx; pl->mem.ctx = ctx; pl->max_batch = 1; pl->pack = pack; pl->cs = cs_oracle;
    const CircuitPack &p = pl->pack;
    const OracleShards &csh = *cs_oracle->sh;
    for (const OracleShard &s : csh.s) pl->shard_ctxs.push_back(s.ctx);
    shard_map::QuotientMap &m = pl->qmap;
    m.d = (unsigned)p.degree_bits; m.r = (unsigned)p.rate_bits; m.lg = csh.map.lg;
    while ((1ull << m.qbits) < p.quotient_degree_factor) m.qbits++;
    const u64 n = p.n(), M = m.points();
    const unsigned d = m.d;
    const uint32_t Gq = m.working(), nch = (uint32_t)p.num_challenges;
    auto fail = [&](int code) {
        const std::string keep = ctx->err;
        qpgpu_stage_plan_free(pl);
        return refuse(ctx, err, code, keep);
    };
    // ---- the home context: what every plan has, with the tables of s6 built for shard 0's LDE ----
    auto build_home = [&]() -> int {
        const StageAlloc take = [pl](u64 **ptr, size_t count, bool secret) { return pl->alloc(ptr, count, secret); };
        QP_TRY(pl->alloc(&pl->d_cs_values, (size_t)p.num_cs_cols() * n, false));
        QP_TRY(ntt_run(ctx, cs_oracle->o.coeffs, pl->d_cs_values, d, d, (size_t)p.num_cs_cols(), false, false, 0));
        pl->tab.cs_values = pl->d_cs_values; pl->tab.cs_lde = csh.s[0].lde;
        const StageGeom geom = shard_geom(m, 0);
        QP_TRY(stage_tables_build(ctx, p, take, pl->tab, &geom));
        pl->work.stage = &pl->stage;
        QP_TRY(stage_work_alloc(p, pl->tab, take, 1, pl->work));
        QP_TRY(pl->alloc(&pl->d_wires_vals, (size_t)p.num_wires * n, true));
        pl->small.assign(pl->tab.small_words, 0);
        pl->stage.words = 2 * stage_ring_words(pl->tab, 1) + 64;
        void *hp = nullptr;
        const hipError_t e = ctx->track_host_malloc(&hp, pl->stage.words * 8, residue::STAGE_PLAN);
        if (e != hipSuccess) return ctx->hip_fail(e, "hipHostMalloc(stage plan)");
        pl->stage.h = (u64 *)hp;
        QP_TRY(ctx->reserve_read_back((1u << 12) + 16));
        if (Gq > 1) {
            QP_TRY(pl->alloc(&pl->d_gather, (size_t)Gq * nch * M, true));
            // the merge kernel's table: w_Gq^-k, then g_mult^(-cM) / Gq
            std::vector<u64> tab(2 * (size_t)Gq);
            const u64 winv = gl::inv(gl::root_of_unity(m.log_working())), sinv = gl::pow(gl::inv(gl::MULT_GEN), M);
            u64 a = 1, b = gl::inv(Gq);
            for (uint32_t k = 0; k < Gq; k++) { tab[k] = gl::canon(a); tab[Gq + k] = gl::canon(b); a = gl::mul(a, winv); b = gl::mul(b, sinv); }
            QP_TRY(pl->alloc(&pl->d_merge_tab, tab.size(), false));
            QP_TRY(h2d_sync(ctx, pl->d_merge_tab, tab.data(), tab.size() * 8));
        }
        QP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // asynchronous faults of the setup kernels surface here
        return QPGPU_OK;
    };
    int rc = build_home();
    if (rc) return fail(rc);
    // ---- working shards 1 .. Gq - 1, each on its own context: tables for its shift and rate, the quotient kernels' workspace ----
    pl->shards.resize(Gq);
    auto build_shard = [&](uint32_t g) -> int {
        pl->shards[g].reset(new StageShard());
        StageShard &s = *pl->shards[g];
        qpgpu_ctx *c = pl->shard_ctxs[g];
        s.mem.ctx = c;
        QP_SHARD_HIP(ctx, g, c, hipSetDevice(c->device));
        const StageAlloc take = [&s](u64 **ptr, size_t count, bool secret) { return s.mem.alloc(ptr, count, secret); };
        s.tab.cs_lde = csh.s[g].lde;
        const StageGeom geom = shard_geom(m, g);
        QP_SHARD(ctx, g, c, stage_tables_build(c, p, take, s.tab, &geom));
        // fused / pair / folded: decided once, by the home context's tables, for all shards
        s.tab.quotient_fused = pl->tab.quotient_fused; s.tab.quotient_plain_map = pl->tab.quotient_plain_map; s.tab.quotient_pair = pl->tab.quotient_pair;
        s.tab.fold_words = pl->tab.fold_words;
        s.work.stage = &s.stage;
        QP_SHARD(ctx, g, c, stage_work_alloc(p, s.tab, take, 1, s.work, true));
        if (c->device != ctx->device) QP_SHARD(ctx, g, c, s.mem.alloc(&s.d_vals, (size_t)nch * M, true));
        s.stage.words = 2 * stage_ring_words(s.tab, 1) + 64;
        void *hp = nullptr;
        QP_SHARD_HIP(ctx, g, c, c->track_host_malloc(&hp, s.stage.words * 8, residue::STAGE_PLAN));
        s.stage.h = (u64 *)hp;
        QP_SHARD_HIP(ctx, g, c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        QP_SHARD_HIP(ctx, g, c, hipStreamSynchronize(c->stream));
        return QPGPU_OK;
    };
    for (uint32_t g = 1; g < Gq && rc == QPGPU_OK; g++) rc = build_shard(g);
    if (rc) return fail(rc);
    (void)hipSetDevice(ctx->device);
    *out = pl;
    return QPGPU_OK;
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

// s6 on a sharded plan: working shards 1 .. Gq - 1 are queued first, each on its own stream; the home context then runs the witness
// check and shard 0, waits for the others' blocks and merges. Every stream is synchronised before the function returns.
int quotient_sharded_impl(qpgpu_stage_plan *pl, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, const uint64_t *betas,
                          const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hash, uint64_t *d_out) {
    qpgpu_ctx *home = pl->ctx;
    const CircuitPack &p = pl->pack;
    {
        std::string why = sharded_mismatch(pl, wires_oracle, p.num_wires);
        if (!why.empty()) return home->fail(QPGPU_EINVAL, "stage_quotient: wires_oracle " + why);
        why = sharded_mismatch(pl, zs_pp_oracle, p.num_zs_pp_cols());
        if (!why.empty()) return home->fail(QPGPU_EINVAL, "stage_quotient: zs_pp_oracle " + why);
    }
    const shard_map::QuotientMap &m = pl->qmap;
    const u64 n = p.n(), M = m.points();
    const unsigned d = (unsigned)p.degree_bits;
    const uint32_t nch = (uint32_t)p.num_challenges, Gq = m.working();
    {
        u64 ch[12], pih[4];
        for (uint32_t k = 0; k < nch; k++) { ch[k] = gl::canon(betas[k]); ch[4 + k] = gl::canon(gammas[k]); ch[8 + k] = gl::canon(alphas[k]); }
        for (int i = 0; i < 4; i++) pih[i] = gl::canon(public_inputs_hash[i]);
        stage_fill_betas(p, pl->small.data(), ch, ch + 4);
        stage_fill_alphas(p, pl->small.data(), ch + 8, pih);
    }
    const OracleShards &wsh = *wires_oracle->sh, &zsh = *zs_pp_oracle->sh;
    auto run = [&]() -> int {
        for (uint32_t g = 1; g < Gq; g++) {
            StageShard &s = *pl->shards[g];
            qpgpu_ctx *c = s.mem.ctx;
            QP_SHARD_HIP(home, g, c, hipSetDevice(c->device));
            s.stage.pos = 0;
            u64 *block = pl->d_gather + (size_t)g * nch * M;
            QuotientViews v;
            v.wires_lde = wsh.s[g].lde; v.zs_lde = zsh.s[g].lde;
            v.out = s.d_vals ? s.d_vals : block;         // on the home context's device the shard's coefficients are written where the merge reads them
            QP_SHARD(home, g, c, stage_put_betas(c, p, s.tab, s.work, 1, pl->small.data()));
            QP_SHARD(home, g, c, stage_quotient_prepare(c, p, s.tab, s.work, 1, pl->small.data(), v));
            QP_SHARD(home, g, c, stage_quotient_values(c, p, s.tab, s.work, 1, v));
            if (s.d_vals) QP_SHARD_HIP(home, g, c, hipMemcpyPeerAsync(block, home->device, s.d_vals, c->device, (size_t)nch * M * 8, c->stream));
            QP_SHARD_HIP(home, g, c, hipEventRecord(s.done, c->stream));
        }
        QP_DEV(home);
        pl->stage.pos = 0;
        QP_TRY(stage_put_betas(home, p, pl->tab, pl->work, 1, pl->small.data()));
        // the witness check's inputs, from the coefficients the home context keeps (as quotient_impl)
        QP_TRY(ntt_run(home, wires_oracle->o.coeffs, pl->d_wires_vals, d, d, (size_t)p.num_wires, false, false, 0));
        QP_TRY(stage_pp_rows(home, p, pl->tab, pl->work, 1, pl->d_wires_vals, p.num_wires * n));
        QP_TRY(ntt_run(home, zs_pp_oracle->o.coeffs, pl->work.d_z, d, d, (size_t)nch, false, false, 0));
        QuotientViews v;
        v.wires_lde = wsh.s[0].lde; v.zs_lde = zsh.s[0].lde;
        v.out = Gq > 1 ? pl->d_gather : d_out;           // one working shard holds the whole quotient domain: nothing to merge
        v.check_wires = pl->d_wires_vals; v.ps_check_wires = p.num_wires * n;
        QP_TRY(stage_quotient_prepare(home, p, pl->tab, pl->work, 1, pl->small.data(), v));
        QP_TRY(stage_quotient_values(home, p, pl->tab, pl->work, 1, v));
        if (Gq > 1) {
            for (uint32_t g = 1; g < Gq; g++) QP_HIP(home, hipStreamWaitEvent(home->stream, pl->shards[g]->done, 0));
            home->prof_begin("prove_quotient_merge");
            const hipError_t e = pk_quotient_merge(pl->d_gather, d_out, M, nch, m.log_working(), pl->d_merge_tab, home->stream);
            home->prof_end();
            QP_HIP(home, e);
        }
        QP_HIP(home, hipStreamSynchronize(home->stream));
        for (uint32_t g = 1; g < Gq; g++) {               // done already (the home stream waited for them): asynchronous faults surface here
            qpgpu_ctx *c = pl->shards[g]->mem.ctx;
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
    if (pl->sharded()) return quotient_sharded_impl(pl, wires_oracle, zs_pp_oracle, betas, gammas, alphas, public_inputs_hash, d_out);
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
