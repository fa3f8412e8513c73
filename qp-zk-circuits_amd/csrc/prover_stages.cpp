// prover_stages.cpp — stages s5 and s6 of plonky2's prove() as launch sequences over plain device views (prover_stages.hpp):
// `all_wires_permutation_partial_products` and `compute_quotient_polys` of qp-plonky2 1.5.5 `plonk::prover`, and the tables both
// read. Called by the all-in-one prover (prover.cpp) and by the stage-level entries (stage_api.cpp).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include "gl64.hpp"
#include "poseidon.hpp"
#include "prover_stages.hpp"

using gl::u64;

namespace {

std::vector<u64> powers_table(u64 base, u64 count) {
    std::vector<u64> t(count);
    u64 a = 1;
    for (u64 i = 0; i < count; i++) { t[i] = gl::canon(a); a = gl::mul(a, base); }
    return t;
}

// the small table of one proof: [betas nch][gammas nch][beta_k_is nch*R][alpha_pows nch*nterms][pi_hash 4]
struct SmallLayout {
    size_t nch, R, nterms, betas, gammas, bk, apow, pih;
    explicit SmallLayout(const CircuitPack &p) {
        nch = p.num_challenges; R = p.num_routed_wires;
        nterms = nch + nch * p.num_chunks() + p.num_gate_constraints;
        betas = 0; gammas = nch; bk = 2 * nch; apow = bk + nch * R; pih = apow + nch * nterms;
    }
    size_t words() const { return (pih + 4 + 3) & ~(size_t)3; }
};

PpArgs pp_args(const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *d_wires, u64 ps_wires) {
    const SmallLayout sl(p);
    const u64 n = p.n();
    const uint32_t nch = (uint32_t)p.num_challenges, nchunks = (uint32_t)p.num_chunks();
    PpArgs pa{};
    pa.wires = d_wires; pa.sigmas = t.cs_values + (p.num_selectors + p.num_constants) * n; pa.omega_pows = t.d_omega; pa.beta_k_is = w.d_small + sl.bk;
    pa.betas = w.d_small + sl.betas; pa.gammas = w.d_small + sl.gammas; pa.qcp = w.d_qcp; pa.rowprod = w.d_rowprod; pa.n = n;
    pa.num_routed = (uint32_t)p.num_routed_wires; pa.chunk = (uint32_t)p.quotient_degree_factor; pa.nchunks = nchunks; pa.nch = nch;
    pa.batch = nb; pa.ps_wires = ps_wires; pa.ps_small = t.small_words; pa.ps_qcp = (u64)nch * nchunks * n; pa.ps_rowprod = (u64)nch * n;
    return pa;
}

}  // namespace

bool StageTables::fused_selected(const CircuitPack &p) const {
    return quotient_fused && pk_quotient_fused_gates(h_gates.data(), (uint32_t)h_gates.size(), (uint32_t)p.num_routed_wires,
                                                     (uint32_t)p.quotient_degree_factor, (uint32_t)p.num_partial_products + 1, nullptr);
}

bool StageTables::pair_selected(const CircuitPack &p) const {
    return quotient_pair && fold_words != 0 && pk_quotient_pairable(h_gates.data(), (uint32_t)h_gates.size(), p.p2_layout);
}

std::string stage_limits(const CircuitPack &p) {
    if (p.num_chunks() > 16 || p.num_challenges > 4) return "too many chunks/challenges";
    if (p.degree_bits + p.rate_bits > 23) return "LDE larger than 2^23 not supported";
    return "";
}

int h2d_sync(qpgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
    QP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    QP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // source is pageable and may go out of scope
    return QPGPU_OK;
}

StageGeom stage_geom_of(const shard_map::QuotientMap &m, uint32_t g) {
    // the quotient lives on the coset of size n * quotient_degree_factor: every 2^q_shift-th point of the LDE, i.e. its first q_n
    // slots; a working shard holds 2^log_q of those points, every 2^q_shift-th of its own LDE on the shift g_mult w_(d+r)^brev(g)
    StageGeom geom;
    geom.shift = gl::canon(gl::mul(gl::MULT_GEN, gl::pow(gl::root_of_unity(m.d + m.r), m.shift_exponent(g))));
    geom.log_lde = m.local_log_lde(); geom.rate_bits = m.local_rate_bits();
    geom.q_shift = m.local_q_shift(); geom.log_q = m.log_points();
    return geom;
}

int stage_tables_build(qpgpu_ctx *ctx, const CircuitPack &p, const StageAlloc &alloc, StageTables &t, const StageGeom *geom) {
    t.geom = geom ? *geom : stage_geom_of(shard_map::QuotientMap::of((unsigned)p.degree_bits, (unsigned)p.rate_bits, p.quotient_degree_factor, 0), 0);
    const u64 n = p.n(), lde_n = 1ull << t.geom.log_lde;
    const unsigned d = (unsigned)p.degree_bits, L = t.geom.log_lde;
    // gates
    std::vector<GateDev> gd(p.gates.size());
    for (size_t i = 0; i < gd.size(); i++) {
        const GateInfo &g = p.gates[i];
        gd[i] = {(uint32_t)g.type, (uint32_t)g.param0, (uint32_t)g.param1, (uint32_t)g.selector_index, (uint32_t)g.group_start,
                 (uint32_t)g.group_end, (uint32_t)g.num_constraints, (uint32_t)g.param2};
    }
    t.h_gates = gd;
    for (const GateInfo &g : p.gates) t.has_p2_gate = t.has_p2_gate || g.type == GATE_POSEIDON2;
    if (t.has_p2_gate) QP_TRY(ctx->ensure_p2_app());
    static_assert(sizeof(GateDev) % 8 == 0, "the gate table is allocated in words");
    QP_TRY(alloc((u64 **)&t.d_gates, gd.size() * (sizeof(GateDev) / 8), false));
    QP_TRY(h2d_sync(ctx, t.d_gates, gd.data(), gd.size() * sizeof(GateDev)));
    QP_TRY(alloc(&t.d_poseidon_rc, 360, false));
    QP_TRY(h2d_sync(ctx, t.d_poseidon_rc, poseidon::host_round_constants(), 360 * 8));
    // subgroup, coset and vanishing tables
    QP_TRY(alloc(&t.d_omega, n, false));
    { auto w = powers_table(gl::root_of_unity(d), n); QP_TRY(h2d_sync(ctx, t.d_omega, w.data(), n * 8)); }
    const uint32_t rate = 1u << t.geom.rate_bits;
    std::vector<u64> zh(rate), zh_inv(rate);
    { u64 gn = gl::pow(t.geom.shift, n), wr = gl::root_of_unity(t.geom.rate_bits), a = 1;
      for (uint32_t i = 0; i < rate; i++) { zh[i] = gl::canon(gl::sub(gl::mul(gn, a), 1)); zh_inv[i] = gl::inv(zh[i]); a = gl::mul(a, wr); } }
    u64 *d_zh = nullptr;
    QP_TRY(alloc(&d_zh, rate, false)); QP_TRY(alloc(&t.d_zh_inv, rate, false));
    QP_TRY(h2d_sync(ctx, d_zh, zh.data(), rate * 8)); QP_TRY(h2d_sync(ctx, t.d_zh_inv, zh_inv.data(), rate * 8));
    {
        const uint32_t lo_bits = (L + 1) / 2;
        u64 *d_lo = nullptr, *d_hi = nullptr;
        const u64 wL = gl::root_of_unity(L);
        auto lo = powers_table(wL, 1ull << lo_bits), hi = powers_table(gl::pow(wL, 1ull << lo_bits), 1ull << (L - lo_bits));
        QP_TRY(alloc(&d_lo, lo.size(), false)); QP_TRY(alloc(&d_hi, hi.size(), false));
        QP_TRY(h2d_sync(ctx, d_lo, lo.data(), lo.size() * 8)); QP_TRY(h2d_sync(ctx, d_hi, hi.data(), hi.size() * 8));
        QP_TRY(alloc(&t.d_x_coset, lde_n, false)); QP_TRY(alloc(&t.d_l0_coset, lde_n, false));
        hipError_t e = pk_coset_tables(lde_n, L, gl::canon(t.geom.shift), d_lo, d_hi, lo_bits, d_zh, rate, gl::canon(n % gl::P), t.d_x_coset, t.d_l0_coset, ctx->stream);
        if (e != hipSuccess) return ctx->hip_fail(e, "coset_tables");
        const u64 ginv = gl::inv(t.geom.shift);
        t.ginv_lo_bits = lo_bits;
        auto glo = powers_table(ginv, 1ull << lo_bits), ghi = powers_table(gl::pow(ginv, 1ull << lo_bits), 1ull << (L - lo_bits));
        QP_TRY(alloc(&t.d_ginv_lo, glo.size(), false)); QP_TRY(alloc(&t.d_ginv_hi, ghi.size(), false));
        QP_TRY(h2d_sync(ctx, t.d_ginv_lo, glo.data(), glo.size() * 8)); QP_TRY(h2d_sync(ctx, t.d_ginv_hi, ghi.data(), ghi.size() * 8));
    }
    t.small_words = SmallLayout(p).words();
    {
        // The hash gates' quotient kernels run in the folded form (quotient_fold.hpp). QPGPU_QUOTIENT_FOLD=0, read here and nowhere
        // else, keeps the round-by-round form for this circuit: the A/B measurement and the parity test.
        const uint32_t n_hash = pk_count_hash_gates(gd.data(), (uint32_t)gd.size());
        const char *e = getenv("QPGPU_QUOTIENT_FOLD");
        if (n_hash > 0 && n_hash <= qfold::MAX_GATES && !(e && *e == '0')) t.fold_words = (size_t)n_hash * p.num_challenges * qfold::WORDS;
    }
    // Stage s6 takes the permutation terms and the wire-local gates in one kernel where the gate list allows it
    // (pk_quotient_fused_gates). QPGPU_QUOTIENT_FUSED=0 starts on the two launches instead (qpgpu_circuit_set_quotient_fused
    // switches a circuit handle later); QPGPU_QUOTIENT_XCD_MAP=0 keeps the one kernel but drops its XCD-grouped workgroup order, for
    // measurements.
    if (const char *e = getenv("QPGPU_QUOTIENT_FUSED")) if (*e == '0') t.quotient_fused = false;
    if (const char *e = getenv("QPGPU_QUOTIENT_XCD_MAP")) if (*e == '0') t.quotient_plain_map = true;
    // A folded PoseidonGate and Poseidon2 gate on the same wires (qfold::pairable: the leaf circuit) share one launch, the target
    // wires' S-boxes and the linear term. QPGPU_QUOTIENT_PAIR=0, read here and nowhere else, keeps one launch per gate: the A/B
    // measurement and the parity test.
    if (const char *e = getenv("QPGPU_QUOTIENT_PAIR")) if (*e == '0') t.quotient_pair = false;
    return QPGPU_OK;
}

int stage_work_alloc(const CircuitPack &p, const StageTables &t, const StageAlloc &alloc, uint32_t B, StageWork &w, bool quotient_only) {
    const u64 n = p.n(), lde_n = 1ull << t.geom.log_lde, nch = p.num_challenges;
    QP_TRY(alloc(&w.d_qacc, (size_t)B * nch * lde_n, true));
    if (!quotient_only) {
        QP_TRY(alloc(&w.d_qcp, (size_t)B * nch * p.num_chunks() * n, true));
        QP_TRY(alloc(&w.d_rowprod, (size_t)B * nch * n, true));
        QP_TRY(alloc(&w.d_z, (size_t)B * nch * n, true));
    }
    QP_TRY(alloc(&w.d_small, (size_t)B * t.small_words, false));
    if (t.fold_words) QP_TRY(alloc(&w.d_fold, (size_t)B * t.fold_words, false));
    if (!quotient_only) QP_TRY(alloc(&w.d_check, (size_t)B * 2, false));
    return QPGPU_OK;
}

size_t stage_ring_words(const StageTables &t, uint32_t B) { return (size_t)B * (t.small_words + 4); }

void stage_fill_betas(const CircuitPack &p, u64 *row, const u64 *betas, const u64 *gammas) {
    const SmallLayout sl(p);
    for (size_t k = 0; k < sl.nch; k++) {
        // every entry canonical: quotient_perm_gates_kernel adds gamma_k with one carry fold (gl::add_canonical needs it)
        row[sl.betas + k] = gl::canon(betas[k]); row[sl.gammas + k] = gl::canon(gammas[k]);
        for (size_t j = 0; j < sl.R; j++) row[sl.bk + k * sl.R + j] = gl::canon(gl::mul(betas[k], p.k_is[j]));
    }
}

void stage_fill_alphas(const CircuitPack &p, u64 *row, const u64 *alphas, const u64 pi_hash[4]) {
    const SmallLayout sl(p);
    u64 *ap = row + sl.apow;
    for (size_t k = 0; k < sl.nch; k++) { u64 a = 1; for (size_t i = 0; i < sl.nterms; i++) { ap[k * sl.nterms + i] = gl::canon(a); a = gl::mul(a, alphas[k]); } }
    std::memcpy(row + sl.pih, pi_hash, 32);
}

int stage_put_betas(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *small) {
    const size_t SW = t.small_words;
    return w.stage->put_rows(ctx, w.d_small, SW, small, SW, SmallLayout(p).apow, nb);
}

int stage_pp_rows(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *d_wires, u64 ps_wires) {
    QP_HIP(ctx, pk_pp_rows(pp_args(p, t, w, nb, d_wires, ps_wires), ctx->stream));
    return QPGPU_OK;
}

int stage_partial_products(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *small,
                           const u64 *d_wires, u64 ps_wires, u64 *d_zs_vals) {
    hipStream_t st = ctx->stream;
    const u64 n = p.n();
    const uint32_t nch = (uint32_t)p.num_challenges;
    // (the alpha part of the table is uploaded after the Z commitment; this upload covers betas .. beta_k_is)
    QP_TRY(stage_put_betas(ctx, p, t, w, nb, small));
    ctx->prof_begin("prove_partial_products");
    const PpArgs pa = pp_args(p, t, w, nb, d_wires, ps_wires);
    QP_HIP(ctx, pk_pp_rows(pa, st));
    QP_HIP(ctx, pk_pp_scan(w.d_rowprod, w.d_z, n, nch * nb, st));
    QP_HIP(ctx, pk_pp_finish(pa, w.d_z, d_zs_vals, (u64)nch * n, (u64)p.num_zs_pp_cols() * n, st));
    ctx->prof_end();
    return QPGPU_OK;
}

namespace {
// the part of the s6 argument block that the fold sweep reads, shared by the two halves below
QuotientArgs quotient_args_base(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb) {
    const SmallLayout sl(p);
    QuotientArgs qa{};
    qa.alpha_pows = w.d_small + sl.apow; qa.poseidon_rc = t.d_poseidon_rc; qa.p2_gate = ctx->d_p2_app; qa.p2_layout = p.p2_layout;
    qa.nch = (uint32_t)p.num_challenges; qa.nchunks = (uint32_t)p.num_chunks(); qa.nterms = (uint32_t)sl.nterms;
    qa.num_gates = (uint32_t)p.gates.size(); qa.batch = nb; qa.ps_small = t.small_words;
    qa.fold = w.d_fold; qa.ps_fold = t.fold_words;
    return qa;
}
}  // namespace

int stage_quotient(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *small,
                   const QuotientViews &v) {
    QP_TRY(stage_quotient_prepare(ctx, p, t, w, nb, small, v));
    return stage_quotient_values(ctx, p, t, w, nb, v);
}

int stage_quotient_prepare(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const u64 *small,
                           const QuotientViews &v) {
    hipStream_t st = ctx->stream;
    const SmallLayout sl(p);
    const u64 n = p.n(), R = p.num_routed_wires;
    const uint32_t nch = (uint32_t)p.num_challenges, nchunks = (uint32_t)p.num_chunks();
    const unsigned d = (unsigned)p.degree_bits;
    const size_t sig0 = p.num_selectors + p.num_constants, nterms = sl.nterms, SW = t.small_words;
    u64 *d_apow = w.d_small + sl.apow, *d_pih = w.d_small + sl.pih;

    QP_TRY(w.stage->put_rows(ctx, d_apow, SW, small + sl.apow, SW, (size_t)nch * nterms + 4, nb));
    // the folded hash gates' weights for this batch's alphas: one small launch, read by the gate kernels of the witness check and of s6
    const QuotientArgs qa = quotient_args_base(ctx, p, t, w, nb);
    QP_HIP(ctx, pk_quotient_fold_sweep(qa, t.h_gates.data(), st));
    if (v.check_wires) {
        // the analogue of plonky2's debug assertions: filtered gate constraints must vanish on every trace row and the
        // permutation product must close; alpha-weighted sums are zero iff every constraint is (alpha is a transcript challenge)
        QuotientArgs ta{};
        ta.wires = v.check_wires; ta.cs = t.cs_values; ta.alpha_pows = d_apow; ta.pi_hash = d_pih; ta.gates = t.d_gates;
        ta.acc = w.d_qacc; ta.out = w.d_qacc; ta.poseidon_rc = t.d_poseidon_rc;
        ta.p2_gate = ctx->d_p2_app; ta.p2_layout = p.p2_layout;
        ta.zh_inv = t.d_zh_inv; ta.lde_n = n; ta.q_n = n; ta.q_shift = 0; ta.log_lde = d; ta.rate = 1; ta.nch = nch; ta.num_routed = (uint32_t)R;
        ta.chunk = (uint32_t)p.quotient_degree_factor; ta.nchunks = nchunks; ta.sig0 = (uint32_t)sig0;
        ta.num_selectors = (uint32_t)p.num_selectors; ta.num_gates = (uint32_t)p.gates.size(); ta.nterms = (uint32_t)nterms;
        ta.batch = nb; ta.ps_wires = v.ps_check_wires; ta.ps_zs = 0; ta.ps_small = SW; ta.ps_acc = (u64)nch * n; ta.ps_out = (u64)nch * n;
        ta.fold = w.d_fold; ta.ps_fold = t.fold_words; ta.pair = t.quotient_pair ? 1 : 0;
        QP_HIP(ctx, hipMemsetAsync(w.d_qacc, 0, (size_t)nb * nch * n * 8, st));
        std::vector<u64> init(2 * (size_t)nb);
        for (uint32_t b = 0; b < nb; b++) { init[2 * b] = ~0ull; init[2 * b + 1] = 0; }
        QP_TRY(w.stage->put(ctx, w.d_check, init.data(), init.size() * 8));
        QP_HIP(ctx, pk_gate_sums(ta, t.h_gates.data(), st));
        QP_HIP(ctx, pk_witness_check(w.d_qacc, n, nch, w.d_z, w.d_rowprod, w.d_check, nb, st));
        std::vector<u64> res(2 * (size_t)nb);
        QP_TRY(ctx->read_back(res.data(), w.d_check, res.size() * 8));
        for (uint32_t b = 0; b < nb; b++) {
            const std::string who = nb > 1 ? " (proof " + std::to_string(b) + " of the batch)" : "";
            if (res[2 * b] != ~0ull) return ctx->fail(QPGPU_EUNSAT, "witness does not satisfy the circuit: gate constraints fail at row " + std::to_string(res[2 * b]) + who);
            if (res[2 * b + 1]) return ctx->fail(QPGPU_EUNSAT, "witness does not satisfy the circuit: a copy constraint is violated (permutation product != 1)" + who);
        }
    }
    return QPGPU_OK;
}

int stage_quotient_values(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const QuotientViews &v) {
    hipStream_t st = ctx->stream;
    const SmallLayout sl(p);
    const u64 lde_n = 1ull << t.geom.log_lde, R = p.num_routed_wires;
    const uint32_t nch = (uint32_t)p.num_challenges, nchunks = (uint32_t)p.num_chunks();
    const unsigned L = t.geom.log_lde, Lq = t.geom.log_q, q_shift = t.geom.q_shift;
    const size_t sig0 = p.num_selectors + p.num_constants, nterms = sl.nterms, SW = t.small_words;
    const u64 q_n = 1ull << Lq;
    u64 *d_betas = w.d_small + sl.betas, *d_gammas = w.d_small + sl.gammas, *d_bk = w.d_small + sl.bk, *d_apow = w.d_small + sl.apow, *d_pih = w.d_small + sl.pih;
    QuotientArgs qa = quotient_args_base(ctx, p, t, w, nb);
    ctx->prof_begin("prove_quotient");
    qa.wires = v.wires_lde; qa.cs = t.cs_lde; qa.zs_pp = v.zs_lde; qa.x_coset = t.d_x_coset; qa.l0_coset = t.d_l0_coset;
    qa.zh_inv = t.d_zh_inv; qa.alpha_pows = d_apow; qa.beta_k_is = d_bk; qa.betas = d_betas; qa.gammas = d_gammas; qa.pi_hash = d_pih;
    qa.gates = t.d_gates; qa.acc = w.d_qacc; qa.poseidon_rc = t.d_poseidon_rc; qa.out = v.out;
    qa.p2_gate = ctx->d_p2_app; qa.p2_layout = p.p2_layout; qa.lde_n = lde_n; qa.q_n = q_n; qa.q_shift = q_shift; qa.log_lde = L; qa.rate = 1u << t.geom.rate_bits; qa.nch = nch;
    qa.num_routed = (uint32_t)R; qa.chunk = (uint32_t)p.quotient_degree_factor; qa.nchunks = nchunks; qa.sig0 = (uint32_t)sig0;
    qa.num_selectors = (uint32_t)p.num_selectors; qa.num_gates = (uint32_t)p.gates.size(); qa.nterms = (uint32_t)nterms;
    qa.batch = nb; qa.ps_wires = v.ps_wires_lde; qa.ps_zs = v.ps_zs_lde; qa.ps_small = SW; qa.ps_acc = (u64)nch * lde_n; qa.ps_out = (u64)nch * q_n;
    qa.fused = t.quotient_fused ? 1 : 0; qa.fused_plain_map = t.quotient_plain_map ? 1 : 0; qa.pair = t.quotient_pair ? 1 : 0;
    QP_HIP(ctx, pk_quotient(qa, t.h_gates.data(), st));
    // coset_ifft(shift) on the quotient domain: ifft then scale coefficient i by shift^-i; the qdf*n coefficients of a challenge
    // are its qdf chunks of n, contiguous
    QP_TRY(ntt_run(ctx, v.out, v.out, Lq, Lq, (size_t)nch * nb, true, false, 0));
    QP_HIP(ctx, pk_scale_powers(v.out, q_n, (u64)nch * nb, t.d_ginv_lo, t.d_ginv_hi, t.ginv_lo_bits, st));
    ctx->prof_end();
    return QPGPU_OK;
}
