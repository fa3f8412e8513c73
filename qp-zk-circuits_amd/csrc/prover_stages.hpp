// prover_stages.hpp — stages s5 (partial products) and s6 (quotient) as launch sequences over plain device views, and the
// witness-independent tables they read. Two callers: the all-in-one prover (prover.cpp, a lockstep batch on a circuit handle's
// workspace) and the stage-level C ABI (stage_api.cpp, one proof or a lockstep batch on a stage plan's workspace, reading the
// caller's oracles in place). One sequence, two callers: the two routes cannot drift apart in bytes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <functional>
#include <string>
#include <vector>
#include "circuit.hpp"
#include "ctx.hpp"
#include "prover_host.hpp"
#include "prover_kernels.hpp"
#include "quotient_shard_map.hpp"

// count words of device memory; secret = the region will hold witness-derived values (its owner overwrites it before release)
using StageAlloc = std::function<int(gl::u64 **p, size_t count, bool secret)>;

// The LDE that the s6 kernels walk. The circuit's own: shift g_mult, 2^(degree_bits + rate_bits) leaves, the quotient on every
// 2^(rate_bits - qbits)-th point. One shard's of a coset-sharded oracle (quotient_shard_map.hpp): a whole LDE at a lower rate on a
// shift of its own, so the same kernels evaluate it from tables built for that shift and rate. The circuit's own is the map of one
// shard (lg = 0), shard 0.
struct StageGeom {
    gl::u64 shift = 0;                   // the LDE's points are shift * w_(log_lde)^i
    unsigned log_lde = 0, rate_bits = 0;
    unsigned q_shift = 0, log_q = 0;     // the quotient points: natural index >> q_shift, 2^log_q of them
};
StageGeom stage_geom_of(const shard_map::QuotientMap &m, uint32_t g);

// What s5 and s6 read that does not depend on a witness. The owner (qpgpu_circuit, qpgpu_stage_plan) frees the allocations.
struct StageTables {
    StageGeom geom;                      // set by stage_tables_build
    // set by the owner: the constants/sigmas polynomials as values on the subgroup [num_cs_cols][n] and as LDE (leaf order, stride lde_n)
    const gl::u64 *cs_values = nullptr, *cs_lde = nullptr;
    // built by stage_tables_build
    GateDev *d_gates = nullptr;
    std::vector<GateDev> h_gates;
    bool has_p2_gate = false;            // the gate list holds a Poseidon2 gate: its constants are the context's d_p2_app block
    gl::u64 *d_poseidon_rc = nullptr;
    gl::u64 *d_omega = nullptr, *d_x_coset = nullptr, *d_l0_coset = nullptr, *d_zh_inv = nullptr;
    gl::u64 *d_ginv_lo = nullptr, *d_ginv_hi = nullptr; uint32_t ginv_lo_bits = 0;
    size_t small_words = 0;              // words of the per-proof small table: betas, gammas, beta_k_is, alpha pows, pi hash
    size_t fold_words = 0;               // words of the per-proof folded hash-gate weights (quotient_fold.hpp); 0: round by round
    bool quotient_fused = true;          // stage s6: quotient_perm_gates_kernel where the gate list allows it (QPGPU_QUOTIENT_FUSED)
    bool quotient_plain_map = false;     // QPGPU_QUOTIENT_XCD_MAP=0: that kernel's workgroups in proof-major order (measurement)
    bool quotient_pair = true;           // stage s6: both folded hash gates from quotient_hash_pair_kernel where they pair (QPGPU_QUOTIENT_PAIR)
    bool fused_selected(const CircuitPack &p) const;
    bool pair_selected(const CircuitPack &p) const;
};

// Per-proof workspace of s5 / s6: every buffer is [max_batch][one proof's size]
struct StageWork {
    gl::u64 *d_small = nullptr, *d_fold = nullptr;
    gl::u64 *d_qcp = nullptr, *d_rowprod = nullptr, *d_z = nullptr;
    gl::u64 *d_qacc = nullptr;
    gl::u64 *d_check = nullptr;          // [max_batch][2]: first bad row, permutation flag
    Stager *stage = nullptr;             // pinned staging of the small tables
};

// limits of the kernels (chunks, challenges, LDE size): empty, or the reason a pack is refused
std::string stage_limits(const CircuitPack &p);
// synchronous upload from pageable memory
int h2d_sync(qpgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
// gate table, Poseidon constants, subgroup / coset / vanishing tables; reads the QPGPU_QUOTIENT_* switches
// (geom: the LDE of s6 where it is not the circuit's own, i.e. a shard's)
int stage_tables_build(qpgpu_ctx *ctx, const CircuitPack &p, const StageAlloc &alloc, StageTables &t, const StageGeom *geom = nullptr);
// quotient_only: the workspace of pk_quotient alone (a shard that runs neither s5 nor the witness check)
int stage_work_alloc(const CircuitPack &p, const StageTables &t, const StageAlloc &alloc, uint32_t max_batch, StageWork &w, bool quotient_only = false);
// pinned words the two stages put into StageWork::stage per batch
size_t stage_ring_words(const StageTables &t, uint32_t max_batch);

// One proof's row of the host copy of the small table (t.small_words words)
void stage_fill_betas(const CircuitPack &p, gl::u64 *row, const gl::u64 *betas, const gl::u64 *gammas);
void stage_fill_alphas(const CircuitPack &p, gl::u64 *row, const gl::u64 *alphas, const gl::u64 pi_hash[4]);

// small: [nb][t.small_words] on the host. Uploads the beta part of the table (betas, gammas, beta_k_is).
int stage_put_betas(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const gl::u64 *small);
// row products and chunk quotients of the permutation argument from wire VALUES [num_wires][n] (proof b at + b * ps_wires),
// into w.d_qcp / w.d_rowprod
int stage_pp_rows(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const gl::u64 *d_wires, gl::u64 ps_wires);
// s5: stage_put_betas, stage_pp_rows, the scan into w.d_z and the Z / partial-product columns into d_zs_vals
// ([num_zs_pp_cols][n] per proof, dense: the order the Z/partial-products oracle commits them in)
int stage_partial_products(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const gl::u64 *small,
                           const gl::u64 *d_wires, gl::u64 ps_wires, gl::u64 *d_zs_vals);

struct QuotientViews {
    const gl::u64 *wires_lde = nullptr, *zs_lde = nullptr;   // leaf order, stride lde_n; proof b at + b * ps_*
    gl::u64 ps_wires_lde = 0, ps_zs_lde = 0;
    gl::u64 *out = nullptr;                                  // [nb][num_challenges][n * quotient_degree_factor], dense: values, then coefficients
    // the optional witness check: wire values on the subgroup; it reads w.d_z and w.d_rowprod as s5 (or stage_pp_rows) left them
    const gl::u64 *check_wires = nullptr; gl::u64 ps_check_wires = 0;
};
// s6: uploads the alpha part of the table (alpha powers, public-input hash; the beta part is already up), sweeps the folded hash
// gates' weights, runs the witness check when v.check_wires is set (QPGPU_EUNSAT names the row), then the quotient values on
// the coset of size n * quotient_degree_factor and their coefficients: num_quotient_cols chunks of n, back to back, in v.out
int stage_quotient(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const gl::u64 *small,
                   const QuotientViews &v);
// The two halves of stage_quotient, for a caller that runs them on different contexts (stage_api.cpp, a sharded plan): the alpha
// upload, the fold sweep and the witness check when v.check_wires is set; then the quotient values on t.geom's points and their
// coefficients in v.out, 2^t.geom.log_q per challenge (the inverse transform of that size, coefficient i times t.geom.shift^-i).
int stage_quotient_prepare(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const gl::u64 *small,
                           const QuotientViews &v);
int stage_quotient_values(qpgpu_ctx *ctx, const CircuitPack &p, const StageTables &t, const StageWork &w, uint32_t nb, const QuotientViews &v);
