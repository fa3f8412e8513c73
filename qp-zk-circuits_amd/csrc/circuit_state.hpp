// circuit_state.hpp — a loaded circuit: setup-time residents and the per-proof workspace (one per in-flight proof).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "circuit.hpp"
#include "ctx.hpp"
#include "prover_host.hpp"
#include "prover_kernels.hpp"
#include "prover_stages.hpp"

struct WitnessPlan;
void witness_plan_free(WitnessPlan *p, qpgpu_ctx *ctx);
// stream-ordered zero fill of the plan's value buffers (public-input values and hash, prepared assignment values, ChaCha keys);
// null plan: nothing
void witness_plan_scrub(WitnessPlan *p, hipStream_t st);

struct qpgpu_circuit {
    qpgpu_ctx *ctx = nullptr;
    CircuitPack pack;
    proof_layout::Proof layout;      // byte layout of this circuit's proofs
    std::vector<void *> allocs;
    // witness-derived regions: overwritten by qpgpu_circuit_scrub, by qpgpu_circuit_free, and after every proof of the
    // host-buffer entry qpgpu_prove. The _dev / batch / pool entries leave them resident between proofs (the next proof
    // overwrites them); include/qpgpu.h says so at qpgpu_circuit_scrub.
    std::vector<std::pair<void *, size_t>> secret_allocs;
    uint32_t max_batch = 1;          // proofs the per-proof workspace below has room for (lockstep batch)
    // setup-time residents
    gl::u64 *d_cs_values = nullptr;
    PolyOracle cs;
    StageTables tab;                 // what stages s5 / s6 read besides the witness: gate table, subgroup / coset tables, switches (prover_stages.hpp)
    gl::u64 *d_poseidon_fast = nullptr;
    // per-proof workspace: every buffer is [max_batch][one proof's size]
    gl::u64 *d_wires_vals = nullptr;
    uint32_t *d_salt_keys = nullptr;     // [max_batch][8] ChaCha20 key words of the zero-knowledge salts
    PolyOracle wires, zs, quot;
    StageWork work;                      // s5 / s6: small tables, folded hash-gate weights, chunk products, Z, accumulators, check result
    gl::u64 *d_zs_vals = nullptr;
    gl::e2 *d_points = nullptr, *d_open = nullptr;
    FriParams fri;
    FriWork fri_work;                // s8..s11 workspace, one allocation
    Stager stage;                    // pinned host staging for the small per-proof tables (no sync on upload)
    bool seed_set = false;
    bool check_witness = false;
    gl::u64 blinding_seed = 0;           // test hook: proof b of the next batch uses the key derived from blinding_seed + b
    WitnessPlan *wplan = nullptr;    // stage s1, built on first use (witness_plan.cpp)
    int witness_wide_rows = -1;      // QPGPU_WITNESS_WIDE_ROWS as read at load: 0 never, 1 always, -1 (unset) the measured threshold (witness.hpp)

    template <class T> int alloc(T **p, size_t count, bool secret = false) {
        void *v = nullptr;
        const size_t bytes = std::max<size_t>(count * sizeof(T), 8);
        hipError_t e = ctx->track_malloc(&v, bytes, secret ? residue::CIRCUIT_WORKSPACE : residue::CIRCUIT_SETUP);
        if (e == hipErrorOutOfMemory) return ctx->fail(QPGPU_ENOMEM, "hipMalloc(circuit): out of device memory");
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMalloc(circuit)");
        allocs.push_back(v);
        if (secret) secret_allocs.push_back({v, bytes});
        *p = (T *)v;
        return QPGPU_OK;
    }
};
