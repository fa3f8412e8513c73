//! qpgpu_backend.rs — the Rust side of the MI355X prover backend: FFI declarations for `libqpgpu.so`, the in-process
//! circuit-pack exporter, the public-input / target maps, and the `prove` hook.
//!
//! STATUS: NOT COMPILED in the build environment of this repository (it has no Rust toolchain and no copy of
//! `qp-plonky2 =1.5.5`). It is written against the plonky2 1.x public API the fork re-exports (field and type names as
//! in upstream `plonk::circuit_data`, `iop::target`, `gates::selectors`); every place that depends on a detail of the
//! fork that this repository could not read is marked `FORK:`. The C side it talks to is tested without it
//! (`tests/`, through the same C ABI from Python and from C).
//!
//! Where it goes: a module of the patched `qp-plonky2` (`src/gpu/mod.rs`), or a small crate next to
//! `wormhole/prover` that depends on `qp-plonky2`. Nothing in the wormhole crates changes their signatures:
//!   * `WormholeProver::new` (wormhole/prover/src/lib.rs:112-140) builds the circuit from source as today and then calls
//!     `GpuCircuit::from_circuit_data(&circuit_data)` once;
//!   * `WormholeProver::prove` (wormhole/prover/src/lib.rs:171-175) calls `gpu.prove(&self.circuit_data, self.partial_witness)`
//!     in place of `self.circuit_data.prove(..)`; same `anyhow::Result<ProofWithPublicInputs<F, C, D>>`;
//!   * the batch provers (wormhole/aggregator/src/private_batch/prover/lib.rs:326-343,
//!     public_batch/prover/lib.rs:301-305) do the same with their own circuit data.
//!
//! Policy note (wormhole/circuit/src/circuit.rs:5-16, wormhole/circuit-builder/src/lib.rs:34-36): the reference never
//! ships prover data as a file ("a poisoned prover artifact cannot exfiltrate witness data through the proof's
//! public-input list"). The pack below is therefore derived IN PROCESS from the circuit the prover has just built and
//! handed to the library as a byte buffer; it is not written to the bins directory. (`QPGPU_ARTIFACT_PROVER_PACK` file
//! names in include/qpgpu_wire.h exist for test fixtures and benchmarks only.)

use anyhow::{anyhow, bail, Result};
use core::ffi::{c_char, c_void};
use plonky2::field::extension::Extendable;
use plonky2::field::polynomial::PolynomialCoeffs;
use plonky2::field::types::PrimeField64;
use plonky2::hash::hash_types::RichField;
use plonky2::iop::target::Target;
use plonky2::iop::witness::{PartialWitness, PartitionWitness};
use plonky2::plonk::circuit_data::{CircuitData, CommonCircuitData, ProverOnlyCircuitData};
use plonky2::plonk::config::GenericConfig;
use plonky2::plonk::proof::ProofWithPublicInputs;

// ---------------------------------------------------------------------------------------------------------------------
// FFI: mirrors include/qpgpu.h (the subset the all-in-one path needs, and the two gate-dependent stages of the stage-level route;
// its commitment / opening / FRI entry points are in INTEGRATION.md section 2a)
// ---------------------------------------------------------------------------------------------------------------------
#[repr(C)] pub struct QpgpuCtx { _p: [u8; 0] }
#[repr(C)] pub struct QpgpuCircuit { _p: [u8; 0] }
#[repr(C)] pub struct QpgpuOracle { _p: [u8; 0] }
#[repr(C)] pub struct QpgpuStagePlan { _p: [u8; 0] }
#[repr(C)] pub struct QpgpuFriSession { _p: [u8; 0] }
#[repr(C)] pub struct QpgpuChallenger { pub sponge_state: [u64; 12], pub input_buffer: [u64; 8], pub output_buffer: [u64; 8], pub input_len: u32, pub output_len: u32 }
#[repr(C)] pub struct QpgpuFriRange { pub oracle: u32, pub first: u32, pub count: u32 }
#[repr(C)] pub struct QpgpuFriBatch { pub point: [u64; 2], pub num_ranges: u32, pub ranges: [QpgpuFriRange; 8] }
#[repr(C)] pub struct QpgpuFriParams { pub rate_bits: u32, pub cap_height: u32, pub proof_of_work_bits: u32, pub num_query_rounds: u32,
                                       pub num_reduction_rounds: u32, pub reduction_arity_bits: [u32; 16] }
// kind 1 (gate): constraint `constraint` of gate `gate` is `value` on `row`; kind 2 (copy): cell (row, wire) holds `value`, the source
// cell of its copy class (row_b, wire_b) holds `value_b`
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct QpgpuWitnessFinding { pub kind: u32, pub gate: u32, pub constraint: u32, pub wire: u32, pub wire_b: u32, pub reserved: u32,
                                 pub row: u64, pub row_b: u64, pub value: u64, pub value_b: u64 }
pub const QPGPU_FINDING_GATE: u32 = 1;
pub const QPGPU_FINDING_COPY: u32 = 2;
pub const QPGPU_STAGE_ERR_CAP: usize = 256;

pub const QPGPU_OK: i32 = 0;
pub const QPGPU_EUNSAT: i32 = -4;

#[link(name = "qpgpu")]
extern "C" {
    pub fn qpgpu_ctx_create(device: i32, out: *mut *mut QpgpuCtx) -> i32;
    pub fn qpgpu_ctx_destroy(ctx: *mut QpgpuCtx);
    pub fn qpgpu_last_error(ctx: *const QpgpuCtx) -> *const c_char;
    pub fn qpgpu_ctx_pci_bus_id(ctx: *const QpgpuCtx, out: *mut c_char, out_len: usize) -> i32;
    pub fn qpgpu_ctx_set_hasher(ctx: *mut QpgpuCtx, kind: i32, params: *const u64, n_words: usize) -> i32;
    pub fn qpgpu_malloc(ctx: *mut QpgpuCtx, bytes: usize, dptr: *mut *mut c_void) -> i32;
    pub fn qpgpu_free(ctx: *mut QpgpuCtx, dptr: *mut c_void) -> i32;
    pub fn qpgpu_free_scrubbed(ctx: *mut QpgpuCtx, dptr: *mut c_void, bytes: usize) -> i32;
    pub fn qpgpu_memcpy_h2d(ctx: *mut QpgpuCtx, dst: *mut c_void, src: *const c_void, bytes: usize) -> i32;
    pub fn qpgpu_circuit_load_batch(ctx: *mut QpgpuCtx, pack: *const u64, n_words: usize, max_batch: u32, out: *mut *mut QpgpuCircuit) -> i32;
    pub fn qpgpu_circuit_free(c: *mut QpgpuCircuit);
    pub fn qpgpu_circuit_scrub(c: *mut QpgpuCircuit) -> i32;
    pub fn qpgpu_circuit_set_witness_check(c: *mut QpgpuCircuit, on: i32) -> i32;
    // After QPGPU_EUNSAT: which gate, which constraints, which cells. Always QPGPU_OK when it could look;
    // `count` findings written (<= cap), GATE findings of the first max_rows (1..=1024) failing rows first, then COPY findings.
    // Findings carry witness values: zeroize `out` like the witness.
    pub fn qpgpu_circuit_explain_witness(c: *mut QpgpuCircuit, wires: *const u64, wires_on_device: i32, public_inputs: *const u64,
                                         max_rows: u32, flags: u32, out: *mut QpgpuWitnessFinding, cap: usize, count: *mut usize,
                                         failing_rows: *mut u64, copy_mismatches: *mut u64) -> i32;
    // host only; QPGPU_EBUFSIZE (-5) = the line was cut at cap
    pub fn qpgpu_witness_finding_format(pack: *const u64, n_words: usize, f: *const QpgpuWitnessFinding, buf: *mut c_char, cap: usize) -> i32;
    pub fn qpgpu_circuit_quotient_pair_info(c: *const QpgpuCircuit, enabled: *mut i32, selected: *mut i32) -> i32;   // introspection
    pub fn qpgpu_proof_size(c: *const QpgpuCircuit) -> usize;
    pub fn qpgpu_prove(c: *mut QpgpuCircuit, wires: *const u64, public_inputs: *const u64, out: *mut u8, out_cap: usize, out_len: *mut usize) -> i32;
    pub fn qpgpu_generate_witness_partial_dev(c: *mut QpgpuCircuit, cells: *const u64, values: *const u64, count: usize,
                                              public_inputs: *const u64, d_wires: *mut u64) -> i32;
    pub fn qpgpu_prove_dev(c: *mut QpgpuCircuit, d_wires: *const u64, public_inputs: *const u64, out: *mut u8, out_cap: usize, out_len: *mut usize) -> i32;
    pub fn qpgpu_prove_batch_dev(c: *mut QpgpuCircuit, d_wires: *const *const u64, batch: u32, public_inputs: *const *const u64,
                                 outs: *const *mut u8, out_cap: usize, out_lens: *mut usize) -> i32;
    pub fn qpgpu_pack_validate(pack: *const u64, n_words: usize, err: *mut c_char) -> i32;
    // include/qpgpu.h — stages s5 / s6 of the stage-level route. `words`: the pack, or the pack without its
    // constants/sigmas value block (header .. circuit_digest, then the trailers); `cs_oracle` must outlive the plan.
    //
    //   let plan = stage_plan_create(ctx, &pack_words[..header_end], o_cs)?;                  // once per circuit
    //   let d_zs = qpgpu_malloc(nch * (1 + npp) * n * 8);  let d_q = qpgpu_malloc(nch * qdf * n * 8);
    //   qpgpu_stage_partial_products(plan, wires.as_ptr(), 0, betas, gammas, d_zs)            // all_wires_permutation_partial_products
    //   let o_zs = qpgpu_oracle_commit(ctx, d_zs, nch * (1 + npp), .., VALUES | DEVICE_INPUT [| BLINDING], seed, 2)
    //   match qpgpu_stage_quotient(plan, o_wires, o_zs, betas, gammas, alphas, pi_hash, d_q)  // compute_quotient_polys
    //       { QPGPU_EUNSAT => bail!("{}", last_error(ctx)), .. }                              // names the violated row
    //   let o_q  = qpgpu_oracle_commit(ctx, d_q, nch * qdf, .., COEFFS | DEVICE_INPUT [| BLINDING], seed, 3)
    //   .. qpgpu_free_scrubbed(ctx, d_zs, ..); qpgpu_free_scrubbed(ctx, d_q, ..);             // both held witness-derived values
    //   qpgpu_stage_plan_free(plan) BEFORE qpgpu_oracle_free(o_cs)
    pub fn qpgpu_stage_plan_create(ctx: *mut QpgpuCtx, words: *const u64, n_words: usize, cs_oracle: *const QpgpuOracle,
                                   out: *mut *mut QpgpuStagePlan, err: *mut c_char) -> i32;
    pub fn qpgpu_stage_plan_free(plan: *mut QpgpuStagePlan);
    pub fn qpgpu_stage_plan_info(plan: *const QpgpuStagePlan, degree_bits: *mut u32, num_challenges: *mut u32, num_partial_products: *mut u32,
                                 quotient_degree_factor: *mut u32, fused_selected: *mut i32) -> i32;
    pub fn qpgpu_stage_partial_products(plan: *mut QpgpuStagePlan, wires: *const u64, wires_on_device: i32, betas: *const u64,
                                        gammas: *const u64, d_out: *mut u64) -> i32;
    pub fn qpgpu_stage_quotient(plan: *mut QpgpuStagePlan, wires_oracle: *const QpgpuOracle, zs_pp_oracle: *const QpgpuOracle,
                                betas: *const u64, gammas: *const u64, alphas: *const u64, public_inputs_hash: *const u64,
                                d_out: *mut u64) -> i32;
    // include/qpgpu.h — stages s8..s11 one step at a time: PolynomialBatch::prove_openings with the
    // challenger, the proof-of-work rule and the query indices kept in Rust. qpgpu_fri_prove is the one-call form; use it unless the
    // fork's prove_openings differs from what DESIGN.md section 9 lists. `Oracle::open` and `FriSession` below wrap these.
    pub fn qpgpu_oracle_leaf_width(o: *const QpgpuOracle) -> usize;
    // one commitment over n_ctx contexts (one per device; ctxs[0] is the home context): the leaves are split by cosets, cap / eval /
    // open / qpgpu_fri_prove on the home context answer as for any oracle, with the same bytes
    pub fn qpgpu_oracle_commit_sharded(ctxs: *const *mut QpgpuCtx, n_ctx: u32, polys: *const u64, num_polys: u32, degree_bits: u32, rate_bits: u32,
                                       cap_height: u32, flags: u32, blinding_seed: u64, blinding_stream: u32, out: *mut *mut QpgpuOracle) -> i32;
    pub fn qpgpu_oracle_shards(o: *const QpgpuOracle) -> u32;
    pub fn qpgpu_oracle_shard_range(o: *const QpgpuOracle, shard: u32, first_leaf: *mut u64, num_leaves: *mut u64) -> i32;
    pub fn qpgpu_oracle_shard_device_ptrs(o: *const QpgpuOracle, shard: u32, d_lde: *mut *const u64, d_digests: *mut *const u64) -> i32;
    pub fn qpgpu_oracle_open(o: *mut QpgpuOracle, indices: *const u64, n: usize, rows_out: *mut u64, paths_out: *mut u64) -> i32;
    pub fn qpgpu_fri_begin(ctx: *mut QpgpuCtx, oracles: *const *mut QpgpuOracle, n: u32, batches: *const QpgpuFriBatch, n_batches: u32,
                           params: *const QpgpuFriParams, alpha: *const u64, out: *mut *mut QpgpuFriSession) -> i32;
    pub fn qpgpu_fri_round_commit(s: *mut QpgpuFriSession, cap_out: *mut u64, cap_words: usize) -> i32;
    pub fn qpgpu_fri_round_fold(s: *mut QpgpuFriSession, beta: *const u64) -> i32;
    pub fn qpgpu_fri_final_poly(s: *mut QpgpuFriSession, out: *mut u64, out_words: usize, num_coeffs: *mut usize) -> i32;
    pub fn qpgpu_fri_query_size(s: *const QpgpuFriSession) -> usize;
    pub fn qpgpu_fri_open(s: *mut QpgpuFriSession, indices: *const u64, n: usize, out: *mut u8, out_cap: usize, out_len: *mut usize) -> i32;
    pub fn qpgpu_fri_session_free(s: *mut QpgpuFriSession);
    pub fn qpgpu_fri_grind(ctx: *mut QpgpuCtx, c: *const QpgpuChallenger, proof_of_work_bits: u32, nonce_out: *mut u64) -> i32;
    // include/qpgpu.h — the stage route for a lockstep batch: one call per stage for `batch` proofs of one circuit (a level of
    // leaves), `batch` transcripts kept in Rust; arrays are [batch][..], proof b first ("a level of
    // leaves"). An oracle made by qpgpu_oracle_commit_batch holds all the proofs' columns; the constants/sigmas oracle holds one proof
    // and is shared. `Oracle::{eval_batch, open_batch}`, `FriSession::begin_batch` and `fri_grind_batch` below wrap these.
    pub fn qpgpu_oracle_commit_batch(ctx: *mut QpgpuCtx, polys: *const *const u64, batch: u32, num_polys: u32, degree_bits: u32, rate_bits: u32,
                                     cap_height: u32, flags: u32, blinding_seed: u64, blinding_stream: u32, out: *mut *mut QpgpuOracle) -> i32;
    pub fn qpgpu_oracle_batch(o: *const QpgpuOracle) -> u32;
    pub fn qpgpu_oracle_strides(o: *const QpgpuOracle, coeffs: *mut u64, lde: *mut u64, digests: *mut u64) -> i32;
    pub fn qpgpu_oracle_eval_batch(o: *mut QpgpuOracle, points: *const u64, first: u32, count: u32, out: *mut u64) -> i32;
    pub fn qpgpu_oracle_open_batch(o: *mut QpgpuOracle, indices: *const u64, n: usize, rows_out: *mut u64, paths_out: *mut u64) -> i32;
    pub fn qpgpu_stage_plan_create_batch(ctx: *mut QpgpuCtx, words: *const u64, n_words: usize, cs_oracle: *const QpgpuOracle, max_batch: u32,
                                         out: *mut *mut QpgpuStagePlan, err: *mut c_char) -> i32;
    pub fn qpgpu_stage_plan_max_batch(plan: *const QpgpuStagePlan) -> u32;
    pub fn qpgpu_stage_plan_create_sharded(ctx: *mut QpgpuCtx, words: *const u64, n_words: usize, cs_oracle: *const QpgpuOracle,
                                           out: *mut *mut QpgpuStagePlan, err: *mut c_char) -> i32;
    pub fn qpgpu_stage_plan_shards(plan: *const QpgpuStagePlan) -> u32;
    pub fn qpgpu_stage_partial_products_batch(plan: *mut QpgpuStagePlan, wires: *const *const u64, batch: u32, wires_on_device: i32,
                                              betas: *const u64, gammas: *const u64, d_out: *mut u64) -> i32;
    pub fn qpgpu_stage_quotient_batch(plan: *mut QpgpuStagePlan, wires_oracle: *const QpgpuOracle, zs_pp_oracle: *const QpgpuOracle, batch: u32,
                                      betas: *const u64, gammas: *const u64, alphas: *const u64, public_inputs_hashes: *const u64,
                                      d_out: *mut u64) -> i32;
    pub fn qpgpu_fri_prove_batch(ctx: *mut QpgpuCtx, oracles: *const *mut QpgpuOracle, n: u32, batches: *const QpgpuFriBatch, n_batches: u32,
                                 points: *const u64, batch: u32, params: *const QpgpuFriParams, challengers: *mut QpgpuChallenger,
                                 outs: *const *mut u8, out_cap: usize, out_lens: *mut usize) -> i32;
    pub fn qpgpu_fri_begin_batch(ctx: *mut QpgpuCtx, oracles: *const *mut QpgpuOracle, n: u32, batches: *const QpgpuFriBatch, n_batches: u32,
                                 points: *const u64, batch: u32, params: *const QpgpuFriParams, alphas: *const u64,
                                 out: *mut *mut QpgpuFriSession) -> i32;
    pub fn qpgpu_fri_session_batch(s: *const QpgpuFriSession) -> u32;
    pub fn qpgpu_fri_grind_batch(ctx: *mut QpgpuCtx, cs: *const QpgpuChallenger, batch: u32, proof_of_work_bits: u32, nonces_out: *mut u64) -> i32;
    pub fn qpgpu_circuit_constants_sigmas_cap(c: *const QpgpuCircuit, out: *mut u64, out_words: usize) -> i32;
    // include/qpgpu_verify.h — host-side verification of the bytes the GPU produced (debug self-check; production keeps
    // plonky2's own `VerifierCircuitData::verify`, which is what consumers of the proof run anyway)
    pub fn qpgpu_verifier_create(pack: *const u64, n_words: usize, cs_cap: *const u64, cap_words: usize, hasher_kind: i32,
                                 hasher_params: *const u64, n_params: usize, out: *mut *mut QpgpuVerifier, err: *mut c_char) -> i32;
    pub fn qpgpu_verifier_free(v: *mut QpgpuVerifier);
    pub fn qpgpu_verifier_verify(v: *const QpgpuVerifier, proof: *const u8, len: usize, err: *mut c_char) -> i32;
    // the query rounds of a batch of proofs on ctx's GPU; results / err as qpgpu_verifier_verify_many, reasons: count * 200 bytes or null
    pub fn qpgpu_verifier_verify_many_device(v: *const QpgpuVerifier, ctx: *mut QpgpuCtx, proofs: *const *const u8, lens: *const usize, count: usize,
                                             threads: u32, results: *mut i32, reasons: *mut c_char, err: *mut c_char) -> i32;
    // the same with flags: 1 (QPGPU_VERIFY_HEAD_ON_DEVICE) runs the transcript, proof of work and quotient identity on the GPU too
    pub fn qpgpu_verifier_verify_many_device_ex(v: *const QpgpuVerifier, ctx: *mut QpgpuCtx, proofs: *const *const u8, lens: *const usize, count: usize,
                                                threads: u32, flags: u32, results: *mut i32, reasons: *mut c_char, err: *mut c_char) -> i32;
    // include/qpgpu_verify.h — fri::verifier::verify_fri_proof on its own, the counterpart of qpgpu_fri_prove: the Rust side keeps its
    // verifier head (transcript, gates at zeta) and hands over all the hashing of a verification. An instance is the oracles' shapes,
    // the opening batches and the FRI parameters; no circuit pack is involved. caps: [num_oracles] pointers; points [num_batches][2];
    // openings [num_openings][2], batch by batch, range by range. _many_device: arrays [count][..] (points [num_batches][count][2]),
    // cap_counts[o] 1 (shared) or count; results / reasons (count * 200 bytes or null) / err as `count` calls of qpgpu_fri_verify.
    pub fn qpgpu_fri_verifier_create(inst: *const QpgpuFriInstance, hasher_kind: i32, hasher_params: *const u64, n_params: usize,
                                     out: *mut *mut QpgpuFriVerifier, err: *mut c_char) -> i32;
    pub fn qpgpu_fri_verifier_free(v: *mut QpgpuFriVerifier);
    pub fn qpgpu_fri_verifier_proof_size(v: *const QpgpuFriVerifier) -> usize;
    pub fn qpgpu_fri_verifier_num_openings(v: *const QpgpuFriVerifier) -> usize;
    // Challenger::fri_challenges; *c is advanced in place. betas [rounds][2], indices [num_query_rounds]
    pub fn qpgpu_fri_verifier_challenges(v: *const QpgpuFriVerifier, c: *mut QpgpuChallenger, proof: *const u8, len: usize, alpha: *mut u64,
                                         betas: *mut u64, pow_response: *mut u64, indices: *mut u64, err: *mut c_char) -> i32;
    pub fn qpgpu_fri_verify(v: *const QpgpuFriVerifier, caps: *const *const u64, points: *const u64, openings: *const u64, alpha: *const u64,
                            betas: *const u64, pow_response: u64, indices: *const u64, proof: *const u8, len: usize, err: *mut c_char) -> i32;
    pub fn qpgpu_fri_verify_many_device(v: *const QpgpuFriVerifier, ctx: *mut QpgpuCtx, count: usize, caps: *const *const u64,
                                        cap_counts: *const u32, points: *const u64, openings: *const u64, alphas: *const u64, betas: *const u64,
                                        pow_responses: *const u64, indices: *const u64, proofs: *const *const u8, lens: *const usize,
                                        results: *mut i32, reasons: *mut c_char, err: *mut c_char) -> i32;
    // include/qpgpu.h — the proving pool over one GPU or several: one queue, a worker set per device,
    // proofs written into the caller's host buffers
    pub fn qpgpu_pool_create_multi(devices: *const i32, n_devices: u32, pack: *const u64, n_words: usize, workers_per_device: u32,
                                   max_batch: u32, flags: u32, out: *mut *mut QpgpuPool) -> i32;
    pub fn qpgpu_pool_destroy(p: *mut QpgpuPool);
    pub fn qpgpu_pool_proof_size(p: *const QpgpuPool) -> usize;
    pub fn qpgpu_pool_last_error(p: *const QpgpuPool) -> *const c_char;
    pub fn qpgpu_pool_submit_host(p: *mut QpgpuPool, wires: *const u64, public_inputs: *const u64, out: *mut u8, out_cap: usize, ticket: *mut u64) -> i32;
    pub fn qpgpu_pool_set_partial_cells(p: *mut QpgpuPool, cells: *const u64, count: usize) -> i32;
    pub fn qpgpu_pool_set_partial_cells_blinded(p: *mut QpgpuPool, cells: *const u64, count: usize, n_blinding: usize) -> i32;
    pub fn qpgpu_pool_submit_partial(p: *mut QpgpuPool, values: *const u64, public_inputs: *const u64, out: *mut u8, out_cap: usize, ticket: *mut u64) -> i32;
    pub fn qpgpu_pool_wait(p: *mut QpgpuPool, ticket: u64, out_len: *mut usize) -> i32;
    // include/qpgpu.h, include/qpgpu_batch.h — zero-knowledge circuits (the private-batch layer): the blinding rows' random wires are
    // the last `n_blinding` cells of the assignment list and are drawn on the device, one ChaCha20 key per witness (seeds = null:
    // operating-system entropy); qpgpu_random_field_elements is the host-side form
    pub fn qpgpu_generate_witness_partial_batch_blinded_dev(c: *mut QpgpuCircuit, cells: *const u64, count: usize, n_blinding: usize, values: *const u64,
                                                            seeds: *const u8, public_inputs: *const u64, batch: u32, d_wires: *mut u64, status: *mut i32) -> i32;
    pub fn qpgpu_random_field_elements(seed32: *const u8, out: *mut u64, n: usize, err: *mut c_char) -> i32;
    // with stage s1 on the device the public inputs are read out of the device witness, the way `prove` reads them out of the
    // partition witness: pass public_inputs = null to the generate_witness_partial* calls, then this, then qpgpu_prove*_dev
    pub fn qpgpu_circuit_gate_rows(c: *const QpgpuCircuit, gate_type: u32, rows_out: *mut u32, cap: usize, count: *mut usize) -> i32;   // introspection
    pub fn qpgpu_witness_public_inputs_dev(c: *mut QpgpuCircuit, d_wires: *const u64, batch: u32, public_inputs_out: *mut u64) -> i32;
    // include/qpgpu_leaf.h, include/qpgpu_batch.h — the circuits built by the library itself: only for
    // deployments that take BOTH prover and verifier data from it; with exported packs of the fork's own circuits these are not used
    pub fn qpgpu_leaf_circuit_build(fragment: u32, min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, pack_out: *mut u64, pack_cap_words: usize,
                                    pack_words: *mut usize, target_map_out: *mut u64, info_out: *mut u64, err: *mut c_char) -> i32;
    // WormholeProver::new(config) (wormhole/prover/src/lib.rs:137-149): the leaf circuit under a caller's CircuitConfig; cfg = null is
    // wormhole_leaf_circuit_config(). A zero-knowledge config (wormhole_private_batch_circuit_config: the bench's prover_create_proof_zk)
    // reports CircuitBuilder::blind's random wires in blinding_cells_out: append them LAST to the cell list and pass their count as
    // n_blinding to qpgpu_pool_set_partial_cells_blinded / qpgpu_generate_witness_partial_batch_blinded_dev. err: 400 bytes.
    pub fn qpgpu_wormhole_circuit_config(level: i32, out: *mut QpgpuCircuitConfig) -> i32;
    pub fn qpgpu_validate_circuit_config(cfg: *const QpgpuCircuitConfig, err: *mut c_char) -> i32;
    pub fn qpgpu_leaf_circuit_build_cfg(fragment: u32, min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, cfg: *const QpgpuCircuitConfig,
                                        pack_out: *mut u64, pack_cap_words: usize, pack_words: *mut usize, target_map_out: *mut u64, info_out: *mut u64,
                                        blinding_cells_out: *mut u64, blinding_cap: usize, blinding_count: *mut usize, err: *mut c_char) -> i32;
    pub fn qpgpu_leaf_circuit_hash_hint_cells_cfg(min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, cfg: *const QpgpuCircuitConfig,
                                                  cells_out: *mut u64, cap: usize, count: *mut usize, err: *mut c_char) -> i32;
    // the density-matched leaf (a measurement and test object, NOT a protocol object): `copies` independent statements of the leaf circuit in
    // one trace, copy 0's 21 targets public, the others private; target_map_out has copies * QPGPU_LT_COUNT words, copy-major. copies = 1
    // is qpgpu_leaf_circuit_build_cfg's full circuit word for word.
    pub fn qpgpu_leaf_circuit_build_dense(copies: u32, min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, cfg: *const QpgpuCircuitConfig,
                                          pack_out: *mut u64, pack_cap_words: usize, pack_words: *mut usize, target_map_out: *mut u64, info_out: *mut u64,
                                          blinding_cells_out: *mut u64, blinding_cap: usize, blinding_count: *mut usize, err: *mut c_char) -> i32;
    pub fn qpgpu_leaf_circuit_hash_hint_cells_dense(copies: u32, min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, cfg: *const QpgpuCircuitConfig,
                                                    cells_out: *mut u64, cap: usize, count: *mut usize, err: *mut c_char) -> i32;
    // ins: `copies` pointers to qpgpu_leaf_inputs (they may repeat); the public inputs are those of ins[0]
    pub fn qpgpu_leaf_commit_dense(ins: *const *const c_void, copies: u32, target_map: *const u64, cells_out: *mut u64, values_out: *mut u64, cap: usize,
                                   count: *mut usize, public_inputs_out: *mut u64, err: *mut c_char) -> i32;
    // optional: the leaf circuit's hash-chain states as extra assignments (796 cells / values appended to qpgpu_leaf_commit's) — the
    // same witness in 14 dependency levels instead of 120 (one proof 4.6 -> 3.7 ms); a hint that disagrees is QPGPU_EUNSAT
    pub fn qpgpu_leaf_circuit_hash_hint_cells(min_degree_bits: u32, inner_hasher: i32, p2_layout: *const u64, cells_out: *mut u64, cap: usize,
                                              count: *mut usize, err: *mut c_char) -> i32;
    pub fn qpgpu_leaf_hash_hints(inputs: *const c_void, values_out: *mut u64, cap: usize, count: *mut usize, err: *mut c_char) -> i32;
    // include/qpgpu_leaf.h — the chain's 4-ary ZK Merkle tree of one block, built and kept on the device:
    // leaves = count x 32 bytes of leaf hashes, or count QpgpuZkLeaf records with flags = QPGPU_ZK_TREE_FROM_TRANSFERS; depth 0 = the
    // smallest valid depth. qpgpu_zk_tree_open fills zk_merkle_siblings / zk_merkle_positions of n leaves in one call
    // (siblings_out: n x depth x 3 x 32 bytes, positions_out: n x depth bytes). err: 160 bytes. A tree is freed before its context.
    pub fn qpgpu_zk_leaf_hash_batch(ctx: *mut QpgpuCtx, leaves: *const QpgpuZkLeaf, count: usize, out: *mut u8) -> i32;
    pub fn qpgpu_zk_tree_build(ctx: *mut QpgpuCtx, leaves: *const c_void, count: usize, depth: u32, flags: u32, out: *mut *mut QpgpuZkTree,
                               err: *mut c_char) -> i32;
    pub fn qpgpu_zk_tree_free(t: *mut QpgpuZkTree);
    pub fn qpgpu_zk_tree_depth(t: *const QpgpuZkTree) -> u32;
    pub fn qpgpu_zk_tree_leaf_count(t: *const QpgpuZkTree) -> usize;
    pub fn qpgpu_zk_tree_root(t: *const QpgpuZkTree, out: *mut u8) -> i32;
    pub fn qpgpu_zk_tree_read_level(t: *const QpgpuZkTree, level: u32, first: usize, n: usize, out: *mut u8) -> i32;
    pub fn qpgpu_zk_tree_open(t: *const QpgpuZkTree, indices: *const u64, n: usize, siblings_out: *mut u8, positions_out: *mut u8) -> i32;
    // the same tree with room to grow: append a block's leaves (only their ancestors are rehashed), keep the 528-byte snapshot per block,
    // open paths against the tree as it stood at a snapshot (the root is snap.last[depth - 1])
    pub fn qpgpu_zk_tree_build_reserved(ctx: *mut QpgpuCtx, leaves: *const c_void, count: usize, capacity: usize, depth: u32, flags: u32,
                                        out: *mut *mut QpgpuZkTree, err: *mut c_char) -> i32;
    pub fn qpgpu_zk_tree_capacity(t: *const QpgpuZkTree) -> usize;
    pub fn qpgpu_zk_tree_append(t: *mut QpgpuZkTree, leaves: *const c_void, k: usize, flags: u32, snap_out: *mut QpgpuZkSnapshot, err: *mut c_char) -> i32;
    pub fn qpgpu_zk_tree_snapshot(t: *const QpgpuZkTree, out: *mut QpgpuZkSnapshot) -> i32;
    pub fn qpgpu_zk_tree_open_at(t: *const QpgpuZkTree, snap: *const QpgpuZkSnapshot, indices: *const u64, n: usize, siblings_out: *mut u8,
                                 positions_out: *mut u8) -> i32;
    // no snapshot kept: the snapshots at earlier counts derived from the resident nodes, a kept one checked against the tree, paths
    // opened at a count per path (roots_out: n x 32 bytes, may be null), and a reorg back to the first n leaves
    pub fn qpgpu_zk_tree_snapshots_at(t: *const QpgpuZkTree, counts: *const u64, m: usize, out: *mut QpgpuZkSnapshot) -> i32;
    pub fn qpgpu_zk_tree_snapshot_check(t: *const QpgpuZkTree, snap: *const QpgpuZkSnapshot) -> i32;
    pub fn qpgpu_zk_tree_open_at_counts(t: *const QpgpuZkTree, counts: *const u64, indices: *const u64, n: usize, siblings_out: *mut u8,
                                        positions_out: *mut u8, roots_out: *mut u8) -> i32;
    pub fn qpgpu_zk_tree_truncate(t: *mut QpgpuZkTree, n: usize, snap_out: *mut QpgpuZkSnapshot, err: *mut c_char) -> i32;
    pub fn qpgpu_wrapper_circuit_build(inner_pack: *const u64, inner_words: usize, inner_cs_cap: *const u64, cap_words: usize, num_proofs: u32,
                                       num_routed_wires: u32, min_degree_bits: u32, inner_hasher: i32, flags: u32, pack_out: *mut u64, pack_cap_words: usize,
                                       pack_words: *mut usize, target_map_out: *mut u64, map_cap: usize, map_count: *mut usize, info_out: *mut u64,
                                       err: *mut c_char) -> i32;
    // PrivateBatchCircuit::new(config, ..) / PublicBatchCircuit::new(config, ..): the same circuit under a caller's CircuitConfig (cfg null:
    // the entry above word for word). With cfg: num_routed_wires = 0 and no QPGPU_WRAPPER_ZERO_KNOWLEDGE (the config carries both),
    // info_out has QPGPU_WRAPPER_CIRCUIT_INFO_WORDS_CFG (16) words, err QPGPU_CONFIG_ERR_CAP (400) bytes.
    pub fn qpgpu_wrapper_circuit_build_cfg(inner_pack: *const u64, inner_words: usize, inner_cs_cap: *const u64, cap_words: usize, num_proofs: u32,
                                           num_routed_wires: u32, min_degree_bits: u32, inner_hasher: i32, flags: u32, cfg: *const QpgpuCircuitConfig,
                                           pack_out: *mut u64, pack_cap_words: usize, pack_words: *mut usize, target_map_out: *mut u64, map_cap: usize,
                                           map_count: *mut usize, info_out: *mut u64, err: *mut c_char) -> i32;
    // AggConfigArgs::validate / ::build (wormhole/memprof/src/config.rs): the sweep knobs on top of the production private-batch config
    pub fn qpgpu_agg_config_validate(args: *const QpgpuAggConfigArgs, err: *mut c_char) -> i32;
    pub fn qpgpu_agg_config_build(args: *const QpgpuAggConfigArgs, out: *mut QpgpuCircuitConfig) -> i32;
}
/// qpgpu_agg_config_args (include/qpgpu_wire.h): a knob counts only when its QPGPU_AGG_HAS_* bit is set in `present`
/// (zk_mode 1, rate_bits 2, cap_height 4, num_wires 8, num_routed_wires 16, max_quotient_degree_factor 32, num_query_rounds 64,
/// security_bits 128, num_challenges 256); zk_mode: 0 rowblinding, 1 disabled
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct QpgpuAggConfigArgs {
    pub present: u32, pub zk_mode: i32,
    pub rate_bits: u64, pub cap_height: u64, pub num_wires: u64, pub num_routed_wires: u64, pub max_quotient_degree_factor: u64,
    pub num_query_rounds: u64, pub security_bits: u64, pub num_challenges: u64,
    pub allow_weakening_security: i32,
}
#[repr(C)] pub struct QpgpuZkTree { _p: [u8; 0] }
/// qpgpu_zk_leaf (include/qpgpu_leaf.h): what a leaf of the ZK tree hashes; 48 bytes
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct QpgpuZkLeaf { pub to_account: [u8; 32], pub transfer_count: u64, pub asset_id: u32, pub input_amount: u32 }
pub const QPGPU_ZK_TREE_FROM_TRANSFERS: u32 = 1;
/// qpgpu_zk_snapshot (include/qpgpu_leaf.h): the tree as it stood at `count` leaves, kept per block; 528 bytes.
/// last[l - 1] = the last node of level l, l = 1 ..= depth, the rest zero; the root is last[depth - 1]
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct QpgpuZkSnapshot { pub count: u64, pub depth: u32, pub reserved: u32, pub last: [[u8; 32]; 16] }
/// qpgpu_circuit_config (include/qpgpu_wire.h): plonky2's CircuitConfig + FriConfig (ConstantArityBits reduction) as plain data
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct QpgpuCircuitConfig {
    pub num_wires: u64, pub num_routed_wires: u64, pub num_constants: u64, pub security_bits: u64, pub num_challenges: u64, pub max_quotient_degree_factor: u64,
    pub use_base_arithmetic_gate: i32, pub zero_knowledge: i32,
    pub rate_bits: u64, pub cap_height: u64, pub proof_of_work_bits: u64, pub num_query_rounds: u64,
    pub reduction_arity_bits: u64, pub reduction_final_poly_bits: u64,
}
pub const QPGPU_LEVEL_LEAF: i32 = 0;
pub const QPGPU_LEVEL_PRIVATE_BATCH: i32 = 1;
pub const QPGPU_LEVEL_PUBLIC_BATCH: i32 = 2;
#[repr(C)] pub struct QpgpuVerifier { _private: [u8; 0] }
#[repr(C)] pub struct QpgpuFriVerifier { _private: [u8; 0] }
#[repr(C)] pub struct QpgpuFriOracleShape { pub num_polys: u32, pub blinded: u32 }
#[repr(C)] pub struct QpgpuFriInstance { pub degree_bits: u32, pub num_oracles: u32, pub oracles: *const QpgpuFriOracleShape,
                                         pub num_batches: u32, pub batches: *const QpgpuFriBatch, pub params: QpgpuFriParams }
#[repr(C)] pub struct QpgpuPool { _private: [u8; 0] }
pub const QPGPU_POOL_HOST_WITNESS: u32 = 1;

/// All the GPUs of a node behind one handle: what `ProvingContext` (wormhole/aggregator/src/aggregator.rs:187-227) or a miner's
/// leaf-proving loop holds instead of a `ProverCircuitData`. Proofs are independent, so there is no collective: any worker of any
/// device takes the next job and writes the proof bytes into the caller's buffer.
pub struct GpuProvingPool { pool: *mut QpgpuPool, proof_size: usize }
unsafe impl Send for GpuProvingPool {}
unsafe impl Sync for GpuProvingPool {}      // submit / wait lock inside the library

impl GpuProvingPool {
    /// `devices`: HIP device ordinals, e.g. `&[0, 1, 2, 3, 4, 5, 6, 7]`; three workers of 32 lockstep proofs per device saturate one.
    pub fn new(pack: &[u64], devices: &[i32], workers_per_device: u32, lockstep: u32) -> Result<Self> {
        let mut pool = std::ptr::null_mut();
        let rc = unsafe { qpgpu_pool_create_multi(devices.as_ptr(), devices.len() as u32, pack.as_ptr(), pack.len(), workers_per_device, lockstep,
                                                  QPGPU_POOL_HOST_WITNESS, &mut pool) };
        if rc != 0 { bail!("qpgpu_pool_create_multi failed ({rc})") }
        Ok(Self { pool, proof_size: unsafe { qpgpu_pool_proof_size(pool) } })
    }
    /// `full_witness`: the wire matrix `generate_partial_witness(..).full_witness()` holds (num_wires x n, column-major, canonical u64).
    /// Returns a ticket; the matrix and `out` must outlive `wait`.
    pub fn submit(&self, full_witness: &[u64], public_inputs: &[u64], out: &mut [u8]) -> Result<u64> {
        let mut ticket = 0u64;
        let rc = unsafe { qpgpu_pool_submit_host(self.pool, full_witness.as_ptr(), public_inputs.as_ptr(), out.as_mut_ptr(), out.len(), &mut ticket) };
        if rc != 0 { bail!("qpgpu_pool_submit_host: {}", unsafe { std::ffi::CStr::from_ptr(qpgpu_pool_last_error(self.pool)).to_string_lossy() }) }
        Ok(ticket)
    }
    /// Blocks until that proof is written; an unsatisfied witness fails its own ticket only ("Failed to prove: ...").
    pub fn wait(&self, ticket: u64) -> Result<usize> {
        let mut len = 0usize;
        let rc = unsafe { qpgpu_pool_wait(self.pool, ticket, &mut len) };
        if rc != 0 { bail!("Failed to prove: {}", unsafe { std::ffi::CStr::from_ptr(qpgpu_pool_last_error(self.pool)).to_string_lossy() }) }
        Ok(len)
    }
    pub fn proof_size(&self) -> usize { self.proof_size }

    /// A circuit whose witness is a PartialWitness (stage s1 on the device too): `cells` is the assignment list resolved once —
    /// for an exported circuit the wire cells of the targets `fill_witness` / `fill_private_batch_witness` set, in their order;
    /// the last `n_blinding` of them are the `RandomValueGenerator` targets of a zero-knowledge circuit (`CircuitBuilder::blind`),
    /// which the device draws per proof.
    pub fn set_partial_cells(&self, cells: &[u64], n_blinding: usize) -> Result<()> {
        let rc = unsafe { qpgpu_pool_set_partial_cells_blinded(self.pool, cells.as_ptr(), cells.len(), n_blinding) };
        if rc != 0 { bail!("qpgpu_pool_set_partial_cells: {}", unsafe { std::ffi::CStr::from_ptr(qpgpu_pool_last_error(self.pool)).to_string_lossy() }) }
        Ok(())
    }
    /// `values`: one per cell of the list, without the blinding ones. `public_inputs = None`: what `ProverCircuitData::prove` does —
    /// they are read out of the generated witness (the batch layers, whose public inputs the circuit computes) and come back as the
    /// last `num_public_inputs` words of the proof.
    pub fn submit_partial(&self, values: &[u64], public_inputs: Option<&[u64]>, out: &mut [u8]) -> Result<u64> {
        let mut ticket = 0u64;
        let pis = public_inputs.map_or(std::ptr::null(), |p| p.as_ptr());
        let rc = unsafe { qpgpu_pool_submit_partial(self.pool, values.as_ptr(), pis, out.as_mut_ptr(), out.len(), &mut ticket) };
        if rc != 0 { bail!("qpgpu_pool_submit_partial: {}", unsafe { std::ffi::CStr::from_ptr(qpgpu_pool_last_error(self.pool)).to_string_lossy() }) }
        Ok(ticket)
    }
}
impl Drop for GpuProvingPool { fn drop(&mut self) { unsafe { qpgpu_pool_destroy(self.pool) } } }

fn last_error(ctx: *const QpgpuCtx) -> String {
    unsafe { std::ffi::CStr::from_ptr(qpgpu_last_error(ctx)).to_string_lossy().into_owned() }
}

// ---------------------------------------------------------------------------------------------------------------------
// Circuit pack ("QPCP1", qp-zk-circuits_amd/csrc/circuit.hpp): everything `prove` reads after witness generation
// ---------------------------------------------------------------------------------------------------------------------
const QPCP_MAGIC: u64 = 0x0000_0031_5043_5051;
const PUBI_MAGIC: u64 = 0x0000_0031_4942_5550;
const P2GL_MAGIC: u64 = 0x0000_0031_4C47_3250;     // "P2GL1": wire layout of the Poseidon2 gate (csrc/circuit.hpp)
const P2_NO_SWAP: u64 = 0xFFFF_FFFF;

/// Gate id string -> (type code, param0, param1, param2) of the pack format. An id this table does not know aborts the
/// export: the backend refuses unknown gates rather than skipping their constraints.
fn gate_code(id: &str) -> Result<(u64, u64, u64, u64)> {
    // ids are the `Debug` renderings plonky2 uses as gate identity, e.g. "ArithmeticGate { num_ops: 20 }"
    let num = |key: &str| -> Result<u64> {
        let at = id.find(key).ok_or_else(|| anyhow!("gate id `{id}` has no `{key}`"))? + key.len();
        let digits: String = id[at..].chars().skip_while(|c| !c.is_ascii_digit()).take_while(|c| c.is_ascii_digit()).collect();
        digits.parse::<u64>().map_err(|_| anyhow!("gate id `{id}`: no number after `{key}`"))
    };
    Ok(if id.starts_with("NoopGate") { (0, 0, 0, 0) }
    else if id.starts_with("ConstantGate") { (1, num("num_consts")?, 0, 0) }
    else if id.starts_with("PublicInputGate") { (2, 0, 0, 0) }
    else if id.starts_with("ArithmeticGate") { (3, num("num_ops")?, 0, 0) }
    else if id.starts_with("PoseidonGate") { (4, 0, 0, 0) }
    else if id.starts_with("BaseSumGate") {
        if !id.ends_with("Base: 2") { bail!("only BaseSumGate<2> is implemented on the device (`{id}`)") }
        (5, num("num_limbs")?, 2, 0)
    }
    else if id.starts_with("ArithmeticExtensionGate") { (6, num("num_ops")?, 0, 0) }
    else if id.starts_with("MulExtensionGate") { (7, num("num_ops")?, 0, 0) }
    else if id.starts_with("ReducingGate") { (8, num("num_coeffs")?, 0, 0) }
    else if id.starts_with("ReducingExtensionGate") { (9, num("num_coeffs")?, 0, 0) }
    else if id.starts_with("RandomAccessGate") {
        // num_extra_constants = min(num_constants, num_routed_wires - (2 + 2^bits) * num_copies): derived by the caller
        (10, num("bits")?, num("num_copies")?, num("num_extra_constants").unwrap_or(0))
    }
    else if id.starts_with("ExponentiationGate") { (11, num("num_power_bits")?, 0, 0) }
    else if id.starts_with("PoseidonMdsGate") { (12, 0, 0, 0) }
    else if id.starts_with("CosetInterpolationGate") { (13, num("subgroup_bits")?, num("degree")?, 0) }
    // FORK: the qp fork's Poseidon2 gate (wormhole/circuit reaches it through `hash_n_to_hash_no_pad_p2::<Poseidon2Hash>`).
    // The device evaluates it as gate type 14 with the wire layout this exporter writes into the "P2GL1" trailer
    // (`poseidon2_gate_layout` below); adjust the prefix if the fork's `Gate::id()` renders differently.
    else if id.starts_with("Poseidon2Gate") { (14, 0, 0, 0) }
    else { bail!("gate `{id}` is not implemented by the MI355X backend") })
}

/// The ten words of the "P2GL1" trailer, read off the fork's gate: first input wire, first output wire, swap wire (or
/// P2_NO_SWAP), first delta wire, first S-box-input wire of the first half's full rounds, of the 22 partial rounds, of the
/// second half's full rounds, whether round 0 of the first half is recorded too, constraint order (0 = swap boolean, deltas,
/// first-half rounds, partial rounds, second-half rounds, outputs), one past the last wire used.
/// FORK: written against the accessor names of upstream's `PoseidonGate` (`wire_input`, `wire_output`, `WIRE_SWAP`,
/// `wire_delta`, `wire_full_sbox_0`, `wire_partial_sbox`, `wire_full_sbox_1`, `end`) carried over to `Poseidon2Gate`; if the
/// fork names or orders them differently, this function is the single place to change — the device, the host verifier and the
/// oracle all read the table (`tests/test_poseidon2_gate*.py` exercise a second layout to prove it). If the fork's gate
/// constrains in another ORDER than upstream's PoseidonGate, add a new `constraint_order` value on both sides.
fn poseidon2_gate_layout() -> [u64; 10] {
    use plonky2::gates::poseidon2::Poseidon2Gate;       // FORK: module path
    type G = Poseidon2Gate<plonky2::field::goldilocks_field::GoldilocksField, 2>;
    let first_round_recorded = 0u64;                    // upstream PoseidonGate records S-box inputs from round 1 on
    [G::wire_input(0) as u64, G::wire_output(0) as u64, G::WIRE_SWAP as u64, G::wire_delta(0) as u64,
     G::wire_full_sbox_0(1, 0) as u64, G::wire_partial_sbox(0) as u64, G::wire_full_sbox_1(0, 0) as u64,
     first_round_recorded, 0, G::end() as u64]
}

/// Index of a target in plonky2's flat target space (`Target::index`): wires first, virtual targets after the trace.
fn target_index(t: Target, num_wires: usize, degree: usize) -> usize {
    match t {
        Target::Wire(w) => w.row * num_wires + w.column,
        Target::VirtualTarget { index } => degree * num_wires + index,
    }
}

/// For every copy class (partition of `representative_map`) one ROUTED wire cell of the trace, if the class has one.
/// `representative_map[i]` is the representative of target i (ProverOnlyCircuitData, built by `CircuitBuilder::build`).
fn class_cells<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
    prover: &ProverOnlyCircuitData<F, C, D>, common: &CommonCircuitData<F, D>,
) -> std::collections::HashMap<usize, u64> {
    let (nw, nr, n) = (common.config.num_wires, common.config.num_routed_wires, common.degree());
    let mut cell_of_rep = std::collections::HashMap::new();
    for row in 0..n {
        for col in 0..nr {
            let idx = row * nw + col;
            cell_of_rep.entry(prover.representative_map[idx]).or_insert((row * nw + col) as u64);
        }
    }
    cell_of_rep
}

/// The wire cell (row * num_wires + column) that carries target `t`, or `None` for a target the builder never routed
/// into the trace (an unused virtual target).
fn cell_of_target<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
    t: Target, prover: &ProverOnlyCircuitData<F, C, D>, common: &CommonCircuitData<F, D>,
    cell_of_rep: &std::collections::HashMap<usize, u64>,
) -> Option<u64> {
    let (nw, n) = (common.config.num_wires, common.degree());
    if let Target::Wire(w) = t {
        if w.column < common.config.num_routed_wires { return Some((w.row * nw + w.column) as u64); }
        return Some((w.row * nw + w.column) as u64);      // an unrouted wire is its own cell
    }
    cell_of_rep.get(&prover.representative_map[target_index(t, nw, n)]).copied()
}

/// Serialise what `prove` needs. Little-endian u64 words, layout documented in csrc/circuit.hpp.
pub fn circuit_pack<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
    data: &CircuitData<F, C, D>,
) -> Result<Vec<u64>> {
    let (c, p, cfg) = (&data.common, &data.prover_only, &data.common.config);
    if c.num_lookup_polys != 0 { bail!("lookup arguments are not implemented by the MI355X backend") }
    let sel = &c.selectors_info;
    let num_selectors = sel.num_selectors();
    let n = c.degree();
    let mut w: Vec<u64> = vec![QPCP_MAGIC];
    w.extend([c.degree_bits(), cfg.num_wires, cfg.num_routed_wires, c.num_constants - num_selectors, num_selectors,
              cfg.num_challenges, c.quotient_degree_factor, c.num_partial_products, c.num_public_inputs,
              cfg.fri_config.rate_bits, cfg.fri_config.cap_height, cfg.fri_config.proof_of_work_bits as usize,
              cfg.fri_config.num_query_rounds,
              // FORK: `zero_knowledge` = salted Merkle leaves (upstream). If the fork's "RowBlinding" mode only randomises
              // padding rows and does not salt leaves (common/src/circuit.rs:382-402), write 0 here.
              cfg.zero_knowledge as usize,
              c.num_gate_constraints, c.gates.len(), c.fri_params.reduction_arity_bits.len()].map(|x| x as u64));
    w.extend(c.fri_params.reduction_arity_bits.iter().map(|&b| b as u64));
    for (i, g) in c.gates.iter().enumerate() {
        let (ty, p0, p1, mut p2) = gate_code(&g.0.id())?;
        if ty == 10 && p2 == 0 {   // RandomAccessGate::num_extra_constants
            let used = (2 + (1usize << p0)) * p1 as usize;
            p2 = core::cmp::min(cfg.num_constants, cfg.num_routed_wires.saturating_sub(used)) as u64;
        }
        let group = &sel.groups[sel.selector_indices[i]];
        w.extend([ty, p0, p1, sel.selector_indices[i] as u64, group.start as u64, group.end as u64, g.0.num_constraints() as u64, p2]);
    }
    w.extend(c.k_is.iter().map(|k| k.to_canonical_u64()));
    w.extend(data.verifier_only.circuit_digest.elements.iter().map(|e| e.to_canonical_u64()));
    // constants_sigmas oracle, column order = plonky2's: selectors, constants, sigmas; VALUES on the subgroup in natural order
    for poly in &p.constants_sigmas_commitment.polynomials {
        let values = PolynomialCoeffs::new(poly.coeffs.clone()).fft().values;
        if values.len() != n { bail!("constants/sigmas polynomial of unexpected length") }
        w.extend(values.iter().map(|v| v.to_canonical_u64()));
    }
    // public-input cells: where `prover_only.public_inputs` (the registered targets, in registration order) sit in the trace
    if c.num_public_inputs > 0 {
        let cells = class_cells(p, c);
        w.push(PUBI_MAGIC);
        w.push(c.num_public_inputs as u64);
        for &t in &p.public_inputs {
            w.push(cell_of_target(t, p, c, &cells).ok_or_else(|| anyhow!("a public-input target is not routed into the trace"))?);
        }
    }
    // the Poseidon2 gate's wire layout, when the circuit uses that gate
    if c.gates.iter().any(|g| g.0.id().starts_with("Poseidon2Gate")) {
        w.push(P2GL_MAGIC);
        w.push(10);
        w.extend(poseidon2_gate_layout());
        let _ = P2_NO_SWAP;      // (a fork gate without swap wires writes P2_NO_SWAP as word 2)
    }
    // (the hint trailer — generators that are not attached to a gate — is only needed for stage s1 on the device; without
    // it qpgpu_prove takes the full witness plonky2's own generate_partial_witness produced. See INTEGRATION.md section 2d.)
    Ok(w)
}

/// Logical-target map of the leaf circuit for `qpgpu_leaf_map_targets` (include/qpgpu_leaf.h): the cell of every target
/// `fill_witness` sets, in the QPGPU_LT_* order. `targets` is `wormhole_circuit::circuit::CircuitTargets`.
/// A target that reached no wire maps to `u64::MAX` (qpgpu_leaf_map_targets skips it).
pub fn leaf_target_map<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
    data: &CircuitData<F, C, D>, flat_targets: &[Target],      // CircuitTargets flattened in QPGPU_LT_* order by the caller
) -> Vec<u64> {
    let cells = class_cells(&data.prover_only, &data.common);
    flat_targets.iter().map(|&t| cell_of_target(t, &data.prover_only, &data.common, &cells).unwrap_or(u64::MAX)).collect()
}

/// Target map of a recursive wrapper (private / public batch) for `qpgpu_batch_fill_proof_targets` (include/qpgpu_batch.h):
/// the cell of every logical target, slot-major, in the header's documented order — per proof target the public inputs, the
/// three caps, the openings of the zeta batch and of the zeta-next batch, pow_witness, the final polynomial, the commit-phase
/// caps and the query rounds — followed by the N x 4 dummy-nullifier preimage targets. `proof_targets` are the wrapper's
/// `ProofWithPublicInputsTarget`s (`PrivateBatchCircuitTargets::leaf_proofs`, private_batch/circuit/circuit_logic.rs),
/// `preimages` its `dummy_nullifier_pre_images`.
pub fn proof_target_map<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
    data: &CircuitData<F, C, D>, proof_targets: &[plonky2::plonk::proof::ProofWithPublicInputsTarget<D>], preimages: &[[Target; 4]],
) -> Vec<u64> {
    let cells = class_cells(&data.prover_only, &data.common);
    let mut flat: Vec<Target> = Vec::new();
    for pt in proof_targets {
        flat.extend(pt.public_inputs.iter().copied());
        let p = &pt.proof;
        for cap in [&p.wires_cap, &p.plonk_zs_partial_products_cap, &p.quotient_polys_cap] {
            for h in &cap.0 { flat.extend(h.elements); }
        }
        let o = &p.openings;
        for batch in [&o.constants, &o.plonk_sigmas, &o.wires, &o.plonk_zs, &o.partial_products, &o.quotient_polys, &o.plonk_zs_next] {
            for e in batch.iter() { flat.extend(e.to_target_array()); }
        }
        let f = &p.opening_proof;
        flat.push(f.pow_witness);
        for e in &f.final_poly.0 { flat.extend(e.to_target_array()); }
        for cap in &f.commit_phase_merkle_caps { for h in &cap.0 { flat.extend(h.elements); } }
        for q in &f.query_round_proofs {
            for (evals, path) in &q.initial_trees_proof.evals_proofs {
                flat.extend(evals.iter().copied());
                for h in &path.siblings { flat.extend(h.elements); }
            }
            for st in &q.steps {
                for e in &st.evals { flat.extend(e.to_target_array()); }
                for h in &st.merkle_proof.siblings { flat.extend(h.elements); }
            }
        }
    }
    for pre in preimages { flat.extend(pre.iter().copied()); }
    flat.iter().map(|&t| cell_of_target(t, &data.prover_only, &data.common, &cells).unwrap_or(u64::MAX)).collect()
}

// ---------------------------------------------------------------------------------------------------------------------
// The prove hook
// ---------------------------------------------------------------------------------------------------------------------
pub struct GpuCircuit { ctx: *mut QpgpuCtx, circuit: *mut QpgpuCircuit }
unsafe impl Send for GpuCircuit {}     // one GpuCircuit per proving worker thread (a ctx owns one HIP stream)

impl GpuCircuit {
    /// Once per circuit, right after `builder.build()` / `build_prover()`.
    pub fn from_circuit_data<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
        device: i32, data: &CircuitData<F, C, D>, max_batch: u32,
    ) -> Result<Self> {
        let pack = circuit_pack(data)?;
        let mut err = [0 as c_char; 200];
        if unsafe { qpgpu_pack_validate(pack.as_ptr(), pack.len(), err.as_mut_ptr()) } != 0 {
            bail!("circuit pack rejected: {}", unsafe { std::ffi::CStr::from_ptr(err.as_ptr()) }.to_string_lossy());
        }
        let mut ctx = core::ptr::null_mut();
        if unsafe { qpgpu_ctx_create(device, &mut ctx) } != QPGPU_OK { bail!("no MI355X device {device}") }
        // FORK: if `PoseidonGoldilocksConfig::Hasher` is Poseidon2 in the fork, select it here BEFORE loading:
        //   qpgpu_ctx_set_hasher(ctx, 1, qp_poseidon_core constants as 146 words: ext rc 8x12, int rc 22, diag 12, M4 16)
        let mut circuit = core::ptr::null_mut();
        let rc = unsafe { qpgpu_circuit_load_batch(ctx, pack.as_ptr(), pack.len(), max_batch, &mut circuit) };
        if rc != QPGPU_OK {
            let msg = last_error(ctx);
            unsafe { qpgpu_ctx_destroy(ctx) };
            bail!("qpgpu_circuit_load: {msg}");
        }
        Ok(Self { ctx, circuit })
    }

    /// `ProverCircuitData::prove(pw)`: witness generation stays plonky2's (it owns the generators), everything after it
    /// runs on the GPU. The returned proof is parsed from the same bytes the CPU prover would serialise.
    pub fn prove<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
        &self, data: &CircuitData<F, C, D>, pw: PartialWitness<F>,
    ) -> Result<ProofWithPublicInputs<F, C, D>> {
        // generate_partial_witness panics on "set twice with different values" exactly as before (the reference's tests
        // rely on it: wormhole/tests/src/circuit/block_header_tests.rs:34-95)
        let partition: PartitionWitness<F> =
            plonky2::iop::generator::generate_partial_witness(pw, &data.prover_only, &data.common)?;
        let public_inputs: Vec<u64> = partition.get_targets(&data.prover_only.public_inputs).iter().map(|f| f.to_canonical_u64()).collect();
        let full = partition.full_witness();                     // MatrixWitness { wire_values: Vec<Vec<F>> }, [wire][row]
        let n = data.common.degree();
        let mut wires: Vec<u64> = Vec::with_capacity(full.wire_values.len() * n);
        for col in &full.wire_values { wires.extend(col.iter().map(|f| f.to_canonical_u64())); }
        let mut bytes = vec![0u8; unsafe { qpgpu_proof_size(self.circuit) }];
        let mut len = 0usize;
        let rc = unsafe { qpgpu_prove(self.circuit, wires.as_ptr(), public_inputs.as_ptr(), bytes.as_mut_ptr(), bytes.len(), &mut len) };
        // the witness holds the spend secret: scrub our host copy (the library scrubs its device copies)
        for w in wires.iter_mut() { unsafe { core::ptr::write_volatile(w, 0) } }
        if rc != QPGPU_OK { bail!("{}", last_error(self.ctx)) }      // callers wrap: "Failed to prove: {e}" (prover/src/lib.rs:174)
        bytes.truncate(len);
        ProofWithPublicInputs::from_bytes(bytes, &data.common)
    }

    /// Many witnesses of this circuit at once (the aggregator's leaves): `GpuCircuit::from_circuit_data(.., max_batch)` sized
    /// the workspace; every stage is launched once for the batch. Proof i is byte-identical to `prove` of witness i alone.
    pub fn prove_batch<F: RichField + Extendable<D>, C: GenericConfig<D, F = F>, const D: usize>(
        &self, data: &CircuitData<F, C, D>, witnesses: Vec<PartialWitness<F>>,
    ) -> Result<Vec<ProofWithPublicInputs<F, C, D>>> {
        let n = data.common.degree();
        let size = unsafe { qpgpu_proof_size(self.circuit) };
        let (mut d_wires, mut pis_all): (Vec<*mut c_void>, Vec<Vec<u64>>) = (Vec::new(), Vec::new());
        for pw in witnesses {
            let partition = plonky2::iop::generator::generate_partial_witness(pw, &data.prover_only, &data.common)?;
            pis_all.push(partition.get_targets(&data.prover_only.public_inputs).iter().map(|f| f.to_canonical_u64()).collect());
            let full = partition.full_witness();
            let mut wires: Vec<u64> = Vec::with_capacity(full.wire_values.len() * n);
            for col in &full.wire_values { wires.extend(col.iter().map(|f| f.to_canonical_u64())); }
            let mut d: *mut c_void = core::ptr::null_mut();
            if unsafe { qpgpu_malloc(self.ctx, wires.len() * 8, &mut d) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
            if unsafe { qpgpu_memcpy_h2d(self.ctx, d, wires.as_ptr() as *const c_void, wires.len() * 8) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
            for w in wires.iter_mut() { unsafe { core::ptr::write_volatile(w, 0) } }
            d_wires.push(d);
        }
        let mut bufs: Vec<Vec<u8>> = (0..d_wires.len()).map(|_| vec![0u8; size]).collect();
        let outs: Vec<*mut u8> = bufs.iter_mut().map(|b| b.as_mut_ptr()).collect();
        let wire_ptrs: Vec<*const u64> = d_wires.iter().map(|d| *d as *const u64).collect();
        let pi_ptrs: Vec<*const u64> = pis_all.iter().map(|p| p.as_ptr()).collect();
        let mut lens = vec![0usize; d_wires.len()];
        let rc = unsafe { qpgpu_prove_batch_dev(self.circuit, wire_ptrs.as_ptr(), d_wires.len() as u32, pi_ptrs.as_ptr(), outs.as_ptr(), size, lens.as_mut_ptr()) };
        unsafe { qpgpu_circuit_scrub(self.circuit); }                 // device copies of everything derived from the witnesses
        let bytes = data.common.config.num_wires * n * 8;
        for d in d_wires { unsafe { qpgpu_free_scrubbed(self.ctx, d, bytes); } }   // witness copies zeroed before release
        if rc != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        bufs.into_iter().zip(lens).map(|(mut b, l)| { b.truncate(l); ProofWithPublicInputs::from_bytes(b, &data.common) }).collect()
    }
}

impl Drop for GpuCircuit {
    fn drop(&mut self) { unsafe { qpgpu_circuit_free(self.circuit); qpgpu_ctx_destroy(self.ctx); } }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stage-level route, s8..s11 step by step. `Oracle` borrows a committed batch made elsewhere
// (qpgpu_oracle_commit); `FriSession` is PolynomialBatch::prove_openings with the transcript on the Rust side:
//
//   let mut fs = FriSession::begin(ctx, &[o_cs, o_wires, o_zs, o_q], &batches, &fri_params, degree_bits, challenger.get_extension_challenge())?;
//   for _ in 0..fri_params.num_reduction_rounds {
//       let cap = fs.round_commit()?;  challenger.observe_cap(&cap);
//       fs.round_fold(challenger.get_extension_challenge())?;
//   }
//   let final_poly = fs.final_poly()?;  challenger.observe_extension_elements(&final_poly);
//   let nonce = fri_grind(ctx, &challenger.to_qpgpu(), pow_bits)?;          // or the fork's own rule
//   challenger.observe_element(nonce);  let _response = challenger.get_challenge();
//   let indices: Vec<u64> = (0..num_query_rounds).map(|_| challenger.get_challenge().to_canonical_u64() % lde_size).collect();
//   let query_rounds = fs.open(&indices)?;                                  // FriQueryRound bytes, write_fri_proof order
// ---------------------------------------------------------------------------------------------------------------------
pub struct Oracle { pub ctx: *mut QpgpuCtx, pub raw: *mut QpgpuOracle, pub path_len: usize }

impl Oracle {
    /// MerkleTree::prove at leaf indices: (rows, n x leaf_width words; paths, n x path_len x 4 words, leaf layer upwards)
    pub fn open(&self, indices: &[u64]) -> Result<(Vec<u64>, Vec<u64>)> {
        let width = unsafe { qpgpu_oracle_leaf_width(self.raw) };
        let (mut rows, mut paths) = (vec![0u64; indices.len() * width], vec![0u64; indices.len() * self.path_len * 4]);
        if unsafe { qpgpu_oracle_open(self.raw, indices.as_ptr(), indices.len(), rows.as_mut_ptr(), paths.as_mut_ptr()) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok((rows, paths))
    }
    /// proofs the oracle holds (qpgpu_oracle_commit_batch); 1 for qpgpu_oracle_commit's
    pub fn batch(&self) -> usize { unsafe { qpgpu_oracle_batch(self.raw) as usize } }
    /// proof b's polynomials [first, first + count) at points[b]: batch x count word pairs, one launch for the whole batch
    pub fn eval_batch(&self, points: &[[u64; 2]], first: u32, count: u32) -> Result<Vec<u64>> {
        if points.len() != self.batch() { bail!("eval_batch: one point per proof of the oracle") }
        let mut out = vec![0u64; points.len() * count as usize * 2];
        if unsafe { qpgpu_oracle_eval_batch(self.raw, points.as_ptr() as *const u64, first, count, out.as_mut_ptr()) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok(out)
    }
    /// `open` for every proof: indices [batch][n], each proof its own; (rows [batch][n][leaf_width], paths [batch][n][path_len][4])
    pub fn open_batch(&self, indices: &[u64]) -> Result<(Vec<u64>, Vec<u64>)> {
        let (batch, width) = (self.batch(), unsafe { qpgpu_oracle_leaf_width(self.raw) });
        if indices.len() % batch != 0 { bail!("open_batch: the same number of indices for every proof") }
        let (mut rows, mut paths) = (vec![0u64; indices.len() * width], vec![0u64; indices.len() * self.path_len * 4]);
        if unsafe { qpgpu_oracle_open_batch(self.raw, indices.as_ptr(), indices.len() / batch, rows.as_mut_ptr(), paths.as_mut_ptr()) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok((rows, paths))
    }
}

/// cap_words and final_words are the session's totals: `batch` proofs back to back for a session made by begin_batch
pub struct FriSession { ctx: *mut QpgpuCtx, raw: *mut QpgpuFriSession, cap_words: usize, final_words: usize, batch: usize }

impl FriSession {
    /// degree_bits: of the oracles. The oracles must outlive the session.
    pub fn begin(ctx: *mut QpgpuCtx, oracles: &[*mut QpgpuOracle], batches: &[QpgpuFriBatch], params: &QpgpuFriParams, degree_bits: u32,
                 alpha: [u64; 2]) -> Result<Self> {
        let mut raw: *mut QpgpuFriSession = core::ptr::null_mut();
        if unsafe { qpgpu_fri_begin(ctx, oracles.as_ptr(), oracles.len() as u32, batches.as_ptr(), batches.len() as u32, params, alpha.as_ptr(), &mut raw) } != QPGPU_OK {
            bail!("{}", last_error(ctx))
        }
        let folded: u32 = params.reduction_arity_bits[..params.num_reduction_rounds as usize].iter().sum();
        Ok(Self { ctx, raw, cap_words: 4usize << params.cap_height, final_words: 2usize << (degree_bits - folded), batch: 1 })
    }
    /// A lockstep batch: points[k][b] is proof b's point of opening batch k (the `point` fields of `batches` are not read), alphas one
    /// per proof. round_commit then returns the proofs' caps back to back, round_fold_batch takes one beta per proof, final_poly
    /// returns the proofs' coefficients back to back, open takes [batch][n] indices and returns [batch][n] query rounds.
    pub fn begin_batch(ctx: *mut QpgpuCtx, oracles: &[*mut QpgpuOracle], batches: &[QpgpuFriBatch], points: &[Vec<[u64; 2]>],
                       params: &QpgpuFriParams, degree_bits: u32, alphas: &[[u64; 2]]) -> Result<Self> {
        let batch = alphas.len();
        if points.len() != batches.len() || points.iter().any(|p| p.len() != batch) { bail!("begin_batch: one point per opening batch and proof") }
        let flat: Vec<u64> = points.iter().flatten().flatten().copied().collect();
        let mut raw: *mut QpgpuFriSession = core::ptr::null_mut();
        if unsafe { qpgpu_fri_begin_batch(ctx, oracles.as_ptr(), oracles.len() as u32, batches.as_ptr(), batches.len() as u32, flat.as_ptr(), batch as u32,
                                          params, alphas.as_ptr() as *const u64, &mut raw) } != QPGPU_OK {
            bail!("{}", last_error(ctx))
        }
        let folded: u32 = params.reduction_arity_bits[..params.num_reduction_rounds as usize].iter().sum();
        Ok(Self { ctx, raw, cap_words: batch * (4usize << params.cap_height), final_words: batch * (2usize << (degree_bits - folded)), batch })
    }
    pub fn batch(&self) -> usize { self.batch }
    pub fn round_fold_batch(&mut self, betas: &[[u64; 2]]) -> Result<()> {
        if betas.len() != self.batch { bail!("round_fold_batch: one beta per proof") }
        if unsafe { qpgpu_fri_round_fold(self.raw, betas.as_ptr() as *const u64) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok(())
    }
    pub fn round_commit(&mut self) -> Result<Vec<u64>> {
        let mut cap = vec![0u64; self.cap_words];
        if unsafe { qpgpu_fri_round_commit(self.raw, cap.as_mut_ptr(), cap.len()) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok(cap)
    }
    pub fn round_fold(&mut self, beta: [u64; 2]) -> Result<()> {
        if self.batch != 1 { bail!("round_fold: a session of {} proofs takes round_fold_batch", self.batch) }
        if unsafe { qpgpu_fri_round_fold(self.raw, beta.as_ptr()) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok(())
    }
    /// coefficients as word pairs
    pub fn final_poly(&mut self) -> Result<Vec<u64>> {
        let (mut out, mut n) = (vec![0u64; self.final_words], 0usize);
        if unsafe { qpgpu_fri_final_poly(self.raw, out.as_mut_ptr(), out.len(), &mut n) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        Ok(out)
    }
    /// the FriQueryRound bytes of each index, back to back
    pub fn open(&mut self, indices: &[u64]) -> Result<Vec<u8>> {
        if indices.len() % self.batch != 0 { bail!("open: the same number of indices for every proof") }
        let (mut out, mut len) = (vec![0u8; indices.len() * unsafe { qpgpu_fri_query_size(self.raw) }], 0usize);
        if unsafe { qpgpu_fri_open(self.raw, indices.as_ptr(), indices.len() / self.batch, out.as_mut_ptr(), out.len(), &mut len) } != QPGPU_OK { bail!("{}", last_error(self.ctx)) }
        out.truncate(len);
        Ok(out)
    }
}

impl Drop for FriSession { fn drop(&mut self) { unsafe { qpgpu_fri_session_free(self.raw) } } }

/// the minimum nonce under qpgpu_fri_prove's proof-of-work rule; the challenger is not advanced
pub fn fri_grind(ctx: *mut QpgpuCtx, challenger: &QpgpuChallenger, proof_of_work_bits: u32) -> Result<u64> {
    let mut nonce = 0u64;
    if unsafe { qpgpu_fri_grind(ctx, challenger, proof_of_work_bits, &mut nonce) } != QPGPU_OK { bail!("{}", last_error(ctx)) }
    Ok(nonce)
}

/// fri_grind for the transcripts of a lockstep batch in one search; none is advanced
pub fn fri_grind_batch(ctx: *mut QpgpuCtx, challengers: &[QpgpuChallenger], proof_of_work_bits: u32) -> Result<Vec<u64>> {
    let mut nonces = vec![0u64; challengers.len()];
    if unsafe { qpgpu_fri_grind_batch(ctx, challengers.as_ptr(), challengers.len() as u32, proof_of_work_bits, nonces.as_mut_ptr()) } != QPGPU_OK { bail!("{}", last_error(ctx)) }
    Ok(nonces)
}

/// A stage plan for up to max_batch proofs in lockstep (qpgpu_stage_plan_create_batch); `cs_oracle` holds one proof and must outlive it
pub struct StagePlan { pub ctx: *mut QpgpuCtx, pub raw: *mut QpgpuStagePlan }

impl StagePlan {
    pub fn create_batch(ctx: *mut QpgpuCtx, words: &[u64], cs_oracle: *const QpgpuOracle, max_batch: u32) -> Result<Self> {
        let (mut raw, mut err) = (core::ptr::null_mut(), [0 as c_char; 256]);
        if unsafe { qpgpu_stage_plan_create_batch(ctx, words.as_ptr(), words.len(), cs_oracle, max_batch, &mut raw, err.as_mut_ptr()) } != QPGPU_OK {
            bail!("{}", unsafe { std::ffi::CStr::from_ptr(err.as_ptr()) }.to_string_lossy())
        }
        Ok(Self { ctx, raw })
    }
    pub fn max_batch(&self) -> u32 { unsafe { qpgpu_stage_plan_max_batch(self.raw) } }
    /// s5 for wires.len() witnesses (device pointers when on_device): d_out receives [batch][nch * (1 + npp)][n] values
    pub fn partial_products_batch(&mut self, wires: &[*const u64], on_device: bool, betas: &[u64], gammas: &[u64], d_out: *mut u64) -> Result<()> {
        if unsafe { qpgpu_stage_partial_products_batch(self.raw, wires.as_ptr(), wires.len() as u32, on_device as i32, betas.as_ptr(), gammas.as_ptr(), d_out) } != QPGPU_OK {
            bail!("{}", last_error(self.ctx))
        }
        Ok(())
    }
    /// s6 for `batch` proofs: d_out receives [batch][nch * qdf][n] coefficients; an unsatisfied witness fails the whole batch and the message names the proof
    pub fn quotient_batch(&mut self, wires: &Oracle, zs_pp: &Oracle, batch: u32, betas: &[u64], gammas: &[u64], alphas: &[u64], pi_hashes: &[u64],
                          d_out: *mut u64) -> Result<()> {
        if unsafe { qpgpu_stage_quotient_batch(self.raw, wires.raw, zs_pp.raw, batch, betas.as_ptr(), gammas.as_ptr(), alphas.as_ptr(), pi_hashes.as_ptr(), d_out) } != QPGPU_OK {
            bail!("{}", last_error(self.ctx))
        }
        Ok(())
    }
}

impl Drop for StagePlan { fn drop(&mut self) { unsafe { qpgpu_stage_plan_free(self.raw) } } }
