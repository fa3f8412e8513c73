/*
 * qpgpu.h — C ABI of libqpgpu, the MI355X (gfx950) backend for the qp-wormhole proving hot path.
 *
 * The reference has no FFI: its "operator API" is the qp-plonky2 1.5.5 type surface reached from
 *   wormhole/prover/src/lib.rs:171-175                         (leaf  prove)
 *   wormhole/aggregator/src/private_batch/prover/lib.rs:326-330 (private batch prove)
 *   wormhole/aggregator/src/public_batch/prover/lib.rs:301-305  (public batch prove)
 * The entry points below are what a patched qp-plonky2 `plonk::prover::prove` would bind, stage by
 * stage, plus the all-in-one qpgpu_prove. INTEGRATION.md shows the
 * Rust `extern "C"` block. Plain pointers and sizes only; the caller owns every host buffer; device
 * memory is owned by the library behind opaque handles (or raw device pointers the caller got from
 * qpgpu_malloc / its own allocator). All field elements are little-endian u64; inputs may be any
 * u64 (reduced on load), outputs are canonical (< p), as `to_canonical_u64` would serialise them
 * (reference common/src/serialization.rs:40-43).
 *
 * Every function returns 0 on success or a negative QPGPU_E* code; qpgpu_last_error(ctx) gives the
 * text. Nothing aborts the process. A ctx is bound to one GPU and one HIP stream and is not
 * thread-safe; use one ctx per in-flight proof stream.
 */
#ifndef QPGPU_H
#define QPGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qpgpu_ctx qpgpu_ctx;
typedef struct qpgpu_circuit qpgpu_circuit;   /* a loaded circuit pack + its device residents and workspace */

enum {
    QPGPU_OK = 0,
    QPGPU_EINVAL = -1,      /* bad argument (size, null pointer, unsupported log_n) */
    QPGPU_EDEVICE = -2,     /* HIP runtime error; see qpgpu_last_error */
    QPGPU_ENOMEM = -3,
    QPGPU_EUNSAT = -4,      /* witness does not satisfy the circuit (quotient not divisible by Z_H) */
    QPGPU_EBUFSIZE = -5     /* caller buffer too small */
};

/* ---- context ---- */
int qpgpu_ctx_create(int device, qpgpu_ctx **out);
void qpgpu_ctx_destroy(qpgpu_ctx *ctx);
const char *qpgpu_last_error(const qpgpu_ctx *ctx);
/* Use an existing HIP stream (hipStream_t passed as void*); NULL = the ctx's own stream. */
int qpgpu_ctx_set_stream(qpgpu_ctx *ctx, void *hip_stream);
int qpgpu_sync(qpgpu_ctx *ctx);
const char *qpgpu_version(void);
/* PCI address of the context's device as "dddd:bb:dd.f" (NUL-terminated, 13 bytes): the key under /sys/bus/pci/devices a
 * caller reads the card's engine clock and power from while it measures (bench.py's `engine_clock_mhz`). */
int qpgpu_ctx_pci_bus_id(const qpgpu_ctx *ctx, char *out, size_t out_len);
/* Post-mortem evidence (csrc/crash_trace.cpp): with QPGPU_CRASH_TRACE=1 (stderr) or =<file> in the environment when the
 * library is loaded, a fatal signal writes its address, the mapping that holds it and the native backtrace of the faulting
 * thread before the previous handler (e.g. python -X faulthandler) or the default action runs. 1 = armed. */
int qpgpu_crash_trace_armed(void);

/* ---- measurement: per-kernel HIP-event timing on the ctx stream (off by default) ---- */
int qpgpu_profile_enable(qpgpu_ctx *ctx, int on);   /* on: clears the counters */
/* kernel: "ntt_pass_strided", "ntt_pass_rows", "ntt_pass_single", ... ; sums since enable */
int qpgpu_profile_read(qpgpu_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);

/* ---- device memory plumbing ---- */
int qpgpu_malloc(qpgpu_ctx *ctx, size_t bytes, void **dptr);
int qpgpu_free(qpgpu_ctx *ctx, void *dptr);
/* for buffers that held a witness: overwritten with zeros on the ctx stream, then released (the reference's zeroization
 * policy, wormhole/circuit/src/sensitive.rs:36-44) */
int qpgpu_free_scrubbed(qpgpu_ctx *ctx, void *dptr, size_t bytes);
int qpgpu_memcpy_h2d(qpgpu_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int qpgpu_memcpy_d2h(qpgpu_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int qpgpu_memcpy_d2d(qpgpu_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);   /* asynchronous on the ctx stream */

/* ---- secret residue audit (a test facility) --------------------------------------------------------------------
 * The library lists every device and pinned buffer it allocates on behalf of a context, by region; the scan looks for
 * witness-derived 64-bit words in them (the counterpart of the reference's allocator test,
 * wormhole/circuit/tests/heap_zeroization.rs). Region r's stable name is qpgpu_residue_region_name(r) (NULL past the end):
 * circuit-setup, circuit-workspace, witness-plan, partial-witness, ctx-scratch, ctx-pinned, oracle, stage-plan, fri-session,
 * pool-witness, verify-staging, zk-tree, tables. Process-wide constant tables belong to no context and are not listed
 * (DESIGN.md section 4.5); neither is anything the caller allocated (qpgpu_malloc, d_wires arguments). */
typedef struct { uint64_t word; uint32_t region; uint32_t pinned; uint64_t offset_words; uint64_t alloc_bytes; } qpgpu_residue_hit;
#define QPGPU_RESIDUE_MAX_NEEDLES 16
/* Scans every tracked buffer of ctx (device: one grid-stride kernel per buffer, 8-byte aligned 64-bit compares against up to 16
 * needles held in kernel arguments, hit count by atomicAdd, the first `cap` hits recorded; pinned: a host loop) for any needle word.
 * region_mask: bit r = scan region r; 0 = every region except circuit-setup, tables, zk-tree and verify-staging (public data).
 * A needle below 2^32 is QPGPU_EINVAL naming it: 32-bit-sized values occur in tables by chance; sensitive 64-bit words do not.
 * Synchronous on the ctx stream; same threading rule as every ctx call. Reads only memory the library itself allocated.
 * Of one device buffer at most 64 hits are recorded (all are counted): with many hits in one buffer fewer than min(hits, cap)
 * entries of first_hits are written; the unwritten ones are left as the caller passed them. hits, first_hits (with cap 0) and
 * bytes_scanned may be NULL. */
int qpgpu_ctx_residue_scan(qpgpu_ctx *ctx, const uint64_t *needles, size_t n_needles, uint64_t region_mask,
                           uint64_t *hits, qpgpu_residue_hit *first_hits, size_t cap, uint64_t *bytes_scanned);
const char *qpgpu_residue_region_name(uint32_t region);
/* From now on every tracked buffer of ctx is scanned for the needles immediately BEFORE the library frees it (i.e. after whatever
 * scrub the release path performs); hits accumulate. _end returns the totals and switches the audit off. Off by default; no cost
 * when off. _end without _begin, and _begin while an audit is open, are QPGPU_EINVAL. */
int qpgpu_ctx_residue_audit_begin(qpgpu_ctx *ctx, const uint64_t *needles, size_t n_needles);
int qpgpu_ctx_residue_audit_end(qpgpu_ctx *ctx, uint64_t *hits, qpgpu_residue_hit *first_hits, size_t cap, uint64_t *buffers_released);

/* ---- proof-system hasher -------------------------------------------------------------------------------------
 * Which permutation backs the fork's `PoseidonGoldilocksConfig` hasher (Merkle trees, Fiat-Shamir challenger, public-input
 * hash, proof of work) cannot be told from the reference, so it is a plug, and a property of the
 * context: kind 0 = plonky2's Poseidon (default; constants derived at start-up), kind 1 = Poseidon2 (width 12, x^7, 4+22+4
 * rounds) with caller-supplied parameters: 96 external round constants (round major), 22 internal round constants, the 12
 * diagonal entries d of the internal matrix J + diag(d), and the 4x4 block M4 (row major) of the external matrix
 * circ(2 M4, M4, M4) — 146 words. qpgpu_ctx_set_hasher must come before the first circuit or oracle is created on the
 * context (QPGPU_EINVAL afterwards); everything created on the context then hashes with it, and contexts with different
 * hashers coexist in one process. */
#define QPGPU_HASH_POSEIDON 0
#define QPGPU_HASH_POSEIDON2 1
#define QPGPU_POSEIDON2_PARAM_WORDS 146
int qpgpu_ctx_set_hasher(qpgpu_ctx *ctx, int kind, const uint64_t *params, size_t n_words);
int qpgpu_ctx_get_hasher(const qpgpu_ctx *ctx);
/* Deprecated process-wide default: what a new context (and the context-free helpers: synthetic circuits,
 * qpgpu_challenger_*, the workers of a proving pool) starts with. Existing contexts are not affected. */
int qpgpu_set_hasher(int kind, const uint64_t *params, size_t n_words);
int qpgpu_get_hasher(void);

/* ---- stage s2: plonky2::field::fft ---- */
enum {
    QPGPU_NTT_FORWARD = 0,        /* fft:  out[i] = P(w^i), natural order in and out */
    QPGPU_NTT_INVERSE = 1,        /* ifft: coefficients from values, includes the 1/n */
    QPGPU_NTT_OUT_BITREV = 2      /* flag: store out[bitrev(i)] (reverse_index_bits order) */
};
/*
 * Batched transform of `batch` polynomials of 2^log_n elements, polynomial c at data + c*2^log_n.
 * coset_shift: 0 or 1 = plain; otherwise forward = coset_fft(shift) (coefficients scaled by
 * shift^i first). Replaces fft_with_options / ifft_with_options / coset_fft. log_n <= 23; an LDE (qpgpu_lde_batch_dev, the
 * oracles) takes every rate_bits with log_n + rate_bits <= 23: 2^1..2^19 coefficients at up to 2^15 cosets.
 * Host-buffer form (copies in and out):
 */
int qpgpu_ntt_batch(qpgpu_ctx *ctx, uint64_t *data, unsigned log_n, size_t batch, int flags,
                    uint64_t coset_shift);
/* Device-buffer form; d_in == d_out is allowed. Asynchronous on the ctx stream. */
int qpgpu_ntt_batch_dev(qpgpu_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, unsigned log_n,
                        size_t batch, int flags, uint64_t coset_shift);
/*
 * Low-degree extension: coefficients (2^log_n per polynomial) -> values of the zero-padded polynomial
 * on the coset shift*<w_{n<<rate_bits}>; PolynomialBatch::from_coeffs minus the Merkle step.
 * flags: 0 or QPGPU_NTT_OUT_BITREV. d_out holds batch << (log_n + rate_bits) elements.
 */
int qpgpu_lde_batch_dev(qpgpu_ctx *ctx, const uint64_t *d_coeffs, uint64_t *d_out, unsigned log_n,
                        unsigned rate_bits, size_t batch, int flags, uint64_t coset_shift);

/* ---- stage s3: plonky2::hash::{poseidon, merkle_tree} ---- */
/* Poseidon permutation (width 12) on n states of 12 elements each, in place. */
int qpgpu_poseidon_permute_dev(qpgpu_ctx *ctx, uint64_t *d_states, size_t n);
/* The APPLICATION hash of the Wormhole circuits on the device: Poseidon2Hash::hash_no_pad of the qp fork (reference call
 * sites wormhole/circuit/src/unspendable_account.rs:87-88, nullifier.rs:119-120, block_header/header.rs:140,
 * common/src/zk_merkle.rs:53-58) for `count` preimages of `len` elements each, row-major at d_in: padded `|| 1 || 0*` to a
 * multiple of the rate 8 (wormhole/circuit/tests/heap_zeroization.rs:133-160), blocks added into the rate part, 4 outputs
 * per preimage at d_out. params = NULL, n_words = 0: qp-poseidon-core's parameter set, pinned by the reference's seven
 * known-answer vectors (include/qpgpu_leaf.h); otherwise a 146-word block as for qpgpu_ctx_set_hasher. Independent of the
 * context's proof-system hasher. Asynchronous on the ctx stream with the built-in set. */
int qpgpu_poseidon2_hash_pad10_dev(qpgpu_ctx *ctx, const uint64_t *params, size_t n_words, const uint64_t *d_in, size_t len,
                                   size_t count, uint64_t *d_out);
/* Digests stored by a tree: level 0 (2^log_leaves leaf digests), then each parent level down to the
 * cap level (2^cap_height digests), concatenated; 4 elements per digest. */
size_t qpgpu_merkle_digest_count(unsigned log_leaves, unsigned cap_height);
/*
 * MerkleTree::new(leaves, cap_height) for leaves given column-major and already in leaf order:
 * leaf j = (d_cols[c*col_stride + j])_{c < n_cols}; leaf digest = hash_or_noop (rows of <= 4 elements
 * are copied, longer rows go through the overwrite-mode sponge, rate 8); node = two_to_one.
 * d_digests receives qpgpu_merkle_digest_count() digests; h_cap_out (host, optional) the cap.
 */
int qpgpu_merkle_build_dev(qpgpu_ctx *ctx, const uint64_t *d_cols, uint64_t col_stride, uint32_t n_cols,
                           unsigned log_leaves, unsigned cap_height, uint64_t *d_digests, uint64_t *h_cap_out);
/* Same for row-major leaves of `width` contiguous elements (FRI round trees). */
int qpgpu_merkle_build_rows_dev(qpgpu_ctx *ctx, const uint64_t *d_rows, uint32_t width, unsigned log_leaves,
                                unsigned cap_height, uint64_t *d_digests, uint64_t *h_cap_out);

/* ---- the whole hot path: ProverCircuitData::prove after witness generation (stages s2..s12) ---- */
/*
 * Load a circuit pack ("QPCP1", qp-zk-circuits_amd/csrc/circuit.hpp: CommonCircuitData + the prover-only
 * constants/sigmas, as a Rust-side exporter would dump them). Computes the constants_sigmas commitment on the
 * GPU (what ProverOnlyCircuitData::constants_sigmas_commitment holds) and allocates the per-proof workspace,
 * so qpgpu_prove* performs no allocation. Replaces the prover-side use of the data built by
 * wormhole/circuit/src/circuit.rs:210-212 (`builder.build_prover()`).
 */
int qpgpu_circuit_load(qpgpu_ctx *ctx, const uint64_t *pack_words, size_t n_words, qpgpu_circuit **out);
/* The same with a per-proof workspace for up to max_batch proofs proven in lockstep (qpgpu_prove_batch_dev): about
 * 260 MB per proof at 2^13 rows x 135 wires. The constants/sigmas commitment is shared by the batch. */
int qpgpu_circuit_load_batch(qpgpu_ctx *ctx, const uint64_t *pack_words, size_t n_words, unsigned max_batch, qpgpu_circuit **out);
unsigned qpgpu_circuit_max_batch(const qpgpu_circuit *c);
size_t qpgpu_circuit_num_public_inputs(const qpgpu_circuit *c);
/* Releases the handle; every device region that held witness-derived data is overwritten first. */
void qpgpu_circuit_free(qpgpu_circuit *c);
/* Overwrites the witness-derived workspace now (witness copy, Z / quotient values, coefficients, LDEs, salts, FRI
 * workspace, openings), the stage s1 value buffers of the circuit (public-input values and hash, prepared partial-witness
 * values and keys) and, of its context, the transform scratch and the pinned bounce buffer. qpgpu_prove does this after
 * every proof; the _dev and pool entries leave the workspace as it is until the next proof, a scrub (qpgpu_pool_scrub for
 * a pool) or the free (the caller owns the witness buffer it passed and clears that itself). */
int qpgpu_circuit_scrub(qpgpu_circuit *c);
int qpgpu_circuit_constants_sigmas_cap(const qpgpu_circuit *c, uint64_t *out, size_t out_words);
/* Zero-knowledge packs (standard_recursion_zk_config, reference common/src/circuit.rs:396-402): the wires,
 * Z/partial-products and quotient oracles carry 4 salt columns per leaf: a ChaCha20 stream keyed with 256 bits that are
 * drawn from the OS entropy source (getrandom) for every proof (the reference uses thread_rng, also a CSPRNG): opened
 * salts say nothing about unopened ones. TEST HOOK: a seed set here applies to the NEXT prove call only (proof b of a
 * batch derives its key from seed + b) and makes its bytes reproducible; a proof made under a known seed is not
 * zero-knowledge against whoever knows the seed. */
int qpgpu_circuit_set_blinding_seed(qpgpu_circuit *c, uint64_t seed);
/* Optional witness check (off by default): before the quotient stage, evaluate every filtered gate constraint on the
 * trace rows and the closing of the permutation product; a violation makes qpgpu_prove* return QPGPU_EUNSAT with the
 * offending row in qpgpu_last_error. plonky2 only finds an unsatisfied witness through debug assertions or a proof that
 * fails to verify (reference tests catch the panic, wormhole/tests/src/circuit/nullifier_tests.rs:53-58). Costs one
 * extra pass over the trace and one stream sync. */
int qpgpu_circuit_set_witness_check(qpgpu_circuit *c, int on);
/* Explain an unsatisfied witness: WHICH gate constraints fail on which rows, and which routed cells break a copy constraint
 * (upstream plonky2 names the partition and both values for a broken copy, its debug assertions name the gate). wires: one
 * proof's [num_wires][2^degree_bits] matrix as qpgpu_prove (wires_on_device = 0) or qpgpu_prove_dev (1) takes it; public_inputs
 * feed the PublicInputGate hash as in qpgpu_prove. A satisfied witness returns QPGPU_OK with *count == 0 and both totals 0; an
 * unsatisfied one also returns QPGPU_OK, with findings. QPGPU_EBUFSIZE is never returned: *count findings are written
 * (<= cap) and the two totals say how much there was. Usable whether or not the witness check is switched on; needs no
 * transcript; changes nothing a later qpgpu_prove* reads. To explain one proof of a failed batch pass that proof's wires.
 *   GATE findings come first, in ascending (row, constraint) order. *failing_rows counts every row with a non-zero filtered
 *   constraint; the first max_rows (1..1024; 0 is QPGPU_EINVAL) of them are expanded, one finding per non-zero constraint:
 *   gate = the gate whose filter is non-zero on the row (index into the pack's gate list), constraint = index within that gate,
 *   value = filter * constraint, the term that enters the quotient, canonical.
 *   COPY findings follow, in ascending (row, wire) order: a routed cell whose value differs from the value at the source cell of
 *   its copy class (wire_b, row_b: the cell stage s1's copy pass fills the class from; a wrong source cell is therefore reported
 *   once per other member). *copy_mismatches counts all of them; at most cap - (GATE findings written) are written. The
 *   circuit's witness plan is made here if it has not been.
 * The values come from the gate kernels that judge the witness in the witness check, run with other weights (csrc/explain_api.cpp);
 * rows are found under a fixed weight table, which a witness not built against it escapes with probability < 2^-56 per
 * challenge column. flags: 0. failing_rows and copy_mismatches may be NULL; out may be NULL when cap is 0.
 * SECRETS: findings are functions of witness values (a COPY finding carries two cells verbatim): treat `out` like the witness.
 * Every device and pinned buffer the call allocates is listed in the residue registry (region circuit-workspace), overwritten
 * and released before the call returns, on every exit path; a host witness is uploaded into such a buffer.
 * NOT covered: stage plans (qpgpu_stage_plan), the proving pool and sharded oracles have no such entry; load the pack with
 * qpgpu_circuit_load and pass the witness here. */
enum { QPGPU_FINDING_GATE = 1, QPGPU_FINDING_COPY = 2 };
typedef struct qpgpu_witness_finding {
    uint32_t kind, gate;          /* GATE: index into the pack's gate list */
    uint32_t constraint;          /* GATE: index within the gate, 0 .. num_constraints-1 */
    uint32_t wire, wire_b;        /* COPY: this cell, and the source cell of its copy class */
    uint32_t reserved;
    uint64_t row, row_b;
    uint64_t value, value_b;      /* GATE: value = filter * constraint, canonical: the term that enters the quotient.
                                     COPY: the two cells' values, canonical */
} qpgpu_witness_finding;
int qpgpu_circuit_explain_witness(qpgpu_circuit *c, const uint64_t *wires, int wires_on_device,
                                  const uint64_t *public_inputs, uint32_t max_rows, unsigned flags,
                                  qpgpu_witness_finding *out, size_t cap, size_t *count,
                                  uint64_t *failing_rows, uint64_t *copy_mismatches);
/* host only: one line of text for a finding; gates are named as tools/pack_dump.py names them. pack_words: the circuit pack, or
 * its header form (qpgpu_stage_plan_create). At most cap - 1 characters and a NUL are written: QPGPU_OK if the line fitted,
 * QPGPU_EBUFSIZE if it was cut (buf holds the cut line). A NULL argument, cap 0, a pack that does not parse, an unknown kind, or a
 * gate, constraint, wire or row outside the pack is QPGPU_EINVAL with buf[0] = 0 (where there is a buf): nothing is read past the pack. */
int qpgpu_witness_finding_format(const uint64_t *pack_words, size_t n_words, const qpgpu_witness_finding *f,
                                 char *buf, size_t cap);
/* Quotient stage: by default a circuit whose gates, the hash gates aside, are Constant, PublicInput, Arithmetic and BaseSum<2>
 * on routed wires (the leaf circuit) gets its permutation terms and those gates from one kernel; every other circuit, and any
 * circuit after on = 0, from the two kernels that pass over the wires once each. Same proof bytes either way. The default at
 * load is 1, or 0 under QPGPU_QUOTIENT_FUSED=0. qpgpu_circuit_quotient_info: the switch, and whether the one kernel is what
 * the next proof of this circuit runs (either pointer may be NULL). */
int qpgpu_circuit_set_quotient_fused(qpgpu_circuit *c, int on);
int qpgpu_circuit_quotient_info(const qpgpu_circuit *c, int *fused_enabled, int *fused_selected);
/* Quotient stage, hash gates: a circuit whose PoseidonGate and Poseidon2 gate sit on the same wires (the Poseidon2 layout
 * carried over from PoseidonGate: the leaf circuit) gets both from one kernel that shares the wire pass and the S-boxes; any
 * other circuit, and every circuit loaded under QPGPU_QUOTIENT_PAIR=0, one kernel per gate. Same proof bytes either way.
 * enabled: the switch as read at load; selected: whether the one kernel is what the next proof of this circuit runs. A NULL
 * argument is QPGPU_EINVAL. */
int qpgpu_circuit_quotient_pair_info(const qpgpu_circuit *c, int *enabled, int *selected);
size_t qpgpu_proof_size(const qpgpu_circuit *c);   /* bytes written by qpgpu_prove for this circuit */
/*
 * prove(): wires = the full witness matrix (num_wires x 2^degree_bits, column-major, as
 * `generate_partial_witness(...).full_witness()` holds it), public_inputs on the host. Writes
 * ProofWithPublicInputs::to_bytes() order into out: wires_cap, zs_partial_products_cap, quotient_cap, openings,
 * FRI commit caps, query rounds, final polynomial, pow_witness, then the public inputs. The proof-of-work nonce
 * is the minimum valid one (the reference's rayon find_any may return any).
 * The _dev form takes wires already resident in HBM and leaves them untouched.
 */
int qpgpu_prove(qpgpu_circuit *c, const uint64_t *wires, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, size_t *out_len);
int qpgpu_prove_dev(qpgpu_circuit *c, const uint64_t *d_wires, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, size_t *out_len);
/* `batch` (<= the handle's max_batch) independent proofs of the circuit in lockstep: every stage is launched once for all
 * of them, the Fiat-Shamir transcripts advance together on the host, one stream synchronisation per stage for the batch.
 * d_wires[b] / public_inputs[b] / outs[b] (each out_cap bytes) / out_lens[b] belong to proof b; witnesses laid out back to
 * back are used in place, others are gathered into the workspace first. Each proof's bytes equal what qpgpu_prove_dev
 * gives for the same witness. An error concerns the whole batch (an unsatisfied witness names its proof). */
int qpgpu_prove_batch_dev(qpgpu_circuit *c, const uint64_t *const *d_wires, uint32_t batch, const uint64_t *const *public_inputs,
                          uint8_t *const *outs, size_t out_cap, size_t *out_lens);

/* ---- stage s1: witness generation on the device ------------------------------------------------------------------
 * `iop::generator::generate_partial_witness` for the gate-attached generators of the supported gate set (Constant,
 * Arithmetic, ArithmeticExtension, MulExtension, BaseSum split, Poseidon, Reducing*, RandomAccess, Exponentiation,
 * PoseidonMds, CosetInterpolation) plus copy-constraint propagation. The dependency order is resolved once per circuit
 * from the pack (copy classes are the cycles of the sigma permutation); generation is one kernel launch per dependency
 * level. The caller supplies the cells no generator produces — plonky2's PartialWitness; qpgpu_witness_free_mask marks
 * them (1 byte per cell, num_wires x 2^degree_bits, column-major like the wire matrix) — every other cell is
 * overwritten. Generators that are not attached to a gate (Copy, Equality, WireSplit, extension Quotient, Constant,
 * NonzeroTest, LowHigh) run too when the pack carries them in its hint trailer (csrc/circuit.hpp); outputs of generators
 * the pack does not describe count as caller-supplied cells. */
int qpgpu_witness_info(qpgpu_circuit *c, uint64_t *num_generators, uint64_t *num_levels, uint64_t *num_free_cells);
int qpgpu_witness_free_mask(qpgpu_circuit *c, uint8_t *mask, size_t mask_len);
/* in place on a device-resident wire matrix / on a host matrix (uploaded, generated, downloaded, device copy scrubbed) */
int qpgpu_generate_witness_dev(qpgpu_circuit *c, uint64_t *d_wires, const uint64_t *public_inputs);
int qpgpu_generate_witness(qpgpu_circuit *c, uint64_t *wires, const uint64_t *public_inputs);
/* `batch` witnesses of the same circuit at once (wire matrices back to back, public inputs back to back): the dependency
 * levels are walked once for all of them, which is how the device pays off — a single witness is latency-bound by the
 * circuit's dependency depth, exactly the part a host core does well. */
/* the trace rows of one gate type (the QPCP gate type codes of csrc/circuit.hpp: 4 PoseidonGate, 14 the Poseidon2 gate, ...), for tools
 * and tests; rows_out may be NULL to ask for the count */
int qpgpu_circuit_gate_rows(const qpgpu_circuit *c, unsigned gate_type, uint32_t *rows_out, size_t cap, size_t *count);
int qpgpu_generate_witness_batch_dev(qpgpu_circuit *c, uint64_t *d_wires, uint32_t batch, const uint64_t *public_inputs);
/* The same from a sparse PartialWitness: `count` assignments (cell = row * num_wires + wire, value), as the reference
 * builds them with `pw.set_target` (wormhole/prover/src/lib.rs:187-221). d_wires (num_wires x 2^degree_bits, device) is
 * cleared, the assignments and the public inputs (at the pack's public-input cells, trailer "PUBI1") are written, the
 * generators run. A target set twice with different values — two assignments inside one copy class, or an assignment that
 * disagrees with the value a generator or the public-input argument gives that target — returns QPGPU_EUNSAT and names
 * the target in qpgpu_last_error: plonky2's "set twice with different values" panic, which six reference tests expect
 * (wormhole/tests/src/circuit/block_header_tests.rs:34-95, nullifier_tests.rs:53-58). Unassigned free cells stay zero.
 * A generator that divides by zero — QuotientGeneratorExtension's denominator, InterpolationGenerator's coset shift; plonky2's
 * Field::inverse panics with "Tried to invert zero" — returns QPGPU_EUNSAT too and names the zero target (every witness entry
 * point; it is reported before a "set twice" the value written in its place may have caused). */
int qpgpu_generate_witness_partial_dev(qpgpu_circuit *c, const uint64_t *cells, const uint64_t *values, size_t count,
                                       const uint64_t *public_inputs, uint64_t *d_wires);
/* `batch` PartialWitnesses over the SAME cell list at once (every proof of one circuit assigns the same targets: the 299 of
 * wormhole/prover/src/lib.rs:187-221): values is batch x count, public_inputs batch x num_public_inputs, d_wires batch wire
 * matrices back to back. The cell list is resolved against the circuit once and kept (copy classes, which assignments seed a
 * free class and which land in a generated one); per call the values go up in one piece, the dependency levels are walked
 * once for all witnesses, and one read-back tells which witnesses had a target set twice with different values — a caller's
 * assignment against a generated value, two assignments of one class, or two generators of one class that disagree (plonky2
 * allows several generators per partition as long as they agree: `connect(computed, claimed)`). status (may be NULL): per
 * witness QPGPU_OK or QPGPU_EUNSAT; the return value is QPGPU_EUNSAT when any witness failed, with the first one's target
 * in qpgpu_last_error. */
int qpgpu_generate_witness_partial_batch_dev(qpgpu_circuit *c, const uint64_t *cells, size_t count, const uint64_t *values,
                                             const uint64_t *public_inputs, uint32_t batch, uint64_t *d_wires, int *status);
/* Resolve a cell list and size every buffer for up to max_batch witnesses now (on the loading thread), so that the generate
 * calls themselves neither allocate nor free. Optional: the generate calls do it on first use. */
int qpgpu_witness_partial_prepare(qpgpu_circuit *c, const uint64_t *cells, size_t count, uint32_t max_batch);
/* The same with RandomValueGenerator targets drawn ON THE DEVICE: the LAST n_blinding cells of `cells` (the blinding rows' wires
 * of a zero-knowledge circuit, CircuitBuilder::blind; qpgpu_wrapper_circuit_build lists them) get one uniform field element
 * each, per witness, from ChaCha20 keyed with seeds[b] (32 bytes per witness; NULL: 32 bytes of operating-system entropy per
 * witness, the key wiped after use). values: [batch][count - n_blinding]. A blinding cell must be a free cell of its own
 * (QPGPU_EINVAL otherwise). Saves drawing and uploading ~0.6 M values per private-batch proof on the host. */
int qpgpu_generate_witness_partial_batch_blinded_dev(qpgpu_circuit *c, const uint64_t *cells, size_t count, size_t n_blinding, const uint64_t *values,
                                                     const uint8_t *seeds, const uint64_t *public_inputs, uint32_t batch, uint64_t *d_wires, int *status);
/* ProverCircuitData::prove takes its public inputs OUT of the generated witness (`get_targets(&prover_data.public_inputs)`). The
 * same here: pass public_inputs = NULL to the two functions above (allowed when the circuit's PublicInputGate wires are
 * copy-connected to the in-circuit hash of the public-input targets, as CircuitBuilder::build wires them: exported circuits and
 * the library's own builder; QPGPU_EINVAL otherwise) — the public-input targets are then whatever the caller's assignments and the
 * generators make of them — and read them back with this call ([batch][num_public_inputs]) for qpgpu_prove*_dev. */
int qpgpu_witness_public_inputs_dev(qpgpu_circuit *c, const uint64_t *d_wires, uint32_t batch, uint64_t *public_inputs_out);

/* ---- stage-level entry points: the circuit-independent parts of prove() ---------------------------------------
 * For a patched `qp-plonky2::plonk::prover::prove` that keeps witness generation in Rust and moves everything after it to
 * the GPU — polynomial commitments (s2/s3), partial products (s5), the quotient (s6), opening evaluations (s7) and the whole
 * FRI opening proof (s8..s11) — so that every polynomial stays on the device from the wire commitment to the proof bytes.
 * Replaces, call for call:
 *   PolynomialBatch::from_values / from_coeffs  -> qpgpu_oracle_commit
 *   batch.merkle_tree.cap                       -> qpgpu_oracle_cap
 *   all_wires_permutation_partial_products      -> qpgpu_stage_partial_products (on a qpgpu_stage_plan, below)
 *   compute_quotient_polys                      -> qpgpu_stage_quotient
 *   batch.polynomials[i].to_extension().eval(z) -> qpgpu_oracle_eval           (OpeningSet::new)
 *   batch.get_lde_values(..)                    -> qpgpu_oracle_read / qpgpu_oracle_device_ptrs (for a caller that evaluates
 *                                                  gates of its own; the two stage entries read the LDEs in place)
 *   Challenger::{observe_*, get_*}              -> qpgpu_challenger_*         (host; optional, the Rust one works too)
 *   PolynomialBatch::prove_openings             -> qpgpu_fri_prove            (returns write_fri_proof bytes)
 * reached in the reference through wormhole/prover/src/lib.rs:171-175 and the aggregator call sites listed above. */
typedef struct qpgpu_oracle qpgpu_oracle;
#define QPGPU_ORACLE_VALUES 0u        /* input polynomials are values on the subgroup (from_values) */
#define QPGPU_ORACLE_COEFFS 1u        /* input polynomials are coefficients (from_coeffs) */
#define QPGPU_ORACLE_BLINDING 2u      /* append 4 salt elements to every leaf (zero-knowledge configs) */
#define QPGPU_ORACLE_DEVICE_INPUT 4u  /* `polys` is a device pointer */
/* polys: num_polys x 2^degree_bits, column-major (polynomial j at polys + j*2^degree_bits). With QPGPU_ORACLE_BLINDING the
 * salts are a ChaCha20 stream: blinding_seed 0 = keyed with 256 fresh bits from the OS entropy source (production);
 * non-zero = key derived from the seed (reproducible, tests only). blinding_stream selects the stream under the key
 * (the all-in-one prover uses 1, 2, 3 for wires, Z/partial products, quotient). */
int qpgpu_oracle_commit(qpgpu_ctx *ctx, const uint64_t *polys, uint32_t num_polys, unsigned degree_bits, unsigned rate_bits,
                        unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream, qpgpu_oracle **out);
void qpgpu_oracle_free(qpgpu_oracle *o);   /* overwrites the device copies before releasing them */
int qpgpu_oracle_cap(const qpgpu_oracle *o, uint64_t *out, size_t out_words);          /* 4 << cap_height words */
/* evaluations of polynomials [first, first+count) at an extension point; out: count x 2 words */
int qpgpu_oracle_eval(qpgpu_oracle *o, const uint64_t point[2], uint32_t first, uint32_t count, uint64_t *out);
#define QPGPU_ORACLE_READ_COEFFS 0u   /* count x 2^degree_bits words */
#define QPGPU_ORACLE_READ_LDE 1u      /* count x 2^(degree_bits+rate_bits) words, slot s = value at g*w^bitrev(s): the Merkle leaf order */
int qpgpu_oracle_read(qpgpu_oracle *o, unsigned what, uint32_t first, uint32_t count, uint64_t *out);
/* device pointers of the resident data, same layouts as qpgpu_oracle_read (digests: leaf layer first, cap last) */
int qpgpu_oracle_device_ptrs(const qpgpu_oracle *o, const uint64_t **d_coeffs, const uint64_t **d_lde, const uint64_t **d_digests);
/* MerkleTree::prove + the leaf: rows_out n x leaf_width words (the num_polys columns at that slot, then the 4 salt words of a
 * blinded oracle: the order the proof carries), paths_out n x (degree_bits + rate_bits - cap_height) x 4 words, siblings from the
 * leaf layer upwards. indices are leaf indices (slot s = value at g*w^bitrev(s), as QPGPU_ORACLE_READ_LDE). Either out may be NULL.
 * An index >= 2^(degree_bits + rate_bits) is QPGPU_EINVAL naming the entry; outputs untouched. n = 0 returns 0. */
int qpgpu_oracle_open(qpgpu_oracle *o, const uint64_t *indices, size_t n, uint64_t *rows_out, uint64_t *paths_out);
size_t qpgpu_oracle_leaf_width(const qpgpu_oracle *o);   /* num_polys, + 4 for a blinded oracle */

/* ---- one commitment across several contexts: coset sharding ----------------------------------------------------
 * qpgpu_oracle_commit over G = n_ctx contexts, on different devices or on the same one. G is a power of two with
 * 2 <= G <= 2^rate_bits; the contexts are distinct and have the same hasher (n_ctx = 1 is QPGPU_EINVAL naming qpgpu_oracle_commit).
 * Shard g runs on ctxs[g] and owns the leaves [g N/G, (g + 1) N/G), N = 2^(degree_bits + rate_bits): whole cosets of the LDE
 * (those k with brev_rate_bits(k) >> (rate_bits - log2 G) == g) and a whole subtree. It gets a copy of the coefficients (1 / 2^rate_bits
 * of the LDE; a peer copy between devices, no peer-access setting is read or changed), transforms, salts and hashes its leaves and
 * reduces them to its max(1, 2^cap_height / G) roots alone. ctxs[0] is the home context: `polys` with QPGPU_ORACLE_DEVICE_INPUT
 * lies on its device, it keeps the coefficients (qpgpu_oracle_eval, QPGPU_ORACLE_READ_COEFFS and the FRI arithmetic read them
 * there), and when G > 2^cap_height it hashes the log2 G - cap_height levels above the shards' roots. Other arguments, flags and
 * limits are qpgpu_oracle_commit's, and so is the result: the cap, the salts (drawn at the global leaf index), every leaf and every
 * path are word for word those of qpgpu_oracle_commit with the same arguments.
 * The calling thread drives all G streams and has synchronised them when the call returns; the threading rule of a context holds
 * for all G contexts during this and every later call on the oracle. Errors are reported on ctxs[0]. NULL ctxs, ctxs[i] or out:
 * QPGPU_EINVAL; *out is NULL after any failure.
 * On a sharded oracle qpgpu_oracle_cap, _leaf_width, _eval, _read (the LDE: the shards' blocks in leaf order), _open (each index
 * goes to its shard, one gather per shard on that shard's stream, results in the caller's order) and _free (every shard scrubbed
 * on its own context) work as on any oracle, and so do qpgpu_fri_prove, qpgpu_fri_begin .. qpgpu_fri_open and
 * qpgpu_fri_proof_size over any mix of sharded and plain oracles, with the same bytes; their ctx must be the home context of
 * every sharded oracle. qpgpu_stage_plan_create_sharded makes a stage plan over a sharded constants/sigmas oracle, and
 * qpgpu_stage_quotient on such a plan takes sharded wire and Z/partial-products oracles (the stage section below).
 * qpgpu_oracle_device_ptrs is QPGPU_EINVAL naming qpgpu_oracle_shard_device_ptrs; qpgpu_stage_plan_create, _create_batch,
 * qpgpu_stage_quotient* on a plan made by either of them, qpgpu_oracle_eval_batch, _open_batch, qpgpu_fri_prove_batch and
 * _begin_batch are QPGPU_EINVAL saying that sharded oracles are not taken there yet: none of them reads shard 0 as if it were
 * the whole. */
int qpgpu_oracle_commit_sharded(qpgpu_ctx *const *ctxs, uint32_t n_ctx, const uint64_t *polys, uint32_t num_polys,
                                unsigned degree_bits, unsigned rate_bits, unsigned cap_height, unsigned flags,
                                uint64_t blinding_seed, uint32_t blinding_stream, qpgpu_oracle **out);
uint32_t qpgpu_oracle_shards(const qpgpu_oracle *o);            /* 1 for every other oracle */
/* shard's leaves [*first_leaf, *first_leaf + *num_leaves); any oracle is its own shard 0. Either out may be NULL. */
int qpgpu_oracle_shard_range(const qpgpu_oracle *o, uint32_t shard, uint64_t *first_leaf, uint64_t *num_leaves);
/* on the shard's device: its LDE [num_polys][num_leaves] in leaf order, and its subtree's digests from the leaf layer up to its
 * roots (qpgpu_merkle_digest_count(log2 num_leaves, max(0, cap_height - log2 G)) digests). Either out may be NULL. */
int qpgpu_oracle_shard_device_ptrs(const qpgpu_oracle *o, uint32_t shard, const uint64_t **d_lde, const uint64_t **d_digests);

/* ---- lockstep batches of the stage flow: one call per stage for `batch` proofs of one circuit ------------------
 * qpgpu_prove_batch_dev launches every stage once for up to max_batch proofs; the entries below give the stage route the same
 * batch dimension, on the same launch sequences (proof = grid.z or a folded leading dimension), so a patched prove() that keeps its
 * own transcript can prove a level of leaves in lockstep. batch is 1..1024 everywhere. The transcripts stay with the caller, one per
 * proof; arrays are [batch][...], dense, proof b first. A batch of one through these entries gives what the single-proof entries give.
 *
 * One qpgpu_oracle may hold the committed batches of `batch` proofs. polys[b]: proof b's num_polys x 2^degree_bits matrix, on the
 * host or (QPGPU_ORACLE_DEVICE_INPUT) on the device, where the matrices may lie back to back (used in place) or be separate
 * allocations (gathered; same result). Flags, limits and messages are qpgpu_oracle_commit's. With QPGPU_ORACLE_BLINDING proof b's
 * key is derived from blinding_seed + b when the seed is non-zero (qpgpu_circuit_set_blinding_seed's rule for a batch); seed 0
 * draws 256 fresh bits per proof. The host copy of the keys is overwritten as soon as the device has them. */
int qpgpu_oracle_commit_batch(qpgpu_ctx *ctx, const uint64_t *const *polys, uint32_t batch, uint32_t num_polys, unsigned degree_bits,
                              unsigned rate_bits, unsigned cap_height, unsigned flags, uint64_t blinding_seed, uint32_t blinding_stream,
                              qpgpu_oracle **out);
uint32_t qpgpu_oracle_batch(const qpgpu_oracle *o);   /* proofs the oracle holds; 1 for qpgpu_oracle_commit's */
/* words between two proofs' coefficients, LDEs and digests (qpgpu_oracle_device_ptrs gives proof 0's base); 0, 0, 0 at batch 1.
 * Any out-pointer may be NULL. */
int qpgpu_oracle_strides(const qpgpu_oracle *o, uint64_t *coeffs, uint64_t *lde, uint64_t *digests);
/* On a batched oracle qpgpu_oracle_cap returns batch x (4 << cap_height) words (a smaller out_words is QPGPU_EINVAL),
 * qpgpu_oracle_leaf_width, _device_ptrs and _free work as for any oracle, and qpgpu_oracle_eval, _read and _open are QPGPU_EINVAL
 * naming the entry to use: they do not silently serve proof 0.
 * qpgpu_oracle_eval_batch: proof b's polynomials [first, first + count) at proof b's point; points [batch][2], out
 * [batch][count][2]. One upload, one launch, one read-back for the whole batch. */
int qpgpu_oracle_eval_batch(qpgpu_oracle *o, const uint64_t *points, uint32_t first, uint32_t count, uint64_t *out);
/* qpgpu_oracle_open for every proof: indices [batch][n] (each proof its own), rows_out [batch][n][leaf_width], paths_out
 * [batch][n][path][4]; either out may be NULL. One gather per 256 indices for all proofs together. An index out of range is
 * QPGPU_EINVAL naming indices[b][i]; outputs untouched. */
int qpgpu_oracle_open_batch(qpgpu_oracle *o, const uint64_t *indices, size_t n, uint64_t *rows_out, uint64_t *paths_out);

/* plonky2::iop::challenger::Challenger as plain data: buffers are Vec<F> contents, lengths their len() */
typedef struct {
    uint64_t sponge_state[12];
    uint64_t input_buffer[8];
    uint64_t output_buffer[8];
    uint32_t input_len, output_len;
} qpgpu_challenger;
void qpgpu_challenger_init(qpgpu_challenger *c);
/* under the context's hasher; QPGPU_EINVAL for a state plonky2 cannot be in (input_len >= 8 or output_len > 8) */
int qpgpu_ctx_challenger_observe(const qpgpu_ctx *ctx, qpgpu_challenger *c, const uint64_t *elements, size_t n);
int qpgpu_ctx_challenger_get(const qpgpu_ctx *ctx, qpgpu_challenger *c, uint64_t *out);
/* under the process-default hasher (first ABI); an invalid state is left untouched and get returns 0 */
void qpgpu_challenger_observe(qpgpu_challenger *c, const uint64_t *elements, size_t n);
uint64_t qpgpu_challenger_get(qpgpu_challenger *c);

typedef struct { uint32_t oracle, first, count; } qpgpu_fri_range;          /* FriPolynomialInfo::from_range */
typedef struct { uint64_t point[2]; uint32_t num_ranges; qpgpu_fri_range ranges[8]; } qpgpu_fri_batch;   /* FriBatchInfo */
typedef struct {                                                            /* FriParams */
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t num_reduction_rounds; uint32_t reduction_arity_bits[16];
} qpgpu_fri_params;
size_t qpgpu_fri_proof_size(qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_params *params);
/* PolynomialBatch::prove_openings(instance, oracles, challenger, fri_params): `challenger` is the transcript state after
 * the openings were observed and comes back as prove_openings leaves it. Writes the FriProof in write_fri_proof order
 * (commit-phase caps, query rounds, final polynomial, pow witness; minimum valid nonce). */
int qpgpu_fri_prove(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, qpgpu_challenger *challenger,
                    uint8_t *out, size_t out_cap, size_t *out_len);

/* The same proof one step at a time, for a caller who keeps the transcript: the order of observations, the proof-of-work rule
 * and the way query indices are drawn stay in the caller's code, the polynomials and trees stay on the device. qpgpu_fri_prove
 * is, over these entries and a challenger: alpha = two draws; per round observe(cap), beta = two draws; observe(final
 * polynomial); grind; observe(nonce); one draw; num_query_rounds draws taken mod 2^(degree_bits + rate_bits); its bytes are the
 * caps, the query rounds, the final polynomial and the nonce. Use qpgpu_fri_prove unless the prover being replaced differs from
 * that. One proof per session; a session follows its context's threading rule and works on the ctx stream;
 * every entry that returns data has synchronised the stream when it returns. Errors are a code with the reason in
 * qpgpu_last_error(ctx). A call out of order is QPGPU_EINVAL saying what was expected, and the session stays usable: a fold with
 * no committed round waiting, a commit while a fold is pending or after the last round, the final polynomial or an opening before
 * the last fold. */
typedef struct qpgpu_fri_session qpgpu_fri_session;
/* s8: validates exactly as qpgpu_fri_prove (same messages); builds the batched opening polynomial for `alpha` (the caller's
 * FRI alpha, 2 words) and the first layer's values. Reads rate_bits, cap_height and the reduction schedule of params;
 * proof_of_work_bits and num_query_rounds are not read. The oracles must outlive the session. *out stays NULL on error. */
int qpgpu_fri_begin(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                    uint32_t num_batches, const qpgpu_fri_params *params, const uint64_t alpha[2], qpgpu_fri_session **out);
/* s9, round r = 0, 1, ...: commit the current layer in leaves of 2^arity_bits[r] extension values -> its cap (4 << cap_height
 * words; any other cap_words is QPGPU_EINVAL naming it, nothing written) */
int qpgpu_fri_round_commit(qpgpu_fri_session *s, uint64_t *cap_out, size_t cap_words);
/* ... then fold it with the caller's beta (2 words). The fold and the next layer's values are queued on the ctx stream. */
int qpgpu_fri_round_fold(qpgpu_fri_session *s, const uint64_t beta[2]);
/* after the last fold (at once for a schedule of zero rounds): 2^(degree_bits - sum arity_bits) coefficients, 2 words each;
 * out_words must be exactly that many words (QPGPU_EINVAL naming it otherwise, nothing written). num_coeffs may be NULL. */
int qpgpu_fri_final_poly(qpgpu_fri_session *s, uint64_t *out, size_t out_words, size_t *num_coeffs);
/* s11, after the last fold, any number of times: for each index the FriQueryRound in write_fri_proof order (per oracle: row
 * [+ salt], one-byte path length, path; per round: the 2^arity_bits evaluations of the coset, one-byte path length, path), i.e.
 * the bytes qpgpu_fri_prove writes for a query round with that index. out_len = n * qpgpu_fri_query_size(s); a smaller out_cap
 * is QPGPU_EINVAL naming it, an index >= 2^(degree_bits + rate_bits) is QPGPU_EINVAL naming the entry; nothing is written. */
size_t qpgpu_fri_query_size(const qpgpu_fri_session *s);
int qpgpu_fri_open(qpgpu_fri_session *s, const uint64_t *indices, size_t n, uint8_t *out, size_t out_cap, size_t *out_len);
void qpgpu_fri_session_free(qpgpu_fri_session *s);   /* overwrites the workspace (witness-derived) before releasing it */
/* s10: the minimum nonce w for which a COPY of *c, after observe(w), answers get() with proof_of_work_bits leading zero bits,
 * the rule qpgpu_fri_prove applies. *c is not modified. 0 bits: *nonce_out = 0, no launch. Above 40 bits, or a state
 * plonky2 cannot be in: QPGPU_EINVAL. */
int qpgpu_fri_grind(qpgpu_ctx *ctx, const qpgpu_challenger *c, unsigned proof_of_work_bits, uint64_t *nonce_out);

/* The FRI opening proof for a lockstep batch. Every oracle holds `batch` proofs (qpgpu_oracle_batch == batch) or one proof shared
 * by all of them (== 1: the constants/sigmas oracle); anything else is QPGPU_EINVAL naming the oracle. The `point` field of each
 * qpgpu_fri_batch is NOT read: proof b's point for opening batch k is points[k][b] (points: [num_batches][batch][2]).
 * qpgpu_fri_prove_batch: challengers [batch], advanced in place; outs[b] receives proof b's FriProof bytes (out_cap each),
 * out_lens[b] its length (out_lens may be NULL). The transcripts advance together: the bytes are those of `batch` calls of
 * qpgpu_fri_prove. */
int qpgpu_fri_prove_batch(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                          uint32_t num_batches, const uint64_t *points, uint32_t batch, const qpgpu_fri_params *params,
                          qpgpu_challenger *challengers, uint8_t *const *outs, size_t out_cap, size_t *out_lens);
/* A session of `batch` proofs; alphas [batch][2]. The step entries above keep their prototypes and read the session's batch
 * count; their arrays hold the proofs back to back:
 *   qpgpu_fri_round_commit   cap_words  exactly batch * (4 << cap_height)
 *   qpgpu_fri_round_fold     beta       [batch][2]
 *   qpgpu_fri_final_poly     out_words  exactly batch x the single-proof count (*num_coeffs stays per proof)
 *   qpgpu_fri_open           indices    [batch][n]; out [batch][n * qpgpu_fri_query_size(s)]; out_cap, out_len: the total
 * A wrong size is QPGPU_EINVAL naming the expected number; nothing is written and the session stays usable. The order rules are
 * unchanged; qpgpu_fri_round_fold still only queues work. */
int qpgpu_fri_begin_batch(qpgpu_ctx *ctx, qpgpu_oracle *const *oracles, uint32_t num_oracles, const qpgpu_fri_batch *batches,
                          uint32_t num_batches, const uint64_t *points, uint32_t batch, const qpgpu_fri_params *params,
                          const uint64_t *alphas, qpgpu_fri_session **out);
uint32_t qpgpu_fri_session_batch(const qpgpu_fri_session *s);   /* 1 for qpgpu_fri_begin's */
/* qpgpu_fri_grind for `batch` transcripts in one search: cs [batch] (not modified; all at the same point of the transcript, i.e.
 * with the same number of pending inputs, QPGPU_EINVAL otherwise), nonces_out [batch]. */
int qpgpu_fri_grind_batch(qpgpu_ctx *ctx, const qpgpu_challenger *cs, uint32_t batch, unsigned proof_of_work_bits, uint64_t *nonces_out);

/* ---- stages s5 and s6 of the stage flow: partial products and the quotient on the device ----------------------
 * A qpgpu_stage_plan holds what the two gate-dependent stages need and what does not depend on a witness — what a circuit
 * handle prepares at load: the sigma values on the subgroup (forward NTT of the constants/sigmas oracle's coefficients), the
 * subgroup / coset / vanishing tables, the gate table and the folded hash-gate schedule. The launch sequences are the ones
 * qpgpu_prove* runs, at a batch of one, so the stage flow's proof equals qpgpu_prove_dev's byte for byte.
 *
 * words: a full QPCP1 pack (qpgpu_circuit_load's input), or the same words with the constants/sigmas VALUE block left out:
 * everything up to and including k_is and circuit_digest, then the trailers (the P2GL1 trailer is needed when gate type 14 is
 * present; hint and PUBI1 trailers are accepted and ignored). The two forms are told apart by length; any other length is
 * QPGPU_EINVAL. The header goes through the rules of qpgpu_circuit_load (a type-14 gate without its layout trailer is refused
 * with the loader's message) BEFORE ctx and cs_oracle are looked at: a refusal of the words needs no device.
 * cs_oracle: the caller's commitment of the constants/sigmas polynomials, qpgpu_oracle_commit(QPGPU_ORACLE_VALUES, no blinding)
 * over num_selectors + num_constants + num_routed_wires columns; its column count, degree_bits and rate_bits are checked
 * against the header (QPGPU_EINVAL names cs_oracle). The plan reads the oracle's LDE in place and does NOT own it: the oracle
 * must outlive the plan; freeing it first is the caller's error.
 * err (may be NULL): QPGPU_STAGE_ERR_CAP bytes for the reason; with a context it is qpgpu_last_error too. *out stays NULL on
 * every error. A plan follows its context's threading rule: one thread at a time, on the ctx stream. */
typedef struct qpgpu_stage_plan qpgpu_stage_plan;
#define QPGPU_STAGE_ERR_CAP 256
int qpgpu_stage_plan_create(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle,
                            qpgpu_stage_plan **out, char *err);
/* Overwrites the workspace (everything that held witness-derived values) before releasing it. */
void qpgpu_stage_plan_free(qpgpu_stage_plan *plan);
/* Sizes for the caller's buffers, and whether the one-kernel quotient (qpgpu_circuit_set_quotient_fused) is what
 * qpgpu_stage_quotient runs for this circuit. Any out-pointer may be NULL. */
int qpgpu_stage_plan_info(const qpgpu_stage_plan *plan, unsigned *degree_bits, unsigned *num_challenges,
                          unsigned *num_partial_products, unsigned *quotient_degree_factor, int *fused_selected);
/* s5. wires: the num_wires x 2^degree_bits witness matrix, column-major — what the caller just committed — on the host or,
 * with wires_on_device != 0, in HBM (left untouched). betas, gammas: num_challenges words each (host). d_out (device):
 * num_challenges * (1 + num_partial_products) columns of 2^degree_bits values in the order the all-in-one prover commits them
 * (Z_0 .. Z_{nch-1}, then the partial products of challenge 0, of challenge 1, ...), ready for
 * qpgpu_oracle_commit(QPGPU_ORACLE_VALUES | QPGPU_ORACLE_DEVICE_INPUT [| QPGPU_ORACLE_BLINDING]). Synchronous on the ctx stream. */
int qpgpu_stage_partial_products(qpgpu_stage_plan *plan, const uint64_t *wires, int wires_on_device, const uint64_t *betas,
                                 const uint64_t *gammas, uint64_t *d_out);
/* s6. Reads the resident LDEs of the wires oracle, the Z/partial-products oracle and the plan's constants/sigmas oracle in
 * place (the salt columns of a blinded oracle are not polynomial columns: they lie outside the column stride and are not read).
 * alphas: num_challenges words; public_inputs_hash: 4 words (host). d_out (device): num_challenges * quotient_degree_factor
 * columns of 2^degree_bits COEFFICIENTS (the quotient chunks), for
 * qpgpu_oracle_commit(QPGPU_ORACLE_COEFFS | QPGPU_ORACLE_DEVICE_INPUT [| QPGPU_ORACLE_BLINDING]). Synchronous on the ctx stream.
 * The witness check of qpgpu_circuit_set_witness_check is part of this call (the stage flow has no later point at which an
 * unsatisfied witness would show): QPGPU_EUNSAT, with the wording qpgpu_prove_dev uses under that check, for a trace that
 * violates a gate constraint (the row is named) or whose permutation product does not close; d_out is then undefined. An
 * oracle whose column count, degree_bits or rate_bits disagrees with the plan is QPGPU_EINVAL naming the argument. After any
 * error the plan's workspace has been overwritten and the plan stays usable. */
int qpgpu_stage_quotient(qpgpu_stage_plan *plan, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle,
                         const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t *public_inputs_hash,
                         uint64_t *d_out);

/* ---- the two stages over coset-sharded oracles -----------------------------------------------------------------------
 * A stage plan over a coset-sharded constants/sigmas oracle. ctx must be cs_oracle's home context; the plan takes the shard
 * contexts, their order and G from the oracle. Header rules, limits, `err` and the order of checks (header before ctx and oracle)
 * are qpgpu_stage_plan_create's. A cs_oracle that is not sharded is QPGPU_EINVAL naming qpgpu_stage_plan_create.
 *
 * On such a plan qpgpu_stage_partial_products works as on any plan, on the home context alone (s5 lives on the 2^degree_bits trace
 * domain; the sigma values come from the coefficients, which the home context keeps). qpgpu_stage_quotient takes wires_oracle and
 * zs_pp_oracle sharded over the same contexts in the same order as the plan's cs_oracle; a plain oracle, another number of shards,
 * another context at some position or another home context is QPGPU_EINVAL naming the argument and what disagrees. The quotient
 * domain is the LDE points with natural index 0 mod 2^q_shift (q_shift = rate_bits - log2 quotient_degree_factor), so the first
 * Gq = max(1, G >> q_shift) shards hold its points, Nq / Gq each, and evaluate them on their own contexts and streams with the launch
 * sequence of qpgpu_stage_quotient, from their own slices of the three LDEs (the standard configuration, rate_bits 3 and factor 8:
 * every shard works; rate_bits above log2 of the factor: only the first Gq do). Each transforms its values to coefficients alone;
 * the home context gathers the Gq blocks (a peer copy between devices; on one device a shard writes its block in place; no
 * peer-access setting is read or changed) and one kernel there, the last radix-Gq pass of the inverse transform, writes the chunks.
 * d_out is on the home context's device; its contents, layout and meaning are qpgpu_stage_quotient's, word for word those of the
 * unsharded call. The witness check is part of the call and runs on the home context from the coefficients, with the same
 * QPGPU_EUNSAT wording. The calling thread drives all G streams and has synchronised them when the call returns; after any error
 * the plan's workspace and pinned staging have been overwritten on every shard context, and the plan stays usable.
 * qpgpu_stage_plan_info and _free (every shard's workspace scrubbed on its own context) work; qpgpu_stage_plan_max_batch is 1;
 * qpgpu_stage_partial_products_batch and qpgpu_stage_quotient_batch are QPGPU_EINVAL saying that a sharded plan takes one proof.
 * Limits are unchanged: degree_bits + rate_bits <= 23. */
int qpgpu_stage_plan_create_sharded(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle,
                                    qpgpu_stage_plan **out, char *err);
uint32_t qpgpu_stage_plan_shards(const qpgpu_stage_plan *plan);   /* 1 for every other plan, 0 for NULL */

/* The two stages for a lockstep batch. qpgpu_stage_plan_create_batch: a plan whose workspace holds max_batch proofs (1..1024,
 * checked together with the header, before ctx or cs_oracle is looked at: the refusal needs no device); qpgpu_stage_plan_create is
 * max_batch = 1. cs_oracle is the constants/sigmas commitment shared by all proofs: it must hold one proof (QPGPU_EINVAL names it
 * otherwise). */
int qpgpu_stage_plan_create_batch(qpgpu_ctx *ctx, const uint64_t *words, size_t n_words, const qpgpu_oracle *cs_oracle,
                                  uint32_t max_batch, qpgpu_stage_plan **out, char *err);
uint32_t qpgpu_stage_plan_max_batch(const qpgpu_stage_plan *plan);
/* s5 for `batch` witnesses (batch > max_batch is QPGPU_EINVAL naming it): wires[b] is proof b's matrix, on the host or, with
 * wires_on_device != 0, in HBM, back to back (read in place) or as separate allocations (gathered into the plan). betas, gammas:
 * [batch][num_challenges]. d_out (device): [batch][num_challenges * (1 + num_partial_products)][2^degree_bits] values, dense, so
 * qpgpu_oracle_commit_batch(QPGPU_ORACLE_DEVICE_INPUT) with polys[b] = d_out + b * cols * n uses them in place. */
int qpgpu_stage_partial_products_batch(qpgpu_stage_plan *plan, const uint64_t *const *wires, uint32_t batch, int wires_on_device,
                                       const uint64_t *betas, const uint64_t *gammas, uint64_t *d_out);
/* s6 for a batch: both oracles must hold exactly `batch` proofs (QPGPU_EINVAL naming the argument otherwise). betas, gammas,
 * alphas: [batch][num_challenges]; public_inputs_hashes: [batch][4]. d_out (device): [batch][num_challenges *
 * quotient_degree_factor][2^degree_bits] coefficients, dense. The witness check is part of the call, with the semantics of
 * qpgpu_prove_batch_dev: QPGPU_EUNSAT concerns the whole batch, and the message names the proof ("(proof b of the batch)").
 * After any error the workspace has been overwritten and the plan stays usable. */
int qpgpu_stage_quotient_batch(qpgpu_stage_plan *plan, const qpgpu_oracle *wires_oracle, const qpgpu_oracle *zs_pp_oracle, uint32_t batch,
                               const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas,
                               const uint64_t *public_inputs_hashes, uint64_t *d_out);

/* ---- proving pool: several proofs of one circuit in flight on one GPU ------------------------------------------
 * The native counterpart of the reference's dedicated proving worker (wormhole/aggregator/src/aggregator.rs:14-43):
 * `workers` host threads, each with its own context (HIP stream) and loaded copy of the circuit, fed from one queue.
 * One proof leaves most of the GPU idle between its latency-bound stages; four workers reach the throughput plateau.
 * submit() never blocks; wait() blocks until that proof is written (tickets may be waited for in any order, once). The
 * witness matrices and output buffers must stay valid until their ticket has been waited for. */
typedef struct qpgpu_pool qpgpu_pool;
int qpgpu_pool_create(int device, const uint64_t *pack_words, size_t n_words, unsigned workers, qpgpu_pool **out);
/* Workers that prove in lockstep: each takes up to max_batch queued proofs at once (qpgpu_prove_batch_dev). Two workers of
 * eight keep the GPU busy while one of them is in a host-side stage. The workers' contexts use the process-default hasher. */
int qpgpu_pool_create_batched(int device, const uint64_t *pack_words, size_t n_words, unsigned workers, unsigned max_batch, qpgpu_pool **out);
/* The same over several GPUs of one process — north_star's "proofs shard one-per-GPU across the node ... invoked from Rust
 * through a thin C-ABI": devices[0..n_devices) (a device may be named twice: two worker sets on one GPU), workers_per_device
 * workers on each, ONE queue. Proofs are independent, so there is no data-path collective: whichever
 * worker takes a job writes the proof into the caller's host buffer, which is the whole "gather of proof bytes" inside one
 * process (RCCL is for bench.py's one-process-per-GPU launch). The level schedule of an aggregation tree
 * (wormhole/aggregator/src/aggregator.rs:187-227) stays the caller's: submit a level's proofs, wait for them, build the next.
 * flags: QPGPU_POOL_HOST_WITNESS gives every worker a workspace of max_batch wire matrices, which qpgpu_pool_submit_host needs
 * (qpgpu_pool_set_partial_cells allocates it too). */
#define QPGPU_POOL_HOST_WITNESS 1u
int qpgpu_pool_create_multi(const int *devices, unsigned n_devices, const uint64_t *pack_words, size_t n_words, unsigned workers_per_device,
                            unsigned max_batch, unsigned flags, qpgpu_pool **out);
/* A job's arguments are checked at submit (null pointers: QPGPU_EINVAL; out_cap below qpgpu_pool_proof_size:
 * QPGPU_EBUFSIZE). Jobs of different callers share a lockstep batch: when a batch fails, its jobs are proven again one at
 * a time, so only the failing job's wait() returns the error (with that job's own message). */
void qpgpu_pool_destroy(qpgpu_pool *p);          /* drains the queue first; scrubs as qpgpu_pool_scrub does before anything is released */
/* Every worker, after the job it is in: scrubs its circuit workspace (qpgpu_circuit_scrub's regions), its resident
 * witness buffers and its partial-witness buffers. Returns when all have. Jobs submitted meanwhile run afterwards. */
int qpgpu_pool_scrub(qpgpu_pool *p);
/* qpgpu_ctx_residue_scan run by each worker on its own context (the threading rule), totals summed; first_hits from the lowest
 * worker that has any. */
int qpgpu_pool_residue_scan(qpgpu_pool *p, const uint64_t *needles, size_t n_needles, uint64_t region_mask,
                            uint64_t *hits, qpgpu_residue_hit *first_hits, size_t cap, uint64_t *bytes_scanned);
/* qpgpu_circuit_set_witness_check on every worker's circuit; only while no ticket is outstanding (QPGPU_EINVAL otherwise) */
int qpgpu_pool_set_witness_check(qpgpu_pool *p, int on);
size_t qpgpu_pool_proof_size(const qpgpu_pool *p);
unsigned qpgpu_pool_workers(const qpgpu_pool *p);
unsigned qpgpu_pool_devices(const qpgpu_pool *p);
/* 1 when the pool's workers take turns on the device: a queue-intercepting profiler (rocprofv3) was found in the process at creation
 * (its interceptor has faulted under concurrent submission from several threads), or QPGPU_POOL_SERIALIZE=1 */
int qpgpu_pool_serialized(const qpgpu_pool *p);
const char *qpgpu_pool_last_error(const qpgpu_pool *p);
/* Three forms of a job's witness. (1) a full wire matrix resident on a device: only that device's workers can read it —
 * qpgpu_pool_submit_on names the device by its index in `devices` (qpgpu_pool_submit = index 0). */
int qpgpu_pool_submit(qpgpu_pool *p, const uint64_t *d_wires, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, uint64_t *ticket);
int qpgpu_pool_submit_on(qpgpu_pool *p, unsigned device_index, const uint64_t *d_wires, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, uint64_t *ticket);
/* (2) a full wire matrix in host memory — what a patched qp-plonky2 prove() holds after
 * `generate_partial_witness(..).full_witness()` — taken by any worker of any device and uploaded on that worker's stream
 * (about 9 MB per proof at 2^13 rows; over PCIe). The matrix must stay valid until the ticket has been waited for. */
int qpgpu_pool_submit_host(qpgpu_pool *p, const uint64_t *wires, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, uint64_t *ticket);
/* (3) a PartialWitness: the values of the cell list set once with qpgpu_pool_set_partial_cells (for the leaf circuit:
 * qpgpu_leaf_commit's cells / values, i.e. WormholeProver::commit, wormhole/prover/src/lib.rs:156-163). The worker that takes
 * the job runs stage s1 for its whole lockstep batch (qpgpu_generate_witness_partial_batch_dev) and then stages s2..s12: this
 * is the reference bench's timed region, `prover.commit(&inputs).unwrap().prove()` (wormhole/prover/benches/prover.rs:38),
 * from the committed assignments on. `values` (as many words as the cell list) are copied at submit and wiped after use; an
 * unsatisfiable witness fails its own ticket with QPGPU_EUNSAT and the target's name, the rest of its batch is proven. */
int qpgpu_pool_set_partial_cells(qpgpu_pool *p, const uint64_t *cells, size_t count);
/* The same for a zero-knowledge circuit: the LAST n_blinding cells are the blinding rows' random wires, drawn on the device for
 * every proof (qpgpu_generate_witness_partial_batch_blinded_dev, operating-system entropy); a job's `values` then has
 * count - n_blinding words. public_inputs may be NULL in qpgpu_pool_submit_partial: the job is proven with the public inputs its
 * witness holds (they are the last num_public_inputs words of the proof) — the batch layers, whose public inputs the circuit
 * computes; public inputs that ARE handed in are compared with the witness's (QPGPU_EUNSAT when they differ). */
int qpgpu_pool_set_partial_cells_blinded(qpgpu_pool *p, const uint64_t *cells, size_t count, size_t n_blinding);
int qpgpu_pool_submit_partial(qpgpu_pool *p, const uint64_t *values, const uint64_t *public_inputs, uint8_t *out, size_t out_cap, uint64_t *ticket);
int qpgpu_pool_wait(qpgpu_pool *p, uint64_t ticket, size_t *out_len);

/* Hash constants the library derives at start-up (host only, no GPU): the 360 Poseidon round constants and plonky2's
 * FAST_PARTIAL_* tables flattened as FIRST[12] | RC[22] | VS[22][11] | W_HATS[22][11] | INIT[11][11] (row c of INIT
 * produces element 1+c). Returns the number of words of the second table. */
size_t qpgpu_poseidon_constants(uint64_t *round_constants_360, uint64_t *fast_partial, size_t fast_partial_cap);

/* ---- synthetic circuits (stand-in for reference rows a1/a6 while no Rust exporter exists) ---- */
/*
 * Builds a satisfied plonky2-shaped circuit (PublicInput / Constant / Arithmetic / Noop gates wired by copy
 * constraints, standard_recursion_config parameters) and its witness. pack_out receives the circuit pack
 * ("QPCP1", see qp-zk-circuits_amd/csrc/circuit.hpp); wires_out num_wires x 2^degree_bits column-major;
 * pis_out num_public_inputs elements. Host-only; no GPU needed.
 */
size_t qpgpu_synth_pack_words(unsigned degree_bits, unsigned num_wires, unsigned num_routed);
/* flags bit 0: every 8th row is a PoseidonGate row (135 wires, 123 constraints of degree 7, its own selector group),
 * the gate that dominates the recursive (aggregator) circuits. bit 1: every 8th row is a BaseSumGate<2> row (the leaf
 * circuit's range checks, reference wormhole/circuit/src/zk_merkle_proof.rs:486-504). bit 2: every 8th row alternates
 * ArithmeticExtensionGate / MulExtensionGate (quadratic-extension arithmetic of the recursive verifier circuits).
 * bit 3: every 8th row cycles through ReducingGate, ReducingExtensionGate, RandomAccessGate(4 bits), ExponentiationGate
 * and PoseidonMdsGate, the rest of the gates plonky2's in-circuit verifier uses (needs >= 48 routed wires). bit 4: some
 * operation inputs come from generators that are not attached to a gate (Equality, LowHigh, NonzeroTest, Constant, Copy,
 * WireSplit, extension quotient): the pack gets a hint trailer (circuit.hpp) and qpgpu_synth_pack_words_ex is an upper bound.
 * bit 6: the LEAF PROFILE — the Wormhole leaf circuit's application hashes as rows of the qp fork's Poseidon2 gate (gate type 14,
 * qp-zk-circuits_amd/csrc/circuit.hpp): pad-10 sponge chains over 7, 4, 9, 4, 8, 45 and 16 x 16 elements (the eight
 * `hash_n_to_hash_no_pad_p2` call sites: wormhole/circuit/src/unspendable_account.rs:229-231, nullifier.rs:298-299,
 * zk_merkle_proof.rs:482,504,606, block_header/mod.rs:66; 61 permutations), one gate row per permutation and one ArithmeticGate
 * row of eight additions per further block, as many as the rows hold, plus four free-standing permutation rows; the pack
 * carries the gate's wire layout ("P2GL1"). bit 7 (with bit 6): a deliberately different wire layout (no swap wires, other block
 * order) to exercise the layout table. qpgpu_synth_p2_sites lists the hash sites (3 words each: preimage length, gate rows,
 * first slot; gate row k of a site is row 8 * (slot + k) + 3, the additions for block k + 1 are operations 0..7 of the row after
 * it, message element i is input wire i of the first gate row or the addend wire 4 (i % 8) + 2 of the add row before block i / 8,
 * the digest is the first four output wires of the last gate row). */
size_t qpgpu_synth_p2_sites(unsigned degree_bits, unsigned num_public_inputs, unsigned flags, uint64_t *out, size_t cap_words);
size_t qpgpu_synth_pack_words_ex(unsigned degree_bits, unsigned num_wires, unsigned num_routed, unsigned flags);
int qpgpu_synth_circuit_ex(unsigned degree_bits, unsigned num_wires, unsigned num_routed, unsigned num_public_inputs,
                           uint64_t seed, unsigned flags, uint64_t *pack_out, size_t pack_cap_words, size_t *pack_words,
                           uint64_t *wires_out, uint64_t *pis_out);
int qpgpu_synth_circuit(unsigned degree_bits, unsigned num_wires, unsigned num_routed, unsigned num_public_inputs,
                        uint64_t seed, uint64_t *pack_out, size_t pack_cap_words, size_t *pack_words,
                        uint64_t *wires_out, uint64_t *pis_out);

/* ---- test hooks ---- */
/*
 * qpgpu_field_probe: ONE Goldilocks primitive of the device code (qp-zk-circuits_amd/csrc/gl64.hpp, and the NTT's register
 * transforms) on caller-chosen operands, so that a test can force the carry / borrow branches that pseudo-random data reaches
 * about once in 2^32 operations. a, b and out are HOST pointers (the hook copies); index i of n reads a[i * wa ..], b[i * wb ..]
 * and writes out[i * wo ..]; out holds the raw 64-bit results, not canonicalised by the probe. on_device = 1: one thread per
 * index, 256 per block, consecutive indices in consecutive lanes of a wave. on_device = 0: the same table through the host
 * versions of the primitives (ctx may be NULL; no GPU needed). QPGPU_EINVAL: bad op / param, a NULL pointer (b only where it is
 * read), n = 0 or above 2^24, out_words < n * wo, an operand outside what the primitive's signature takes (see below), or an
 * operation the host path does not have.
 *
 *   op                         (wa, wb, wo)   out
 *   CANON NEG SQR MUL7 INV      (1, 0, 1)     f(a)                         INV: a^(p-2), canonical; CANON canonical
 *   MUL_EPS                     (1, 0, 1)     a * (2^32 - 1)               a < 2^32
 *   ADD SUB MUL                 (1, 1, 1)     a op b
 *   REDUCE128                   (1, 1, 1)     a + b * 2^64                 any (lo, hi)
 *   REDUCE96                    (1, 1, 1)     a + b * 2^64                 b < 2^32
 *   ADD_CANONICAL               (1, 1, 1)     a + b                        b < p
 *   POW                         (1, 1, 1)     a^b, canonical               b is an integer exponent
 *   MUL_POW2                    (1, 0, 1)     a * 2^param                  param < 192: gl::mul_pow2<param>
 *   MUL_POW2_DYN                (1, 0, 1)     a * 2^param                  param < 96: the NTT's mul_pow2_dyn, constant shift
 *   MUL_GROUP                   (N, N, N)     a[k] * b[k], k < N           param = N in {1, 2, 12}: gl::mul_group<N>
 *   ACC                         (T, T, 1)     sum of a[t] * b[t], t < T    param = T in 1..4096: acc_zero, T x acc_mul, acc_reduce
 *   E2_ADD E2_SUB E2_MUL        (2, 2, 2)     extension elements as word pairs [a, b] = a + b x, x^2 = 7
 *   E2_SCALE                    (2, 1, 2)     a * b, b in the base field
 *   E2_POW                      (2, 1, 2)     a^b, canonical
 *   E2_INV                      (2, 0, 2)     1 / a, canonical
 *   DIF_REGS                    (2^K, 0, 2^K) param = K | INV << 8, K in 1..6: dif_regs<K, INV>; device only
 *   DIF_SPARSE                  (2^K, 0, 2^K) param = K | INV << 8 | LV << 16: dif_sparse<K, INV, LV> for the instances the LDE
 *                                             kernels use, (K, INV, LV) = (4, 0, 1) and (5, 0, 2); device only
 */
enum {
    QPGPU_FP_CANON = 0, QPGPU_FP_ADD, QPGPU_FP_SUB, QPGPU_FP_NEG, QPGPU_FP_MUL, QPGPU_FP_SQR, QPGPU_FP_REDUCE128, QPGPU_FP_REDUCE96,
    QPGPU_FP_MUL_EPS, QPGPU_FP_ADD_CANONICAL, QPGPU_FP_MUL7, QPGPU_FP_INV, QPGPU_FP_POW, QPGPU_FP_MUL_POW2, QPGPU_FP_MUL_POW2_DYN,
    QPGPU_FP_MUL_GROUP, QPGPU_FP_ACC, QPGPU_FP_E2_ADD, QPGPU_FP_E2_SUB, QPGPU_FP_E2_MUL, QPGPU_FP_E2_SCALE, QPGPU_FP_E2_INV,
    QPGPU_FP_E2_POW, QPGPU_FP_DIF_REGS, QPGPU_FP_DIF_SPARSE, QPGPU_FP_OP_COUNT
};
int qpgpu_field_probe(qpgpu_ctx *ctx, unsigned op, unsigned param, const uint64_t *a, const uint64_t *b, size_t n,
                      uint64_t *out, size_t out_words, int on_device);

#ifdef __cplusplus
}
#endif
#endif
