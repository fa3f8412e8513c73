/*
 * stage_prove_example.c — the stage-level C ABI from plain C: plonky2's prove() after witness generation, one call per stage,
 * the way a patched qp-plonky2 `plonk::prover::prove` would issue them. Commitments
 * (qpgpu_oracle_commit), partial products and the quotient (qpgpu_stage_partial_products / qpgpu_stage_quotient on a
 * qpgpu_stage_plan made from the pack's header), openings (qpgpu_oracle_eval) and the FRI proof (qpgpu_fri_prove); the Z /
 * partial-product columns and the quotient chunks never leave the device. The assembled bytes are compared with qpgpu_prove's.
 * With a second argument "steps" the FRI proof is built one step at a time instead (qpgpu_fri_begin .. qpgpu_fri_open and
 * qpgpu_fri_grind, the transcript kept here): the route for a prover whose prove_openings differs from qpgpu_fri_prove's.
 * With "batch <N>" the whole flow runs for N witnesses in lockstep, one call per stage for all of them (the *_batch entries, N
 * transcripts kept here), and each proof's bytes are compared with qpgpu_prove_batch_dev's: a level of leaves of the aggregator.
 *
 *   gcc -O2 -I include examples/stage_prove_example.c -L qp-zk-circuits_amd -lqpgpu -Wl,-rpath,$PWD/qp-zk-circuits_amd -o /tmp/stage_prove_example
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qpgpu.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, ctx ? qpgpu_last_error(ctx) : "?"); return 1; } } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ull;
static uint64_t mulmod(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % P); }
/* the generator of the subgroup of order 2^bits: plonky2's POWER_OF_TWO_GENERATOR squared down from order 2^32 */
static uint64_t root_of_unity(unsigned bits) {
    uint64_t r = 7277203076849721926ull;
    for (unsigned i = bits; i < 32; i++) r = mulmod(r, r);
    return r;
}
static size_t put(uint8_t *out, size_t at, const uint64_t *v, size_t n) { memcpy(out + at, v, n * 8); return at + n * 8; }

static int run_batch(unsigned degree_bits, uint32_t B);

int main(int argc, char **argv) {
    unsigned degree_bits = argc > 1 ? (unsigned)atoi(argv[1]) : 10;
    if (argc > 3 && !strcmp(argv[2], "batch")) return run_batch(degree_bits, (uint32_t)atoi(argv[3]));
    const int stepwise = argc > 2 && !strcmp(argv[2], "steps");
    const unsigned num_wires = 135, num_routed = 80, num_pis = 21, flags = 3; /* Poseidon + BaseSum rows */
    qpgpu_ctx *ctx = NULL;
    if (qpgpu_ctx_create(0, &ctx)) { fprintf(stderr, "no gfx950 device: the library has no CPU fallback\n"); return 2; }

    size_t words = qpgpu_synth_pack_words_ex(degree_bits, num_wires, num_routed, flags), got = 0;
    uint64_t *pack = malloc(words * 8), *wires = malloc((size_t)num_wires * 8 << degree_bits), pis[21];
    CHECK(qpgpu_synth_circuit_ex(degree_bits, num_wires, num_routed, num_pis, 42, flags, pack, words, &got, wires, pis));

    /* the reference bytes: the all-in-one prover */
    qpgpu_circuit *circuit = NULL;
    CHECK(qpgpu_circuit_load(ctx, pack, got, &circuit));
    const size_t cap = qpgpu_proof_size(circuit);
    size_t want_len = 0;
    uint8_t *want = malloc(cap), *mine = malloc(cap);
    CHECK(qpgpu_prove(circuit, wires, pis, want, cap, &want_len));
    qpgpu_circuit_free(circuit);

    /* what the flow needs from the pack header (csrc/circuit.hpp): sizes, FRI parameters, circuit digest, constants/sigmas values */
    const size_t n = (size_t)1 << degree_bits;
    const unsigned nconst = (unsigned)pack[4], nsel = (unsigned)pack[5], nch = (unsigned)pack[6], qdf = (unsigned)pack[7], npp = (unsigned)pack[8];
    const unsigned rate_bits = (unsigned)pack[10], cap_height = (unsigned)pack[11], ngates = (unsigned)pack[16], narity = (unsigned)pack[17];
    const size_t hdr_end = 18 + narity + 8 * (size_t)ngates + num_routed + 4, ncs = nsel + nconst + num_routed, cap_words = (size_t)4 << cap_height;
    const uint64_t *digest = pack + hdr_end - 4, *cs_values = pack + hdr_end;
    qpgpu_fri_params fp = {rate_bits, cap_height, (uint32_t)pack[12], (uint32_t)pack[13], narity, {0}};
    for (unsigned i = 0; i < narity; i++) fp.reduction_arity_bits[i] = (uint32_t)pack[18 + i];

    /* per circuit: the constants/sigmas commitment and the stage plan. The plan takes the pack WITHOUT its value block. */
    qpgpu_oracle *o_cs = NULL, *o_w = NULL, *o_zs = NULL, *o_q = NULL;
    qpgpu_stage_plan *plan = NULL;
    char why[QPGPU_STAGE_ERR_CAP];
    CHECK(qpgpu_oracle_commit(ctx, cs_values, (uint32_t)ncs, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 0, &o_cs));
    if (qpgpu_stage_plan_create(ctx, pack, hdr_end, o_cs, &plan, why)) { fprintf(stderr, "stage_plan_create: %s\n", why); return 3; }

    /* per proof */
    qpgpu_challenger ch;
    uint64_t pih[4], caps[3][4 << 4], betas[4], gammas[4], alphas[4], zeta[2], g_zeta[2];
    if (cap_height > 4 || nch > 4) { fprintf(stderr, "cap_height / num_challenges beyond this example's buffers\n"); return 3; }
    {   /* hash_no_pad(public inputs): observe them, squeeze once; the digest is the head of the sponge */
        qpgpu_challenger_init(&ch);
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, pis, num_pis));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &pih[0]));
        memcpy(pih, ch.sponge_state, sizeof pih);
    }
    qpgpu_challenger_init(&ch);
    CHECK(qpgpu_oracle_commit(ctx, wires, num_wires, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 1, &o_w));
    CHECK(qpgpu_oracle_cap(o_w, caps[0], cap_words));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, digest, 4));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, pih, 4));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, caps[0], cap_words));
    for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &betas[k]));
    for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &gammas[k]));
    const uint32_t nzp = nch * (1 + npp), nq = nch * qdf;
    void *d_zs = NULL, *d_q = NULL;
    CHECK(qpgpu_malloc(ctx, (size_t)nzp * n * 8, &d_zs));
    CHECK(qpgpu_malloc(ctx, (size_t)nq * n * 8, &d_q));
    CHECK(qpgpu_stage_partial_products(plan, wires, 0, betas, gammas, d_zs));
    CHECK(qpgpu_oracle_commit(ctx, d_zs, nzp, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES | QPGPU_ORACLE_DEVICE_INPUT, 0, 2, &o_zs));
    CHECK(qpgpu_oracle_cap(o_zs, caps[1], cap_words));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, caps[1], cap_words));
    for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &alphas[k]));
    CHECK(qpgpu_stage_quotient(plan, o_w, o_zs, betas, gammas, alphas, pih, d_q));
    CHECK(qpgpu_oracle_commit(ctx, d_q, nq, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_COEFFS | QPGPU_ORACLE_DEVICE_INPUT, 0, 3, &o_q));
    CHECK(qpgpu_oracle_cap(o_q, caps[2], cap_words));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, caps[2], cap_words));
    CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &zeta[0]));
    CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &zeta[1]));
    const uint64_t g = root_of_unity(degree_bits);
    g_zeta[0] = mulmod(zeta[0], g); g_zeta[1] = mulmod(zeta[1], g);
    /* openings: every polynomial at zeta, the Zs also at g * zeta */
    qpgpu_oracle *os[4] = {o_cs, o_w, o_zs, o_q};
    const uint32_t counts[4] = {(uint32_t)ncs, num_wires, nzp, nq};
    const size_t n_open = ncs + num_wires + nzp + nq;
    uint64_t *open = malloc((n_open + nch) * 16), *at_zeta[4];
    {
        size_t off = 0;
        for (int i = 0; i < 4; i++) { at_zeta[i] = open + 2 * off; CHECK(qpgpu_oracle_eval(os[i], zeta, 0, counts[i], at_zeta[i])); off += counts[i]; }
    }
    uint64_t *zs_next = open + 2 * n_open;
    CHECK(qpgpu_oracle_eval(o_zs, g_zeta, 0, nch, zs_next));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, open, 2 * (n_open + nch)));
    /* ProofWithPublicInputs::to_bytes: caps, openings (Zs, Zs at g * zeta, partial products split out of one oracle), FRI, public inputs */
    size_t at = 0, fri_len = 0;
    for (int i = 0; i < 3; i++) at = put(mine, at, caps[i], cap_words);
    at = put(mine, at, at_zeta[0], 2 * ncs);
    at = put(mine, at, at_zeta[1], 2 * (size_t)num_wires);
    at = put(mine, at, at_zeta[2], 2 * (size_t)nch);
    at = put(mine, at, zs_next, 2 * (size_t)nch);
    at = put(mine, at, at_zeta[2] + 2 * nch, 2 * (size_t)nch * npp);
    at = put(mine, at, at_zeta[3], 2 * (size_t)nq);
    qpgpu_fri_batch fb[2];
    memset(fb, 0, sizeof fb);
    fb[0].point[0] = zeta[0]; fb[0].point[1] = zeta[1]; fb[0].num_ranges = 4;
    for (uint32_t i = 0; i < 4; i++) { fb[0].ranges[i].oracle = i; fb[0].ranges[i].first = 0; fb[0].ranges[i].count = counts[i]; }
    fb[1].point[0] = g_zeta[0]; fb[1].point[1] = g_zeta[1]; fb[1].num_ranges = 1;
    fb[1].ranges[0].oracle = 2; fb[1].ranges[0].first = 0; fb[1].ranges[0].count = nch;
    if (!stepwise) {
        CHECK(qpgpu_fri_prove(ctx, os, 4, fb, 2, &fp, &ch, mine + at, cap - at, &fri_len));
    } else {
        /* prove_openings with the transcript on this side: caps, query rounds, final polynomial, nonce (write_fri_proof order) */
        qpgpu_fri_session *fs = NULL;
        uint64_t alpha[2], beta[2], nonce = 0, response, idx[64];
        size_t n_final = 0, q_len = 0;
        uint8_t *o = mine + at;
        if (fp.num_query_rounds > 64) { fprintf(stderr, "num_query_rounds beyond this example's buffers\n"); return 3; }
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &alpha[0]));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &alpha[1]));
        CHECK(qpgpu_fri_begin(ctx, os, 4, fb, 2, &fp, alpha, &fs));
        for (unsigned r = 0; r < narity; r++) {
            CHECK(qpgpu_fri_round_commit(fs, (uint64_t *)o, cap_words));
            CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, (const uint64_t *)o, cap_words));
            o += cap_words * 8;
            CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &beta[0]));
            CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &beta[1]));
            CHECK(qpgpu_fri_round_fold(fs, beta));
        }
        unsigned folded = 0;
        for (unsigned r = 0; r < narity; r++) folded += fp.reduction_arity_bits[r];
        const size_t final_words = (size_t)2 << (degree_bits - folded), q_bytes = fp.num_query_rounds * qpgpu_fri_query_size(fs);
        uint64_t *final_poly = malloc(final_words * 8);
        CHECK(qpgpu_fri_final_poly(fs, final_poly, final_words, &n_final));
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, final_poly, 2 * n_final));
        CHECK(qpgpu_fri_grind(ctx, &ch, fp.proof_of_work_bits, &nonce));
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, &nonce, 1));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &response));
        for (unsigned q = 0; q < fp.num_query_rounds; q++) {
            CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &idx[q]));
            idx[q] %= (uint64_t)n << rate_bits;
        }
        CHECK(qpgpu_fri_open(fs, idx, fp.num_query_rounds, o, q_bytes, &q_len));
        memcpy(o + q_len, final_poly, final_words * 8);                  /* query rounds hold one-byte path lengths: no alignment here */
        memcpy(o + q_len + final_words * 8, &nonce, 8);
        free(final_poly);
        fri_len = (size_t)(o - (mine + at)) + q_len + final_words * 8 + 8;
        qpgpu_fri_session_free(fs);
    }
    at += fri_len;
    for (unsigned i = 0; i < num_pis; i++) { const uint64_t v = pis[i] % P; at = put(mine, at, &v, 1); }
    if (at != want_len || memcmp(mine, want, want_len)) { fprintf(stderr, "the staged proof differs from qpgpu_prove's\n"); return 4; }

    /* a witness that does not satisfy the circuit is refused at the quotient stage, and the plan stays usable */
    wires[3 * n + 20] = (wires[3 * n + 20] + 1) % P;                 /* arithmetic output of operation 0 on row 20 */
    qpgpu_oracle *o_bad = NULL;
    CHECK(qpgpu_oracle_commit(ctx, wires, num_wires, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 1, &o_bad));
    if (qpgpu_stage_quotient(plan, o_bad, o_zs, betas, gammas, alphas, pih, d_q) != QPGPU_EUNSAT) { fprintf(stderr, "missing EUNSAT\n"); return 5; }
    printf("refused: %s\n", qpgpu_last_error(ctx));
    CHECK(qpgpu_stage_quotient(plan, o_w, o_zs, betas, gammas, alphas, pih, d_q));

    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < at; i++) h = (h ^ mine[i]) * 1099511628211ull;
    printf("ok degree_bits=%u proof_bytes=%zu fnv1a=%016llx (staged flow%s == qpgpu_prove)\n", degree_bits, at, (unsigned long long)h,
           stepwise ? ", FRI step by step," : "");
    qpgpu_oracle_free(o_bad); qpgpu_oracle_free(o_q); qpgpu_oracle_free(o_zs); qpgpu_oracle_free(o_w);
    qpgpu_stage_plan_free(plan);                                       /* before the oracle it reads */
    qpgpu_oracle_free(o_cs);
    CHECK(qpgpu_free_scrubbed(ctx, d_zs, (size_t)nzp * n * 8));
    CHECK(qpgpu_free_scrubbed(ctx, d_q, (size_t)nq * n * 8));
    qpgpu_ctx_destroy(ctx);
    free(pack); free(wires); free(want); free(mine); free(open);
    return 0;
}

/* `<degree_bits> batch <N>`: N witnesses of one circuit through the stage flow in lockstep. Every array is [N][...], proof b first. */
static int run_batch(unsigned degree_bits, uint32_t B) {
    const unsigned num_wires = 135, num_routed = 80, num_pis = 21, flags = 3;
    qpgpu_ctx *ctx = NULL;
    if (B == 0 || B > 64) { fprintf(stderr, "batch: 1..64 in this example\n"); return 3; }
    if (qpgpu_ctx_create(0, &ctx)) { fprintf(stderr, "no gfx950 device: the library has no CPU fallback\n"); return 2; }
    const size_t n = (size_t)1 << degree_bits, mat = (size_t)num_wires * n;
    size_t words = qpgpu_synth_pack_words_ex(degree_bits, num_wires, num_routed, flags), got = 0;
    uint64_t *pack = malloc(words * 8), *wires = malloc((size_t)B * mat * 8), *pis = malloc((size_t)B * num_pis * 8);
    CHECK(qpgpu_synth_circuit_ex(degree_bits, num_wires, num_routed, num_pis, 42, flags, pack, words, &got, wires, pis));

    /* N different witnesses: the first one's free cells under other public inputs, completed by stage s1; then the reference
     * bytes from the all-in-one prover, which runs each stage once for the batch */
    qpgpu_circuit *circuit = NULL;
    CHECK(qpgpu_circuit_load_batch(ctx, pack, got, B, &circuit));
    CHECK(qpgpu_circuit_set_witness_check(circuit, 1));
    const size_t cap = qpgpu_proof_size(circuit);
    for (uint32_t b = 1; b < B; b++) {
        memcpy(wires + b * mat, wires, mat * 8);
        for (unsigned i = 0; i < num_pis; i++) pis[b * num_pis + i] = (pis[i] + (uint64_t)b * (i + 1)) % P;
        CHECK(qpgpu_generate_witness(circuit, wires + b * mat, pis + b * num_pis));
    }
    void *d_wires = NULL;
    CHECK(qpgpu_malloc(ctx, (size_t)B * mat * 8, &d_wires));
    CHECK(qpgpu_memcpy_h2d(ctx, d_wires, wires, (size_t)B * mat * 8));
    uint8_t *want = malloc((size_t)B * cap), *mine = malloc((size_t)B * cap);
    const uint64_t *w_ptrs[64], *pi_ptrs[64], *host_ptrs[64];
    uint8_t *want_ptrs[64], *fri_ptrs[64];
    size_t want_lens[64], fri_lens[64], at[64];
    for (uint32_t b = 0; b < B; b++) {
        w_ptrs[b] = (const uint64_t *)d_wires + b * mat; host_ptrs[b] = wires + b * mat; pi_ptrs[b] = pis + b * num_pis; want_ptrs[b] = want + b * cap;
    }
    CHECK(qpgpu_prove_batch_dev(circuit, w_ptrs, B, pi_ptrs, want_ptrs, cap, want_lens));
    qpgpu_circuit_free(circuit);

    const unsigned nconst = (unsigned)pack[4], nsel = (unsigned)pack[5], nch = (unsigned)pack[6], qdf = (unsigned)pack[7], npp = (unsigned)pack[8];
    const unsigned rate_bits = (unsigned)pack[10], cap_height = (unsigned)pack[11], ngates = (unsigned)pack[16], narity = (unsigned)pack[17];
    const size_t hdr_end = 18 + narity + 8 * (size_t)ngates + num_routed + 4, ncs = nsel + nconst + num_routed, cap_words = (size_t)4 << cap_height;
    const uint64_t *digest = pack + hdr_end - 4, *cs_values = pack + hdr_end;
    qpgpu_fri_params fp = {rate_bits, cap_height, (uint32_t)pack[12], (uint32_t)pack[13], narity, {0}};
    for (unsigned i = 0; i < narity; i++) fp.reduction_arity_bits[i] = (uint32_t)pack[18 + i];

    /* per circuit: the shared constants/sigmas commitment (one proof) and a plan whose workspace holds B proofs */
    qpgpu_oracle *o_cs = NULL, *o_w = NULL, *o_zs = NULL, *o_q = NULL;
    qpgpu_stage_plan *plan = NULL;
    char why[QPGPU_STAGE_ERR_CAP];
    CHECK(qpgpu_oracle_commit(ctx, cs_values, (uint32_t)ncs, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 0, &o_cs));
    if (qpgpu_stage_plan_create_batch(ctx, pack, hdr_end, o_cs, B, &plan, why)) { fprintf(stderr, "stage_plan_create_batch: %s\n", why); return 3; }

    /* per level of leaves: B transcripts on this side, one call per stage */
    qpgpu_challenger *ch = malloc(B * sizeof *ch);
    const uint32_t nzp = nch * (1 + npp), nq = nch * qdf;
    uint64_t *pih = malloc((size_t)B * 4 * 8), *caps = malloc(3 * (size_t)B * cap_words * 8), *chal = malloc(3 * (size_t)B * nch * 8);
    uint64_t *betas = chal, *gammas = chal + (size_t)B * nch, *alphas = chal + 2 * (size_t)B * nch;
    uint64_t *w_caps = caps, *zs_caps = caps + B * cap_words, *q_caps = caps + 2 * B * cap_words;
    uint64_t *points = malloc(2 * (size_t)B * 2 * 8), *zetas = points, *g_zetas = points + 2 * (size_t)B;   /* [2 opening batches][B][2] */
    for (uint32_t b = 0; b < B; b++) {
        qpgpu_challenger_init(&ch[b]);
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], pi_ptrs[b], num_pis));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &pih[4 * b]));
        memcpy(pih + 4 * b, ch[b].sponge_state, 32);
        qpgpu_challenger_init(&ch[b]);
    }
    /* the wire matrices lie back to back on the device: committed and read by s5 in place */
    CHECK(qpgpu_oracle_commit_batch(ctx, w_ptrs, B, num_wires, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES | QPGPU_ORACLE_DEVICE_INPUT, 0, 1, &o_w));
    CHECK(qpgpu_oracle_cap(o_w, w_caps, B * cap_words));
    for (uint32_t b = 0; b < B; b++) {
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], digest, 4));
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], pih + 4 * b, 4));
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], w_caps + b * cap_words, cap_words));
        for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &betas[b * nch + k]));
        for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &gammas[b * nch + k]));
    }
    void *d_zs = NULL, *d_q = NULL;
    CHECK(qpgpu_malloc(ctx, (size_t)B * nzp * n * 8, &d_zs));
    CHECK(qpgpu_malloc(ctx, (size_t)B * nq * n * 8, &d_q));
    const uint64_t *zs_ptrs[64], *q_ptrs[64];
    for (uint32_t b = 0; b < B; b++) { zs_ptrs[b] = (const uint64_t *)d_zs + (size_t)b * nzp * n; q_ptrs[b] = (const uint64_t *)d_q + (size_t)b * nq * n; }
    CHECK(qpgpu_stage_partial_products_batch(plan, w_ptrs, B, 1, betas, gammas, d_zs));
    CHECK(qpgpu_oracle_commit_batch(ctx, zs_ptrs, B, nzp, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES | QPGPU_ORACLE_DEVICE_INPUT, 0, 2, &o_zs));
    CHECK(qpgpu_oracle_cap(o_zs, zs_caps, B * cap_words));
    for (uint32_t b = 0; b < B; b++) {
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], zs_caps + b * cap_words, cap_words));
        for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &alphas[b * nch + k]));
    }
    CHECK(qpgpu_stage_quotient_batch(plan, o_w, o_zs, B, betas, gammas, alphas, pih, d_q));
    CHECK(qpgpu_oracle_commit_batch(ctx, q_ptrs, B, nq, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_COEFFS | QPGPU_ORACLE_DEVICE_INPUT, 0, 3, &o_q));
    CHECK(qpgpu_oracle_cap(o_q, q_caps, B * cap_words));
    const uint64_t g = root_of_unity(degree_bits);
    for (uint32_t b = 0; b < B; b++) {
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], q_caps + b * cap_words, cap_words));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &zetas[2 * b]));
        CHECK(qpgpu_ctx_challenger_get(ctx, &ch[b], &zetas[2 * b + 1]));
        g_zetas[2 * b] = mulmod(zetas[2 * b], g); g_zetas[2 * b + 1] = mulmod(zetas[2 * b + 1], g);
    }
    /* openings: one call per oracle for all proofs; the shared constants/sigmas oracle holds one proof and is asked per point */
    qpgpu_oracle *os[4] = {o_cs, o_w, o_zs, o_q};
    const uint32_t counts[4] = {(uint32_t)ncs, num_wires, nzp, nq};
    uint64_t *ev[4], *zs_next = malloc((size_t)B * nch * 16);
    for (int i = 0; i < 4; i++) ev[i] = malloc((size_t)B * counts[i] * 16);
    for (uint32_t b = 0; b < B; b++) CHECK(qpgpu_oracle_eval(o_cs, zetas + 2 * b, 0, counts[0], ev[0] + (size_t)b * counts[0] * 2));
    for (int i = 1; i < 4; i++) CHECK(qpgpu_oracle_eval_batch(os[i], zetas, 0, counts[i], ev[i]));
    CHECK(qpgpu_oracle_eval_batch(o_zs, g_zetas, 0, nch, zs_next));
    for (uint32_t b = 0; b < B; b++) {
        uint8_t *out = mine + b * cap;
        for (int i = 0; i < 4; i++) CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], ev[i] + (size_t)b * counts[i] * 2, 2 * (size_t)counts[i]));
        CHECK(qpgpu_ctx_challenger_observe(ctx, &ch[b], zs_next + (size_t)b * nch * 2, 2 * (size_t)nch));
        const uint64_t *zs_b = ev[2] + (size_t)b * nzp * 2;
        size_t a = 0;
        a = put(out, a, w_caps + b * cap_words, cap_words); a = put(out, a, zs_caps + b * cap_words, cap_words); a = put(out, a, q_caps + b * cap_words, cap_words);
        a = put(out, a, ev[0] + (size_t)b * ncs * 2, 2 * ncs);
        a = put(out, a, ev[1] + (size_t)b * num_wires * 2, 2 * (size_t)num_wires);
        a = put(out, a, zs_b, 2 * (size_t)nch);
        a = put(out, a, zs_next + (size_t)b * nch * 2, 2 * (size_t)nch);
        a = put(out, a, zs_b + 2 * nch, 2 * (size_t)nch * npp);
        a = put(out, a, ev[3] + (size_t)b * nq * 2, 2 * (size_t)nq);
        at[b] = a; fri_ptrs[b] = out + a;
    }
    qpgpu_fri_batch fb[2];
    memset(fb, 0, sizeof fb);                                           /* the point fields are not read: `points` carries them */
    fb[0].num_ranges = 4;
    for (uint32_t i = 0; i < 4; i++) { fb[0].ranges[i].oracle = i; fb[0].ranges[i].first = 0; fb[0].ranges[i].count = counts[i]; }
    fb[1].num_ranges = 1;
    fb[1].ranges[0].oracle = 2; fb[1].ranges[0].first = 0; fb[1].ranges[0].count = nch;
    size_t fri_cap = cap;
    for (uint32_t b = 0; b < B; b++) if (cap - at[b] < fri_cap) fri_cap = cap - at[b];
    CHECK(qpgpu_fri_prove_batch(ctx, os, 4, fb, 2, points, B, &fp, ch, fri_ptrs, fri_cap, fri_lens));
    uint64_t h = 1469598103934665603ull;
    for (uint32_t b = 0; b < B; b++) {
        uint8_t *out = mine + b * cap;
        size_t a = at[b] + fri_lens[b];
        for (unsigned i = 0; i < num_pis; i++) { const uint64_t v = pi_ptrs[b][i] % P; a = put(out, a, &v, 1); }
        if (a != want_lens[b] || memcmp(out, want_ptrs[b], a)) { fprintf(stderr, "proof %u of the lockstep flow differs from qpgpu_prove_batch_dev's\n", b); return 4; }
        for (size_t i = 0; i < a; i++) h = (h ^ out[i]) * 1099511628211ull;
    }
    if (B > 1 && want_lens[0] == want_lens[1] && !memcmp(want_ptrs[0], want_ptrs[1], want_lens[0])) { fprintf(stderr, "the witnesses do not differ\n"); return 5; }
    printf("ok degree_bits=%u proof_bytes=%zu fnv1a=%016llx (staged flow in lockstep, %u proofs, == qpgpu_prove_batch_dev)\n", degree_bits, want_lens[0],
           (unsigned long long)h, B);
    qpgpu_oracle_free(o_q); qpgpu_oracle_free(o_zs); qpgpu_oracle_free(o_w);
    qpgpu_stage_plan_free(plan);                                       /* before the oracle it reads */
    qpgpu_oracle_free(o_cs);
    CHECK(qpgpu_free_scrubbed(ctx, d_zs, (size_t)B * nzp * n * 8));
    CHECK(qpgpu_free_scrubbed(ctx, d_q, (size_t)B * nq * n * 8));
    CHECK(qpgpu_free_scrubbed(ctx, d_wires, (size_t)B * mat * 8));
    qpgpu_ctx_destroy(ctx);
    for (int i = 0; i < 4; i++) free(ev[i]);
    free(zs_next); free(points); free(chal); free(caps); free(pih); free(ch); free(pack); free(wires); free(pis); free(want); free(mine);
    (void)host_ptrs;
    return 0;
}
