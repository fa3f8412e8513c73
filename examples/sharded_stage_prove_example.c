/*
 * sharded_stage_prove_example.c — the stage flow of stage_prove_example.c with every commitment split by cosets over two contexts
 * (here both on device 0; on a box with several GPUs, one context per device): commit -> partial products -> quotient ->
 * openings -> FRI, every LDE and every Merkle tree sharded. The four commitments go through qpgpu_oracle_commit_sharded, the plan
 * comes from qpgpu_stage_plan_create_sharded, and qpgpu_stage_quotient evaluates the quotient on the shards: each context works on
 * its own slice of the three LDEs, the home context merges the shards' coefficients into the chunks. The assembled bytes are
 * compared with qpgpu_prove's and verified with qpgpu_verifier_verify. One line per check.
 *
 *   gcc -O2 -I include examples/sharded_stage_prove_example.c -L qp-zk-circuits_amd -lqpgpu -Wl,-rpath,$PWD/qp-zk-circuits_amd -o /tmp/sharded_stage_prove_example
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qpgpu.h"
#include "qpgpu_verify.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, ctx ? qpgpu_last_error(ctx) : "?"); return 1; } } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ull;
static uint64_t mulmod(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % P); }
static uint64_t root_of_unity(unsigned bits) {
    uint64_t r = 7277203076849721926ull;
    for (unsigned i = bits; i < 32; i++) r = mulmod(r, r);
    return r;
}
static size_t put(uint8_t *out, size_t at, const uint64_t *v, size_t n) { memcpy(out + at, v, n * 8); return at + n * 8; }

int main(int argc, char **argv) {
    unsigned degree_bits = argc > 1 ? (unsigned)atoi(argv[1]) : 10;
    const unsigned num_wires = 135, num_routed = 80, num_pis = 21, flags = 3; /* Poseidon + BaseSum rows */
    enum { G = 2 };
    qpgpu_ctx *ctxs[G] = {NULL, NULL}, *ctx = NULL;
    for (int i = 0; i < G; i++)
        if (qpgpu_ctx_create(0, &ctxs[i])) { fprintf(stderr, "no gfx950 device: the library has no CPU fallback\n"); return 2; }
    ctx = ctxs[0];                                                      /* the home context: every call below is made on it */

    size_t words = qpgpu_synth_pack_words_ex(degree_bits, num_wires, num_routed, flags), got = 0;
    uint64_t *pack = malloc(words * 8), *wires = malloc((size_t)num_wires * 8 << degree_bits), pis[21];
    CHECK(qpgpu_synth_circuit_ex(degree_bits, num_wires, num_routed, num_pis, 42, flags, pack, words, &got, wires, pis));

    /* the reference bytes: the all-in-one prover on one context */
    qpgpu_circuit *circuit = NULL;
    CHECK(qpgpu_circuit_load(ctx, pack, got, &circuit));
    const size_t cap = qpgpu_proof_size(circuit);
    size_t want_len = 0;
    uint8_t *want = malloc(cap), *mine = malloc(cap);
    CHECK(qpgpu_prove(circuit, wires, pis, want, cap, &want_len));
    qpgpu_circuit_free(circuit);

    const size_t n = (size_t)1 << degree_bits;
    const unsigned nconst = (unsigned)pack[4], nsel = (unsigned)pack[5], nch = (unsigned)pack[6], qdf = (unsigned)pack[7], npp = (unsigned)pack[8];
    const unsigned rate_bits = (unsigned)pack[10], cap_height = (unsigned)pack[11], ngates = (unsigned)pack[16], narity = (unsigned)pack[17];
    const size_t hdr_end = 18 + narity + 8 * (size_t)ngates + num_routed + 4, ncs = nsel + nconst + num_routed, cap_words = (size_t)4 << cap_height;
    const uint64_t *digest = pack + hdr_end - 4, *cs_values = pack + hdr_end;
    qpgpu_fri_params fp = {rate_bits, cap_height, (uint32_t)pack[12], (uint32_t)pack[13], narity, {0}};
    for (unsigned i = 0; i < narity; i++) fp.reduction_arity_bits[i] = (uint32_t)pack[18 + i];

    /* per circuit: the sharded constants/sigmas commitment and the plan over it */
    qpgpu_oracle *o_cs = NULL, *o_w = NULL, *o_zs = NULL, *o_q = NULL;
    qpgpu_stage_plan *plan = NULL;
    char why[QPGPU_STAGE_ERR_CAP];
    CHECK(qpgpu_oracle_commit_sharded(ctxs, G, cs_values, (uint32_t)ncs, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 0, &o_cs));
    if (qpgpu_stage_plan_create(ctx, pack, hdr_end, o_cs, &plan, why) != QPGPU_EINVAL || plan) { fprintf(stderr, "a plain plan took a sharded oracle\n"); return 3; }
    printf("qpgpu_stage_plan_create refuses it: %s\n", why);
    if (qpgpu_stage_plan_create_sharded(ctx, pack, hdr_end, o_cs, &plan, why)) { fprintf(stderr, "stage_plan_create_sharded: %s\n", why); return 3; }
    printf("plan over %u shards\n", qpgpu_stage_plan_shards(plan));

    /* per proof */
    qpgpu_challenger ch;
    uint64_t pih[4], caps[4][4 << 4], betas[4], gammas[4], alphas[4], zeta[2], g_zeta[2];
    if (cap_height > 4 || nch > 4) { fprintf(stderr, "cap_height / num_challenges beyond this example's buffers\n"); return 3; }
    qpgpu_challenger_init(&ch);
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, pis, num_pis));
    CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &pih[0]));
    memcpy(pih, ch.sponge_state, sizeof pih);
    qpgpu_challenger_init(&ch);
    CHECK(qpgpu_oracle_commit_sharded(ctxs, G, wires, num_wires, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 1, &o_w));
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
    CHECK(qpgpu_stage_partial_products(plan, wires, 0, betas, gammas, d_zs));          /* on the home context alone */
    CHECK(qpgpu_oracle_commit_sharded(ctxs, G, d_zs, nzp, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES | QPGPU_ORACLE_DEVICE_INPUT, 0, 2, &o_zs));
    CHECK(qpgpu_oracle_cap(o_zs, caps[1], cap_words));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, caps[1], cap_words));
    for (unsigned k = 0; k < nch; k++) CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &alphas[k]));
    CHECK(qpgpu_stage_quotient(plan, o_w, o_zs, betas, gammas, alphas, pih, d_q));      /* on the shards, merged on the home context */
    printf("quotient on %u shards: done\n", qpgpu_stage_plan_shards(plan));
    CHECK(qpgpu_oracle_commit_sharded(ctxs, G, d_q, nq, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_COEFFS | QPGPU_ORACLE_DEVICE_INPUT, 0, 3, &o_q));
    CHECK(qpgpu_oracle_cap(o_q, caps[2], cap_words));
    CHECK(qpgpu_ctx_challenger_observe(ctx, &ch, caps[2], cap_words));
    CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &zeta[0]));
    CHECK(qpgpu_ctx_challenger_get(ctx, &ch, &zeta[1]));
    const uint64_t g = root_of_unity(degree_bits);
    g_zeta[0] = mulmod(zeta[0], g); g_zeta[1] = mulmod(zeta[1], g);
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
    CHECK(qpgpu_fri_prove(ctx, os, 4, fb, 2, &fp, &ch, mine + at, cap - at, &fri_len));
    at += fri_len;
    for (unsigned i = 0; i < num_pis; i++) { const uint64_t v = pis[i] % P; at = put(mine, at, &v, 1); }
    if (at != want_len || memcmp(mine, want, want_len)) { fprintf(stderr, "the sharded staged proof differs from qpgpu_prove's\n"); return 4; }
    printf("sharded staged flow == qpgpu_prove: %zu bytes\n", at);

    {   /* the library's host verifier, verifier data from the sharded constants/sigmas commitment's cap */
        qpgpu_verifier *v = NULL;
        char verr[QPGPU_VERIFY_ERR_CAP];
        CHECK(qpgpu_oracle_cap(o_cs, caps[3], cap_words));
        if (qpgpu_verifier_create(pack, got, caps[3], cap_words, 0, NULL, 0, &v, verr)) { fprintf(stderr, "verifier: %s\n", verr); return 6; }
        if (qpgpu_verifier_verify(v, mine, at, verr)) { fprintf(stderr, "verifier: %s\n", verr); return 6; }
        printf("qpgpu_verifier_verify: accepted\n");
        qpgpu_verifier_free(v);
    }

    /* a witness that does not satisfy the circuit is refused at the quotient stage, and the plan stays usable */
    wires[3 * n + 20] = (wires[3 * n + 20] + 1) % P;                 /* arithmetic output of operation 0 on row 20 */
    qpgpu_oracle *o_bad = NULL;
    CHECK(qpgpu_oracle_commit_sharded(ctxs, G, wires, num_wires, degree_bits, rate_bits, cap_height, QPGPU_ORACLE_VALUES, 0, 1, &o_bad));
    if (qpgpu_stage_quotient(plan, o_bad, o_zs, betas, gammas, alphas, pih, d_q) != QPGPU_EUNSAT) { fprintf(stderr, "missing EUNSAT\n"); return 5; }
    printf("refused: %s\n", qpgpu_last_error(ctx));
    CHECK(qpgpu_stage_quotient(plan, o_w, o_zs, betas, gammas, alphas, pih, d_q));

    printf("sharded stage flow: ok\n");
    qpgpu_oracle_free(o_bad); qpgpu_oracle_free(o_q); qpgpu_oracle_free(o_zs); qpgpu_oracle_free(o_w);
    qpgpu_stage_plan_free(plan);                                       /* before the oracle it reads */
    qpgpu_oracle_free(o_cs);
    CHECK(qpgpu_free_scrubbed(ctx, d_zs, (size_t)nzp * n * 8));
    CHECK(qpgpu_free_scrubbed(ctx, d_q, (size_t)nq * n * 8));
    for (int i = G - 1; i >= 0; i--) qpgpu_ctx_destroy(ctxs[i]);
    free(pack); free(wires); free(want); free(mine); free(open);
    return 0;
}
