/*
 * sharded_commit_example.c — one polynomial commitment across several contexts from plain C: qpgpu_oracle_commit_sharded splits the
 * leaves of the commitment by cosets over the contexts it is given (on different devices, or, as here on a one-GPU machine, two
 * contexts of device 0), and everything after it — the cap, openings, the FRI opening proof and its verification — is used as
 * with an oracle of one context. The example commits, compares the cap with qpgpu_oracle_commit's, opens the first and the last
 * leaf of each shard, proves the openings at a point with qpgpu_fri_prove and checks the proof with qpgpu_fri_verify.
 *
 *   gcc -O2 -I include examples/sharded_commit_example.c -L qp-zk-circuits_amd -lqpgpu -Wl,-rpath,$PWD/qp-zk-circuits_amd -o /tmp/sharded_commit_example
 *   /tmp/sharded_commit_example [degree_bits]          (default 10)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qpgpu.h"
#include "qpgpu_verify.h"

#define SHARDS 2
#define POLYS 7
#define RATE_BITS 3
#define CAP_HEIGHT 4
#define QUERIES 6

#define CHECK(ctx, call) do { int rc_ = (call); if (rc_ != QPGPU_OK) { \
    fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, qpgpu_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
    const unsigned d = argc > 1 ? (unsigned)atoi(argv[1]) : 10;
    if (d < 4 || d > 18) { fprintf(stderr, "degree_bits 4..18\n"); return 2; }
    const size_t n = (size_t)1 << d, N = n << RATE_BITS;
    const uint64_t P = 0xFFFFFFFF00000001ull;

    qpgpu_ctx *ctxs[SHARDS] = {0};
    for (int g = 0; g < SHARDS; g++)
        if (qpgpu_ctx_create(0, &ctxs[g]) != QPGPU_OK) { fprintf(stderr, "no gfx950 device\n"); return 1; }
    qpgpu_ctx *home = ctxs[0];

    /* values on the subgroup, column-major */
    uint64_t *polys = malloc(POLYS * n * 8);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < POLYS * n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; polys[i] = x % P; }

    qpgpu_oracle *sharded = NULL, *plain = NULL;
    CHECK(home, qpgpu_oracle_commit_sharded(ctxs, SHARDS, polys, POLYS, d, RATE_BITS, CAP_HEIGHT, QPGPU_ORACLE_VALUES, 0, 0, &sharded));
    CHECK(home, qpgpu_oracle_commit(home, polys, POLYS, d, RATE_BITS, CAP_HEIGHT, QPGPU_ORACLE_VALUES, 0, 0, &plain));
    uint64_t cap[4 << CAP_HEIGHT], cap_plain[4 << CAP_HEIGHT];
    CHECK(home, qpgpu_oracle_cap(sharded, cap, 4 << CAP_HEIGHT));
    CHECK(home, qpgpu_oracle_cap(plain, cap_plain, 4 << CAP_HEIGHT));
    if (memcmp(cap, cap_plain, sizeof cap)) { fprintf(stderr, "the sharded cap differs from qpgpu_oracle_commit's\n"); return 1; }
    printf("%u shards, cap == qpgpu_oracle_commit's\n", qpgpu_oracle_shards(sharded));

    /* the first and last leaf of every shard, rows and paths, against the one-context oracle */
    uint64_t idx[2 * SHARDS];
    for (uint32_t g = 0; g < SHARDS; g++) {
        uint64_t first, num;
        CHECK(home, qpgpu_oracle_shard_range(sharded, g, &first, &num));
        printf("shard %u: leaves [%llu, %llu)\n", g, (unsigned long long)first, (unsigned long long)(first + num));
        idx[2 * g] = first; idx[2 * g + 1] = first + num - 1;
    }
    const size_t width = qpgpu_oracle_leaf_width(sharded), plen = d + RATE_BITS - CAP_HEIGHT;
    uint64_t *rows = malloc(2 * (2 * SHARDS) * width * 8), *paths = malloc(2 * (2 * SHARDS) * plen * 32);
    CHECK(home, qpgpu_oracle_open(sharded, idx, 2 * SHARDS, rows, paths));
    CHECK(home, qpgpu_oracle_open(plain, idx, 2 * SHARDS, rows + 2 * SHARDS * width, paths + 2 * SHARDS * plen * 4));
    if (memcmp(rows, rows + 2 * SHARDS * width, 2 * SHARDS * width * 8) || memcmp(paths, paths + 2 * SHARDS * plen * 4, 2 * SHARDS * plen * 32)) {
        fprintf(stderr, "an opening of the sharded oracle differs\n"); return 1;
    }
    printf("openings == qpgpu_oracle_commit's\n");
    qpgpu_oracle_free(plain);

    /* the FRI opening proof of all columns at one point; ctx is the sharded oracle's home context */
    qpgpu_fri_batch batch;
    memset(&batch, 0, sizeof batch);
    batch.point[0] = 0x1234567; batch.point[1] = 0x89ABCDE;
    batch.num_ranges = 1; batch.ranges[0].oracle = 0; batch.ranges[0].first = 0; batch.ranges[0].count = POLYS;
    qpgpu_fri_params prm;
    memset(&prm, 0, sizeof prm);
    prm.rate_bits = RATE_BITS; prm.cap_height = CAP_HEIGHT; prm.proof_of_work_bits = 8; prm.num_query_rounds = QUERIES;
    prm.num_reduction_rounds = 1; prm.reduction_arity_bits[0] = d >= 8 ? 4 : 2;
    uint64_t openings[2 * POLYS];
    CHECK(home, qpgpu_oracle_eval(sharded, batch.point, 0, POLYS, openings));

    qpgpu_challenger ch, start;
    qpgpu_challenger_init(&ch);
    CHECK(home, qpgpu_ctx_challenger_observe(home, &ch, cap, 4 << CAP_HEIGHT));
    CHECK(home, qpgpu_ctx_challenger_observe(home, &ch, openings, 2 * POLYS));
    start = ch;
    const size_t size = qpgpu_fri_proof_size(&sharded, 1, &prm);
    uint8_t *proof = malloc(size);
    size_t len = 0;
    CHECK(home, qpgpu_fri_prove(home, &sharded, 1, &batch, 1, &prm, &ch, proof, size, &len));
    printf("FRI proof: %zu bytes\n", len);

    qpgpu_fri_oracle_shape shape = {POLYS, 0};
    qpgpu_fri_instance inst;
    memset(&inst, 0, sizeof inst);
    inst.degree_bits = d; inst.num_oracles = 1; inst.oracles = &shape; inst.num_batches = 1; inst.batches = &batch; inst.params = prm;
    qpgpu_fri_verifier *fv = NULL;
    char err[256] = "";
    if (qpgpu_fri_verifier_create(&inst, qpgpu_ctx_get_hasher(home), NULL, 0, &fv, err) != QPGPU_OK) { fprintf(stderr, "verifier: %s\n", err); return 1; }
    uint64_t alpha[2], betas[2 * 16], pow_response, indices[QUERIES];
    if (qpgpu_fri_verifier_challenges(fv, &start, proof, len, alpha, betas, &pow_response, indices, err) != QPGPU_OK) { fprintf(stderr, "challenges: %s\n", err); return 1; }
    const uint64_t *caps[1] = {cap};
    int rc = qpgpu_fri_verify(fv, caps, batch.point, openings, alpha, betas, pow_response, indices, proof, len, err);
    if (rc != QPGPU_OK) { fprintf(stderr, "qpgpu_fri_verify rejected the proof: %d (%s)\n", rc, err); return 1; }
    printf("qpgpu_fri_verify: accepted (queries at");
    for (int q = 0; q < QUERIES; q++) printf(" %llu", (unsigned long long)(indices[q] % N));
    printf(")\n");
    proof[len / 2] ^= 1;
    rc = qpgpu_fri_verify(fv, caps, batch.point, openings, alpha, betas, pow_response, indices, proof, len, err);
    if (rc == QPGPU_OK) { fprintf(stderr, "a broken proof was accepted\n"); return 1; }
    printf("a flipped proof byte: rejected (%s)\n", err);

    qpgpu_fri_verifier_free(fv);
    qpgpu_oracle_free(sharded);
    for (int g = 0; g < SHARDS; g++) qpgpu_ctx_destroy(ctxs[g]);
    free(polys); free(rows); free(paths); free(proof);
    printf("sharded commitment: ok\n");
    return 0;
}
