/*
 * explain_witness_example.c — what to do with QPGPU_EUNSAT, from plain C: build a synthetic circuit, flip one cell of a
 * PoseidonGate row, let qpgpu_prove refuse the witness ("gate constraints fail at row N"), then ask
 * qpgpu_circuit_explain_witness which gate, which constraints and which cells, and print qpgpu_witness_finding_format's lines.
 * Exits 0 only if the findings name the flipped row and its gate, and a flipped routed cell comes back as a copy finding.
 *
 *   gcc -O2 -I include examples/explain_witness_example.c -L qp-zk-circuits_amd -lqpgpu -Wl,-rpath,$PWD/qp-zk-circuits_amd -o /tmp/explain_example
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qpgpu.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, ctx ? qpgpu_last_error(ctx) : "?"); return 1; } } while (0)
#define CAP 256

int main(int argc, char **argv) {
    const unsigned degree_bits = argc > 1 ? (unsigned)atoi(argv[1]) : 7;
    const unsigned num_wires = 135, num_routed = 80, num_pis = 21, flags = 3; /* Poseidon + BaseSum rows */
    const size_t n = (size_t)1 << degree_bits;
    qpgpu_ctx *ctx = NULL;
    if (qpgpu_ctx_create(0, &ctx)) { fprintf(stderr, "no gfx950 device: the library has no CPU fallback\n"); return 2; }

    size_t words = qpgpu_synth_pack_words_ex(degree_bits, num_wires, num_routed, flags), got = 0;
    uint64_t *pack = malloc(words * 8), *wires = malloc(num_wires * n * 8), pis[21];
    CHECK(qpgpu_synth_circuit_ex(degree_bits, num_wires, num_routed, num_pis, 42, flags, pack, words, &got, wires, pis));
    qpgpu_circuit *circuit = NULL;
    CHECK(qpgpu_circuit_load(ctx, pack, got, &circuit));

    static qpgpu_witness_finding found[CAP];
    size_t count = 99;
    uint64_t failing = 99, mismatches = 99;
    char line[256];
    /* the witness as generated satisfies the circuit: nothing to report */
    CHECK(qpgpu_circuit_explain_witness(circuit, wires, 0, pis, 8, 0, found, CAP, &count, &failing, &mismatches));
    if (count || failing || mismatches) { fprintf(stderr, "findings on a satisfied witness\n"); return 3; }

    /* a PoseidonGate row (gate type 4), and its last wire: an S-box input of the last full round, not routed */
    size_t n_hash = 0;
    CHECK(qpgpu_circuit_gate_rows(circuit, 4, NULL, 0, &n_hash));
    if (n_hash == 0) { fprintf(stderr, "no PoseidonGate row\n"); return 3; }
    uint32_t *hash_rows = malloc(n_hash * sizeof *hash_rows);
    CHECK(qpgpu_circuit_gate_rows(circuit, 4, hash_rows, n_hash, &n_hash));
    const uint64_t row = hash_rows[0];
    free(hash_rows);
    wires[(size_t)134 * n + row] ^= 1;

    /* what the prover says today */
    CHECK(qpgpu_circuit_set_witness_check(circuit, 1));
    size_t cap = qpgpu_proof_size(circuit), len = 0;
    uint8_t *proof = malloc(cap);
    if (qpgpu_prove(circuit, wires, pis, proof, cap, &len) != QPGPU_EUNSAT) { fprintf(stderr, "the flipped witness was not refused\n"); return 4; }
    printf("prove: %s\n", qpgpu_last_error(ctx));

    /* and what explain_witness adds */
    CHECK(qpgpu_circuit_explain_witness(circuit, wires, 0, pis, 8, 0, found, CAP, &count, &failing, &mismatches));
    if (failing != 1 || mismatches != 0 || count == 0) { fprintf(stderr, "expected one failing row and no copy mismatch, got %llu / %llu / %zu findings\n", (unsigned long long)failing, (unsigned long long)mismatches, count); return 5; }
    for (size_t i = 0; i < count; i++) {
        CHECK(qpgpu_witness_finding_format(pack, got, &found[i], line, sizeof line));
        printf("%s\n", line);
        if (found[i].kind != QPGPU_FINDING_GATE || found[i].row != row || !strstr(line, "(Poseidon)")) { fprintf(stderr, "finding %zu does not name row %llu's PoseidonGate\n", i, (unsigned long long)row); return 5; }
    }
    wires[(size_t)134 * n + row] ^= 1;

    /* a routed cell that is off: wire 0 of that row. Whichever side of its copy class the cell is, copy findings name it */
    wires[row] ^= 1;
    CHECK(qpgpu_circuit_explain_witness(circuit, wires, 0, pis, 8, 0, found, CAP, &count, &failing, &mismatches));
    int named = 0;
    for (size_t i = 0; i < count; i++) {
        CHECK(qpgpu_witness_finding_format(pack, got, &found[i], line, sizeof line));
        printf("%s\n", line);
        if (found[i].kind == QPGPU_FINDING_COPY && ((found[i].row == row && found[i].wire == 0) || (found[i].row_b == row && found[i].wire_b == 0))) named++;
    }
    if (failing == 0 && mismatches == 0) { fprintf(stderr, "a flipped routed cell went unnoticed\n"); return 6; }
    if (mismatches && !named) { fprintf(stderr, "the copy findings do not name the flipped cell\n"); return 6; }

    printf("ok degree_bits=%u row=%llu\n", degree_bits, (unsigned long long)row);
    qpgpu_circuit_free(circuit);
    qpgpu_ctx_destroy(ctx);
    free(pack); free(wires); free(proof);
    return 0;
}
