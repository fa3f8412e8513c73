// fri_verify_check.cpp — the host FRI verifier (qp-zk-circuits_amd/csrc/fri_verify.cpp and the query loop in verifier.cpp) on
// inputs no prover made: for a spread of instances (no rounds, one-bit rounds, a 256-ary round, blinded and narrow oracles, split
// ranges, a tree that is its cap), proofs of the right length filled with random canonical words, with every path-length byte
// right and then with each one in turn wrong or out of range. Every call must return a verdict (QPGPU_EVERIFY with a text) and
// read nothing outside the proof, the caps and the arrays it was given: host only, meant to be built with
// -fsanitize=address,undefined (the buffers are heap blocks of exactly the stated sizes):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I qp-zk-circuits_amd/csrc \
//       tools/host_checks/fri_verify_check.cpp qp-zk-circuits_amd/csrc/{fri_verify,verifier,circuit,poseidon_constants}.cpp
// tests/test_fri_verify_host.py builds and runs it that way.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "../../include/qpgpu.h"
#include "../../include/qpgpu_verify.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ULL;

struct Shape {
    uint32_t degree_bits, rate_bits, cap_height;
    std::vector<uint32_t> arity;
    std::vector<qpgpu_fri_oracle_shape> oracles;
    std::vector<std::vector<qpgpu_fri_range>> batches;
};

int main() {
    const std::vector<Shape> shapes = {
        {5, 1, 0, {}, {{3, 0}}, {{{0, 0, 3}}}},
        {5, 3, 2, {1}, {{1, 0}, {4, 0}}, {{{0, 0, 1}, {1, 0, 4}}, {{1, 0, 4}}}},
        {8, 3, 2, {3, 2}, {{5, 0}, {8, 1}, {9, 0}}, {{{0, 0, 2}, {0, 2, 3}, {1, 0, 8}, {2, 0, 9}}, {{2, 4, 2}}}},
        {9, 3, 4, {8}, {{3, 0}}, {{{0, 0, 3}}}},
        {8, 3, 0, {4, 4}, {{17, 1}}, {{{0, 0, 17}}, {{0, 3, 5}}}},
        {7, 1, 1, {1, 1, 1, 1, 1, 1, 1}, {{2, 1}}, {{{0, 1, 1}}}},
    };
    std::mt19937_64 rng(20240607);
    auto felt = [&] { return rng() % P; };
    long calls = 0;
    for (size_t si = 0; si < shapes.size(); si++) {
        const Shape &s = shapes[si];
        const uint32_t nq = 3;
        std::vector<qpgpu_fri_batch> bs(s.batches.size());
        size_t n_openings = 0;
        for (size_t b = 0; b < bs.size(); b++) {
            std::memset(&bs[b], 0, sizeof bs[b]);
            bs[b].num_ranges = (uint32_t)s.batches[b].size();
            for (size_t r = 0; r < s.batches[b].size(); r++) { bs[b].ranges[r] = s.batches[b][r]; n_openings += s.batches[b][r].count; }
        }
        qpgpu_fri_instance inst;
        std::memset(&inst, 0, sizeof inst);
        inst.degree_bits = s.degree_bits; inst.num_oracles = (uint32_t)s.oracles.size(); inst.oracles = s.oracles.data();
        inst.num_batches = (uint32_t)bs.size(); inst.batches = bs.data();
        inst.params.rate_bits = s.rate_bits; inst.params.cap_height = s.cap_height; inst.params.proof_of_work_bits = 0;
        inst.params.num_query_rounds = nq; inst.params.num_reduction_rounds = (uint32_t)s.arity.size();
        for (size_t r = 0; r < s.arity.size(); r++) inst.params.reduction_arity_bits[r] = s.arity[r];
        char err[QPGPU_VERIFY_ERR_CAP] = "";
        qpgpu_fri_verifier *v = nullptr;
        EXPECT(qpgpu_fri_verifier_create(&inst, 0, nullptr, 0, &v, err) == 0 && v, "shape %zu: create: %s", si, err);
        if (!v) continue;
        std::memset(bs.data(), 0xEE, bs.size() * sizeof bs[0]);           // the verifier owns its copy of the instance
        EXPECT(qpgpu_fri_verifier_num_openings(v) == n_openings, "shape %zu: num_openings", si);
        const size_t len = qpgpu_fri_verifier_proof_size(v), cap_words = (size_t)4 << s.cap_height, L = s.degree_bits + s.rate_bits;

        // the layout, restated: where the path-length bytes are and what they should hold
        std::vector<std::pair<size_t, uint8_t>> plen_at;
        {
            size_t off = s.arity.size() * cap_words * 8, lvl = L;
            std::vector<std::pair<size_t, size_t>> ops;                  // (row words, path length)
            for (const qpgpu_fri_oracle_shape &o : s.oracles) ops.push_back({o.num_polys + (o.blinded ? 4 : 0), L - s.cap_height});
            for (uint32_t ab : s.arity) { lvl -= ab; ops.push_back({(size_t)2 << ab, lvl - s.cap_height}); }
            for (uint32_t q = 0; q < nq; q++)
                for (auto &o : ops) { off += 8 * o.first; plen_at.push_back({off, (uint8_t)o.second}); off += 1 + 32 * o.second; }
            size_t fin = s.degree_bits;
            for (uint32_t ab : s.arity) fin -= ab;
            EXPECT(off + ((size_t)16 << fin) + 8 == len, "shape %zu: proof_size %zu, the layout restated gives %zu", si, len, off + ((size_t)16 << fin) + 8);
        }

        // heap blocks of exactly the stated sizes, so that a read past any of them is seen
        std::vector<std::vector<uint64_t>> caps(s.oracles.size(), std::vector<uint64_t>(cap_words));
        std::vector<const uint64_t *> cap_ptrs;
        for (auto &c : caps) { for (uint64_t &x : c) x = felt(); cap_ptrs.push_back(c.data()); }
        std::vector<uint64_t> points(2 * bs.size()), openings(2 * n_openings), betas(2 * s.arity.size() + 1), indices(nq), alpha(2);
        for (auto *vec : {&points, &openings, &betas, &alpha}) for (uint64_t &x : *vec) x = felt();
        indices = {0, ((uint64_t)1 << L) - 1, rng() % ((uint64_t)1 << L)};
        std::vector<uint8_t> proof(len);
        for (size_t i = 0; i + 8 <= len; i += 8) { const uint64_t x = felt(); std::memcpy(&proof[i], &x, 8); }
        // words behind a path-length byte are not aligned: make every 8-byte window at every alignment canonical by keeping
        // the top byte of each window below 0xFF
        for (size_t i = 0; i < len; i++) if (proof[i] == 0xFF) proof[i] = 0x7F;
        for (auto &p : plen_at) proof[p.first] = p.second;

        auto run = [&](const char *what, bool want_text) {
            err[0] = 0;
            const int rc = qpgpu_fri_verify(v, cap_ptrs.data(), points.data(), openings.data(), alpha.data(), s.arity.empty() ? nullptr : betas.data(), 0,
                                            indices.data(), proof.data(), proof.size(), err);
            calls++;
            EXPECT(rc == QPGPU_EVERIFY && (err[0] != 0) == want_text, "shape %zu, %s: rc %d, '%s'", si, what, rc, err);
        };
        run("random proof", true);                                        // some path does not lead to its cap
        for (auto &p : plen_at) {
            for (uint8_t wrong : {(uint8_t)(p.second ^ 1), (uint8_t)61, (uint8_t)255}) {
                proof[p.first] = wrong;
                run("path length byte", true);
            }
            proof[p.first] = p.second;
        }
        // the caller's own garbage is refused, not judged
        indices[1] = (uint64_t)1 << L;
        err[0] = 0;
        EXPECT(qpgpu_fri_verify(v, cap_ptrs.data(), points.data(), openings.data(), alpha.data(), betas.data(), 0, indices.data(), proof.data(), proof.size(), err) == QPGPU_EINVAL,
               "shape %zu: index out of range: '%s'", si, err);
        indices[1] = 0;
        // the challenges of any bytes: a transcript is made, the state advances, nothing else is touched
        qpgpu_challenger c;
        std::memset(&c, 0, sizeof c);                                     // Challenger::new(): an empty sponge, empty buffers
        uint64_t powr = 0;
        EXPECT(qpgpu_fri_verifier_challenges(v, &c, proof.data(), proof.size(), alpha.data(), betas.data(), &powr, indices.data(), err) == 0, "shape %zu: challenges: %s", si, err);
        for (uint64_t x : indices) EXPECT(x < ((uint64_t)1 << L), "shape %zu: index %llu", si, (unsigned long long)x);
        run("drawn challenges", true);
        qpgpu_fri_verifier_free(v);
    }
    std::printf("fri_verify_check: %zu instances, %ld verifications, %d failures\n", shapes.size(), calls, failures);
    return failures ? 1 : 0;
}
