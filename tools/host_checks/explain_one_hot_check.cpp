// explain_one_hot_check.cpp — is the folded form of the hash gates (csrc/quotient_fold.hpp) exact under weights that are NOT
// powers of a challenge? qpgpu_circuit_explain_witness (csrc/explain_api.cpp) runs the gate kernels with one-hot weight tables
// (column c = the indicator of one constraint) and reads the sums as the constraints themselves; that is right only if the fold's
// backward walk is linear in the weights and reads nothing but the table it is given. Here, on the host and stand-alone: for
// every constraint q of PoseidonGate and of the Poseidon2 gate (default layout and a moved one, with and without swap wires and
// recorded first round), the table swept from the indicator of q gives, through folded_sum, exactly constraint q of the
// round-by-round form (qfold::walk) and of verify_math.hpp, on random rows that do not satisfy the gate; and a table swept from
// arbitrary weights gives the weighted sum. Meant to be built with -fsanitize=address,undefined; run by
// tests/test_witness_explain_host.py.
#include <cstdio>
#include <vector>
#include "quotient_fold.hpp"
#include "verify_math.hpp"

using gl::e2;
using gl::u64;
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

static u64 seed = 0xD1B54A32D192ED03ull;
static u64 rnd() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; }
static u64 felt() { return gl::canon(rnd()); }

constexpr size_t NW = 160, MAXQ = 135;

static void check_gate(const char *name, const GateInfo &g, const P2GateLayout &lay) {
    const qfold::Schedule s = g.type == GATE_POSEIDON ? qfold::poseidon_schedule() : qfold::poseidon2_schedule(lay);
    const qfold::Consts K = {poseidon::host_round_constants(), &poseidon2::qp_params()};
    const size_t nq = s.q0 + s.nw + 12;
    size_t compared = 0;
    for (int trial = 0; trial < 3; trial++) {
        std::vector<u64> row(NW);
        for (auto &v : row) v = felt();
        if (trial == 1) for (auto &v : row) v = gl::P - 1 - (v & 3);
        if (s.w_swap != qfold::NO_SWAP && trial == 2) row[s.w_swap] &= 1;
        std::vector<e2> w(NW), out(MAXQ);
        for (size_t i = 0; i < NW; i++) w[i] = gl::e2_from(row[i]);
        const e2 pih[4] = {};
        EXPECT(vmath::gate_constraints_to(g, lay, (const e2 *)nullptr, w.data(), pih, out.data()) == nq);
        std::vector<u64> walked(nq, 0);
        qfold::walk(s, K, [&](uint32_t wire) { return row[wire]; }, [&](uint32_t q, u64 cst) { if (q < nq) walked[q] = gl::canon(cst); });
        for (size_t q = 0; q < nq; q++) {
            std::vector<u64> ap(MAXQ, 0);
            ap[q] = 1;
            qfold::Scratch scratch;
            std::vector<u64> table(qfold::WORDS, 0xDEADBEEFull);
            qfold::sweep(s, K, ap.data(), scratch, table.data(), 0, 1, [] {});
            const u64 folded = gl::canon(qfold::folded_sum(s, K, row.data(), ap.data(), table.data()));
            EXPECT(folded == walked[q]);
            EXPECT(folded == gl::canon(out[q].a) && gl::canon(out[q].b) == 0);
            compared++;
        }
        {   // arbitrary weights: the weighted sum
            std::vector<u64> ap(MAXQ);
            for (auto &v : ap) v = felt();
            u64 plain = 0;
            for (size_t q = 0; q < nq; q++) plain = gl::add(plain, gl::mul(ap[q], walked[q]));
            qfold::Scratch scratch;
            std::vector<u64> table(qfold::WORDS, 0);
            qfold::sweep(s, K, ap.data(), scratch, table.data(), 0, 1, [] {});
            EXPECT(gl::canon(qfold::folded_sum(s, K, row.data(), ap.data(), table.data())) == gl::canon(plain));
        }
    }
    std::printf("%s: %zu one-hot folds compared\n", name, compared);
}

int main() {
    GateInfo pg{}; pg.type = GATE_POSEIDON; pg.num_constraints = 123;
    check_gate("PoseidonGate", pg, P2GateLayout());
    {
        GateInfo g{}; g.type = GATE_POSEIDON2; g.num_constraints = 123;
        check_gate("Poseidon2 gate default layout", g, P2GateLayout());
    }
    for (int has_swap = 0; has_swap < 2; has_swap++)
        for (int frw = 0; frw < 2; frw++) {
            P2GateLayout lay;
            lay.w_input = 3; lay.w_output = 20; lay.w_partial = 33; lay.w_full1 = 56; lay.w_full0 = 105;
            lay.first_round_wires = (uint32_t)frw;
            uint32_t end = lay.w_full0 + 12 * lay.full0_rounds();
            if (has_swap) { lay.w_swap = end; lay.w_delta = end + 1; end += 5; }
            else { lay.w_swap = P2GateLayout::NO_SWAP; lay.w_delta = 0; }
            lay.end_wire = end;
            EXPECT(end <= NW);
            GateInfo g{}; g.type = GATE_POSEIDON2; g.num_constraints = lay.num_constraints();
            char name[96];
            std::snprintf(name, sizeof name, "Poseidon2 gate has_swap %d first_round_wires %d", has_swap, frw);
            check_gate(name, g, lay);
        }
    std::printf("explain one-hot fold: failures %d\n", bad);
    return bad != 0;
}
