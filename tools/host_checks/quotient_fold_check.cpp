// quotient_fold_check.cpp — the folded form of the hash gates' quotient terms (csrc/quotient_fold.hpp: the backward walk that
// turns alpha powers into per-S-box weights, and the folded sum the per-point kernels compute) and the forward walk the
// round-by-round kernel is instantiated over (qfold::walk), both against the plain
// sum_q alpha^(t0+q) c_q over the constraints of the host gate evaluation (verify_math.hpp, base-field values), stand-alone and
// without a GPU, meant to be built with -fsanitize=address,undefined. Random wire rows that do NOT satisfy the gate (every
// constraint non-zero) and rows made to satisfy it; PoseidonGate with swap 0 and 1, the Poseidon2 gate in its four
// has_swap x first_round_wires layouts (one with the wire blocks moved around); two challenges, t0 != 0. Agreement is exact.
// Built and run by tests/test_quotient_fold_host.py.
#include <cstdio>
#include <cstring>
#include <vector>
#include "quotient_fold.hpp"
#include "verify_math.hpp"

using gl::e2;
using gl::u64;
static int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)

static u64 seed = 0x9E3779B97F4A7C15ull;
static u64 rnd() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; }
static u64 felt() { return gl::canon(rnd()); }

constexpr size_t NW = 160, T0 = 7, MAXQ = 135, NTERMS = T0 + MAXQ;   // 135: the Poseidon2 gate with swap and round 0 recorded

// a row that satisfies the gate: the S-box-input wires and outputs take the values the constraints ask for, in constraint order
static void satisfy(const GateInfo &g, const P2GateLayout &lay, const qfold::Schedule &s, std::vector<u64> &row) {
    if (s.w_swap != qfold::NO_SWAP) {
        row[s.w_swap] &= 1;
        for (int i = 0; i < 4; i++)
            row[s.w_delta + i] = gl::canon(gl::mul(row[s.w_swap], gl::sub(row[s.w_input + 4 + i], row[s.w_input + i])));
    }
    for (uint32_t t = 0; t < s.nw + 12; t++) {   // constraint q0 + t reads only earlier targets: fix them one by one
        std::vector<e2> w(NW), out(MAXQ);
        for (size_t i = 0; i < NW; i++) w[i] = gl::e2_from(row[i]);
        const e2 pih[4] = {};
        const size_t k = vmath::gate_constraints_to(g, lay, (const e2 *)nullptr, w.data(), pih, out.data());
        EXPECT(k == s.q0 + s.nw + 12);
        const uint32_t wire = t < s.nw ? qfold::target_wire(s, t) : s.w_output + (t - s.nw);
        row[wire] = gl::canon(gl::add(row[wire], out[s.q0 + t].a));   // constraint = state - wire
    }
}

static void check_gate(const char *name, const GateInfo &g, const P2GateLayout &lay, int swap_mode) {
    const qfold::Schedule s = g.type == GATE_POSEIDON ? qfold::poseidon_schedule() : qfold::poseidon2_schedule(lay);
    const qfold::Consts K = {poseidon::host_round_constants(), &poseidon2::qp_params()};
    const size_t nq = s.q0 + s.nw + 12;
    EXPECT(nq == (g.type == GATE_POSEIDON ? 123 : lay.num_constraints()));
    int rows = 0;
    for (int trial = 0; trial < 24; trial++) {
        std::vector<u64> row(NW);
        for (auto &v : row) v = felt();
        if (trial % 4 == 1) for (auto &v : row) v = gl::P - 1 - (v & 3);          // near p
        if (trial % 4 == 2) for (auto &v : row) v &= 0xFFFFFFFFull;               // 32-bit values
        if (s.w_swap != qfold::NO_SWAP && swap_mode >= 0) row[s.w_swap] = (u64)swap_mode;
        const bool sat = trial % 3 == 2;
        if (sat) satisfy(g, lay, s, row);
        std::vector<e2> w(NW), out(MAXQ);
        for (size_t i = 0; i < NW; i++) w[i] = gl::e2_from(row[i]);
        const e2 pih[4] = {};
        const size_t k = vmath::gate_constraints_to(g, lay, (const e2 *)nullptr, w.data(), pih, out.data());
        EXPECT(k == nq);
        for (int c = 0; c < 2; c++) {             // two challenges
            const u64 alpha = felt();
            std::vector<u64> apow(NTERMS);
            u64 a = 1;
            for (auto &v : apow) { v = gl::canon(a); a = gl::mul(a, alpha); }
            u64 plain = 0;
            bool all_zero = true;
            for (size_t q = 0; q < nq; q++) {
                EXPECT(gl::canon(out[q].b) == 0);
                all_zero = all_zero && gl::canon(out[q].a) == 0;
                plain = gl::add(plain, gl::mul(apow[T0 + q], out[q].a));
            }
            EXPECT(all_zero == sat);
            qfold::Scratch scratch;
            std::vector<u64> table(qfold::WORDS, 0xDEADBEEFull);
            qfold::sweep(s, K, apow.data() + T0, scratch, table.data(), 0, 1, [] {});
            const u64 folded = qfold::folded_sum(s, K, row.data(), apow.data() + T0, table.data());
            EXPECT(folded == gl::canon(plain));
            if (sat) EXPECT(folded == 0);
            // the forward walk (the round-by-round kernel's form): the same constraints in the same order, weighted as it emits them
            u64 walked = 0;
            size_t emitted = 0;
            qfold::walk(s, K, [&](uint32_t wire) { return row[wire]; }, [&](uint32_t q, u64 cst) {
                EXPECT(q < nq);
                walked = gl::add(walked, gl::mul(apow[T0 + q], cst));
                emitted++;
            });
            EXPECT(emitted == nq);
            EXPECT(gl::canon(walked) == gl::canon(plain));
            if (sat) EXPECT(gl::canon(walked) == 0);
            rows++;
        }
    }
    std::printf("%s: %d (row, challenge) pairs compared\n", name, rows);
}

int main() {
    GateInfo pg{}; pg.type = GATE_POSEIDON; pg.num_constraints = 123;
    check_gate("PoseidonGate swap 0", pg, P2GateLayout(), 0);
    check_gate("PoseidonGate swap 1", pg, P2GateLayout(), 1);
    check_gate("PoseidonGate swap any (boolean constraint non-zero)", pg, P2GateLayout(), -1);
    for (int has_swap = 0; has_swap < 2; has_swap++)
        for (int frw = 0; frw < 2; frw++) {
            P2GateLayout lay;                      // the blocks moved around: inputs, outputs, partial, second half, first half, swap, deltas
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
            check_gate(name, g, lay, -1);
            if (has_swap) { check_gate(name, g, lay, 0); check_gate(name, g, lay, 1); }
        }
    {   // the default layout as well (the one the leaf circuit uses)
        GateInfo g{}; g.type = GATE_POSEIDON2; g.num_constraints = 123;
        check_gate("Poseidon2 gate default layout", g, P2GateLayout(), -1);
    }
    std::printf("quotient fold: failures %d\n", bad);
    return bad != 0;
}
