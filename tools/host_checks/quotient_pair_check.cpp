// quotient_pair_check.cpp — the pair form of the two hash gates' quotient terms (csrc/quotient_fold.hpp: pairable, pair_sum, the
// plain-arithmetic statement of quotient_hash_pair_kernel), stand-alone and without a GPU, meant to be built with
// -fsanitize=address,undefined. On the default Poseidon2 layout (PoseidonGate's carried over) the two gates are a pair: the swept
// tables hold the same T_NALPHA (the kernel reads slot 0's for both), and the pair's sum at a point, under arbitrary filters,
// equals folded_sum(PoseidonGate) * fA + folded_sum(Poseidon2 gate) * fB, in either gate order, on random rows that satisfy
// neither gate and on rows made to satisfy one of them (the other gate's sum is then what is left). The three other Poseidon2
// layouts (no swap, round 0 on wires, both), a moved block and two gates of one kind are no pair. Two challenges, t0 != 0.
// Agreement is exact. Built and run by tests/test_quotient_pair_host.py.
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

constexpr size_t NW = 135, T0 = 7, NQ = 123, NTERMS = T0 + NQ;

// a row that satisfies gate g: the S-box-input wires and outputs take the values its constraints ask for, in constraint order
static void satisfy(const GateInfo &g, const P2GateLayout &lay, const qfold::Schedule &s, std::vector<u64> &row) {
    row[s.w_swap] &= 1;
    for (int i = 0; i < 4; i++) row[s.w_delta + i] = gl::canon(gl::mul(row[s.w_swap], gl::sub(row[s.w_input + 4 + i], row[s.w_input + i])));
    for (uint32_t t = 0; t < s.nw + 12; t++) {
        std::vector<e2> w(NW), out(NQ);
        for (size_t i = 0; i < NW; i++) w[i] = gl::e2_from(row[i]);
        const e2 pih[4] = {};
        EXPECT(vmath::gate_constraints_to(g, lay, (const e2 *)nullptr, w.data(), pih, out.data()) == NQ);
        const uint32_t wire = t < s.nw ? qfold::target_wire(s, t) : s.w_output + (t - s.nw);
        row[wire] = gl::canon(gl::add(row[wire], out[s.q0 + t].a));
    }
}

static void check_pair() {
    const P2GateLayout lay;
    GateInfo g1{}; g1.type = GATE_POSEIDON; g1.num_constraints = NQ;
    GateInfo g2{}; g2.type = GATE_POSEIDON2; g2.num_constraints = lay.num_constraints();
    const qfold::Schedule s1 = qfold::poseidon_schedule(), s2 = qfold::poseidon2_schedule(lay);
    const qfold::Consts K = {poseidon::host_round_constants(), &poseidon2::qp_params()};
    EXPECT(qfold::pairable(s1, s2) && qfold::pairable(s2, s1));
    EXPECT(!qfold::pairable(s1, s1) && !qfold::pairable(s2, s2));
    EXPECT(s1.nw == 106 && s2.nw == 106 && s1.q0 + s1.nw + 12 == NQ);
    int rows = 0, tables = 0;
    for (int trial = 0; trial < 36; trial++) {
        std::vector<u64> row(NW);
        for (auto &v : row) v = felt();
        if (trial % 4 == 1) for (auto &v : row) v = gl::P - 1 - (v & 3);          // near p
        if (trial % 4 == 2) for (auto &v : row) v &= 0xFFFFFFFFull;               // 32-bit values
        if (trial % 6 == 3) row[s1.w_swap] = 0;
        if (trial % 6 == 5) row[s1.w_swap] = 1;
        const int sat = trial % 3;               // 0: neither gate satisfied, 1: the PoseidonGate, 2: the Poseidon2 gate
        if (sat == 1) satisfy(g1, lay, s1, row);
        if (sat == 2) satisfy(g2, lay, s2, row);
        for (int c = 0; c < 2; c++) {
            const u64 alpha = felt();
            std::vector<u64> apow(NTERMS);
            u64 a = 1;
            for (auto &v : apow) { v = gl::canon(a); a = gl::mul(a, alpha); }
            qfold::Scratch scratch;
            std::vector<u64> t1(qfold::WORDS, 0xDEADBEEFull), t2(qfold::WORDS, 0xFEEDFACEull);
            qfold::sweep(s1, K, apow.data() + T0, scratch, t1.data(), 0, 1, [] {});
            qfold::sweep(s2, K, apow.data() + T0, scratch, t2.data(), 0, 1, [] {});
            bool same = true;
            for (uint32_t k = 0; k < s1.nw + 12; k++) same = same && t1[qfold::T_NALPHA + k] == t2[qfold::T_NALPHA + k];
            EXPECT(same);
            tables++;
            const u64 f1 = trial % 5 == 4 ? 0 : felt(), f2 = trial % 7 == 6 ? 0 : felt();
            const u64 sum1 = qfold::folded_sum(s1, K, row.data(), apow.data() + T0, t1.data());
            const u64 sum2 = qfold::folded_sum(s2, K, row.data(), apow.data() + T0, t2.data());
            EXPECT((sum1 == 0) == (sat == 1) && (sum2 == 0) == (sat == 2));
            const u64 want = gl::canon(gl::add(gl::mul(sum1, f1), gl::mul(sum2, f2)));
            // the PoseidonGate in table slot 0, then the Poseidon2 gate in slot 0: T_NALPHA comes from the first table given
            EXPECT(qfold::pair_sum(s1, s2, K, row.data(), apow.data() + T0, t1.data(), t2.data(), f1, f2) == want);
            EXPECT(qfold::pair_sum(s2, s1, K, row.data(), apow.data() + T0, t2.data(), t1.data(), f2, f1) == want);
            rows++;
        }
    }
    std::printf("pair on the default layout: %d (row, challenge) sums compared, %d table pairs with equal T_NALPHA\n", rows, tables);
}

static void check_not_pairable() {
    const qfold::Schedule s1 = qfold::poseidon_schedule();
    int layouts = 0;
    for (int has_swap = 0; has_swap < 2; has_swap++)
        for (int frw = 0; frw < 2; frw++) {
            if (has_swap && !frw) continue;      // that one is the default's shape
            P2GateLayout lay;                    // the default's blocks, without the swap and / or with round 0 on wires behind them
            lay.first_round_wires = (uint32_t)frw;
            uint32_t end = 29;
            lay.w_full0 = end; end += 12 * lay.full0_rounds();
            lay.w_partial = end; end += 22;
            lay.w_full1 = end; end += 48;
            if (has_swap) { lay.w_swap = 24; lay.w_delta = 25; }
            else { lay.w_swap = P2GateLayout::NO_SWAP; lay.w_delta = 0; }
            lay.end_wire = end;
            const qfold::Schedule s2 = qfold::poseidon2_schedule(lay);
            EXPECT(!qfold::pairable(s1, s2) && !qfold::pairable(s2, s1));
            layouts++;
        }
    {   // the default's shape with one block elsewhere: same counts, other wires
        P2GateLayout lay;
        lay.w_partial = 135; lay.end_wire = 157;
        const qfold::Schedule s2 = qfold::poseidon2_schedule(lay);
        EXPECT(s2.head == qfold::HEAD_SBOX && s2.q0 == s1.q0 && s2.nw == s1.nw);
        EXPECT(!qfold::pairable(s1, s2) && !qfold::pairable(s2, s1));
        lay = P2GateLayout();
        lay.w_output = 140; lay.end_wire = 152;
        EXPECT(!qfold::pairable(s1, qfold::poseidon2_schedule(lay)));
    }
    std::printf("not a pair: %d other Poseidon2 layouts, moved blocks, two gates of one kind\n", layouts);
}

int main() {
    check_pair();
    check_not_pairable();
    std::printf("quotient pair: failures %d\n", bad);
    return bad != 0;
}
