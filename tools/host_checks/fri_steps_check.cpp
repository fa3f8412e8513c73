// fri_steps_check.cpp — the call-order state machine of a FRI session (qp-zk-circuits_amd/csrc/fri_steps.hpp) driven through every
// state of schedules of 0, 1, 3 and 16 rounds. Host only; meant to be built with -fsanitize=address,undefined:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I qp-zk-circuits_amd/csrc tools/host_checks/fri_steps_check.cpp
//
// The rule restated without the header's fields: a session is at position k of 2R + 1. At an even k < 2R only the commit of round
// k / 2 is legal, at an odd k only its fold, at k = 2R only the final polynomial and the openings, any number of times in any order.
// At every position every call is tried: a legal one advances (or stays, at the end), an illegal one is refused with a message
// that begins with its own name and names the call that is expected, and changes nothing.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "fri_steps.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const char *entry_name(FriSteps::Call c) {
    switch (c) {
        case FriSteps::COMMIT: return "fri_round_commit";
        case FriSteps::FOLD: return "fri_round_fold";
        case FriSteps::FINAL_POLY: return "fri_final_poly";
        default: return "fri_open";
    }
}
static bool legal_at(unsigned k, unsigned rounds, FriSteps::Call c) {
    if (k == 2 * rounds) return c == FriSteps::FINAL_POLY || c == FriSteps::OPEN;
    return k % 2 == 0 ? c == FriSteps::COMMIT : c == FriSteps::FOLD;
}
static bool same(const FriSteps &a, const FriSteps &b) { return a.rounds == b.rounds && a.round == b.round && a.committed == b.committed; }

static void check_position(const FriSteps &s, unsigned k, unsigned rounds, long &refusals) {
    const FriSteps::Call all[4] = {FriSteps::COMMIT, FriSteps::FOLD, FriSteps::FINAL_POLY, FriSteps::OPEN};
    EXPECT(s.round == k / 2 && s.committed == (k % 2 == 1) && s.folded() == (k == 2 * rounds), "position %u of %u rounds: cursor %u/%d", k, rounds, s.round, (int)s.committed);
    for (FriSteps::Call c : all) {
        FriSteps t = s;
        const std::string why = t.refuse(c);
        EXPECT(same(t, s), "refuse() changed the state at position %u", k);
        EXPECT(t.allowed(c) == legal_at(k, rounds, c), "%s at position %u of %u rounds: allowed = %d", entry_name(c), k, rounds, (int)t.allowed(c));
        EXPECT(why.empty() == legal_at(k, rounds, c), "%s at position %u of %u rounds: message '%s'", entry_name(c), k, rounds, why.c_str());
        if (legal_at(k, rounds, c)) continue;
        refusals++;
        EXPECT(why.rfind(std::string(entry_name(c)) + ": ", 0) == 0, "'%s' does not begin with %s", why.c_str(), entry_name(c));
        const char *next = k == 2 * rounds ? "qpgpu_fri_final_poly or qpgpu_fri_open expected" : (k % 2 == 0 ? "qpgpu_fri_round_commit" : "qpgpu_fri_round_fold");
        EXPECT(why.find(next) != std::string::npos && why.find("expected") != std::string::npos, "'%s' does not name %s", why.c_str(), next);
        if (k < 2 * rounds) {
            const std::string at = "round " + std::to_string(k / 2) + " of " + std::to_string(rounds);
            EXPECT(why.find(at) != std::string::npos, "'%s' does not say '%s'", why.c_str(), at.c_str());
        }
    }
}

int main() {
    const unsigned schedules[4] = {0, 1, 3, 16};
    long refusals = 0, orders = 0;
    for (unsigned rounds : schedules) {
        FriSteps s(rounds);
        for (unsigned k = 0; k < 2 * rounds; k++) {
            check_position(s, k, rounds, refusals);
            const FriSteps::Call c = k % 2 == 0 ? FriSteps::COMMIT : FriSteps::FOLD;
            s.done(c);
        }
        check_position(s, 2 * rounds, rounds, refusals);
        // at the end: every order of up to five final-polynomial / opening calls, refused calls mixed in; the state never moves
        for (unsigned len = 0; len <= 5; len++)
            for (unsigned bits = 0; bits < (1u << len); bits++) {
                FriSteps t = s;
                for (unsigned i = 0; i < len; i++) {
                    const FriSteps::Call c = (bits >> i) & 1 ? FriSteps::OPEN : FriSteps::FINAL_POLY;
                    EXPECT(t.refuse(c).empty(), "%s refused at the end of %u rounds", entry_name(c), rounds);
                    t.done(c);
                    EXPECT(!t.allowed(FriSteps::COMMIT) && !t.allowed(FriSteps::FOLD), "a round call became legal at the end of %u rounds", rounds);
                    EXPECT(same(t, s), "%s moved the state at the end of %u rounds", entry_name(c), rounds);
                }
                orders++;
            }
    }
    // a default-constructed machine is the schedule of zero rounds
    FriSteps z;
    EXPECT(z.folded() && z.allowed(FriSteps::OPEN) && !z.allowed(FriSteps::COMMIT), "default state");
    std::printf("fri steps: %ld refusals and %ld closing orders checked over schedules of 0, 1, 3 and 16 rounds\n", refusals, orders);
    std::printf("fri steps: failures %d\n", failures);
    return failures ? 1 : 0;
}
