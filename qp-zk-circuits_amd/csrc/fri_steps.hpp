// fri_steps.hpp — the order in which the steps of one FRI opening proof may be taken (fri_prover.hpp: fri_round_commit,
// fri_round_fold, fri_final_poly, fri_gather; include/qpgpu.h: qpgpu_fri_session). Host only, no device types: checked as a
// stand-alone program by tools/host_checks/fri_steps_check.cpp.
//
// A schedule of R reduction rounds is R times (commit, fold); the final polynomial and the query openings exist once the last
// fold has been taken (at once when R = 0) and may then be asked for any number of times, in any order. refuse() says why a
// call is out of order, naming what is expected instead; a refused call changes nothing.
#pragma once
#include <string>

struct FriSteps {
    enum Call { COMMIT, FOLD, FINAL_POLY, OPEN };
    unsigned rounds = 0;        // reduction rounds of the schedule
    unsigned round = 0;         // folds taken: the round the next commit (or the pending fold) belongs to
    bool committed = false;     // round `round` has its cap and waits for its beta

    explicit FriSteps(unsigned n_rounds = 0) : rounds(n_rounds) {}
    bool folded() const { return round == rounds && !committed; }
    bool allowed(Call c) const {
        switch (c) {
            case COMMIT: return !committed && round < rounds;
            case FOLD: return committed;
            default: return folded();
        }
    }
    // empty when the call is in order
    std::string refuse(Call c) const {
        if (allowed(c)) return std::string();
        const std::string at = "round " + std::to_string(round) + " of " + std::to_string(rounds);
        switch (c) {
            case COMMIT:
                if (committed) return "fri_round_commit: " + at + " is committed and waits for its fold (qpgpu_fri_round_fold expected)";
                return "fri_round_commit: all " + std::to_string(rounds) + " rounds are folded (qpgpu_fri_final_poly or qpgpu_fri_open expected)";
            case FOLD:
                if (round < rounds) return "fri_round_fold: no committed round is waiting (qpgpu_fri_round_commit of " + at + " expected)";
                return "fri_round_fold: no committed round is waiting: all " + std::to_string(rounds) + " rounds are folded (qpgpu_fri_final_poly or qpgpu_fri_open expected)";
            default: {
                const std::string who = c == FINAL_POLY ? "fri_final_poly" : "fri_open";
                return who + ": before the last fold (" + (committed ? "qpgpu_fri_round_fold" : "qpgpu_fri_round_commit") + " of " + at + " expected)";
            }
        }
    }
    // the call has been made: advance. Only for a call that allowed() admits.
    void done(Call c) {
        if (c == COMMIT) committed = true;
        else if (c == FOLD) { committed = false; round++; }
    }
};
