// Host-only test of the launch order of the descent optimisers (uav_motion_planning_amd/csrc/uavqp_descent.h): which solve writes which
// status buffer, when `propose` drops to 0 and which trial index a step sees are rules a GPU run shows only as wrong numbers, so the
// sequence is pinned here with recording hooks, without the HIP runtime.  Compiled and run by tests/test_descent_sequence.py.
#include <cstdio>
#include <vector>

#include "uavqp_descent.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

enum Kind { SOLVE, GRADIENT, STEP };
struct Call {
    Kind kind;
    DescentAt at;    // SOLVE, GRADIENT
    int it;          // the trial index; -1 at the start, at the end and in the INIT step
    bool caller;     // SOLVE, GRADIENT: the caller's status buffer
    bool init;       // STEP
    bool propose;    // STEP
};
static bool same(const Call& a, const Call& b) {
    return a.kind == b.kind && a.at == b.at && a.it == b.it && a.caller == b.caller && a.init == b.init && a.propose == b.propose;
}

// the sequence with recording hooks; call number fail_at (from 0) returns `error`
static int record(int max_iters, int fail_at, int error, std::vector<Call>& log) {
    log.clear();
    auto result = [&] { return (int)log.size() - 1 == fail_at ? error : 0; };
    return descent_sequence(
        max_iters,
        [&](const DescentPoint& p) {
            log.push_back(Call{SOLVE, p.at, p.it, p.caller_status, false, false});
            return result();
        },
        [&](const DescentPoint& p) {
            log.push_back(Call{GRADIENT, p.at, p.it, p.caller_status, false, false});
            return result();
        },
        [&](bool init, int it, bool propose) {
            log.push_back(Call{STEP, DescentAt::START, it, false, init, propose});
            return result();
        });
}

// what the contract says, written out independently of the header
static std::vector<Call> expected(int max_iters) {
    std::vector<Call> e;
    const bool none = max_iters == 0;   // no trial: the start solve is what is handed back
    e.push_back(Call{SOLVE, DescentAt::START, -1, none, false, false});
    e.push_back(Call{GRADIENT, DescentAt::START, -1, none, false, false});
    e.push_back(Call{STEP, DescentAt::START, -1, false, true, max_iters > 0});
    for (int it = 0; it < max_iters; ++it) {
        e.push_back(Call{SOLVE, DescentAt::TRIAL, it, false, false, false});
        e.push_back(Call{GRADIENT, DescentAt::TRIAL, it, false, false, false});
        e.push_back(Call{STEP, DescentAt::START, it, false, false, it != max_iters - 1});
    }
    if (max_iters > 0) e.push_back(Call{SOLVE, DescentAt::FINAL, -1, true, false, false});
    return e;
}

int main() {
    std::vector<Call> log;
    const int iters[] = {0, 1, 2, 5};
    for (int max_iters : iters) {
        CHECK(record(max_iters, -1, 0, log) == 0);
        const std::vector<Call> e = expected(max_iters);
        // the exact list of calls, with the status buffer of every solve / gradient and the propose of every step
        CHECK(log.size() == e.size() && log.size() == (size_t)(3 + 3 * max_iters + (max_iters > 0 ? 1 : 0)));
        for (size_t i = 0; i < log.size() && i < e.size(); ++i) CHECK(same(log[i], e[i]));
        // propose: [max_iters > 0], then 1 for every trial but the last, then 0
        std::vector<bool> propose;
        std::vector<int> trials;
        int finals = 0;
        for (const Call& c : log) {
            if (c.kind == STEP) propose.push_back(c.propose);
            if (c.kind == SOLVE && c.at == DescentAt::TRIAL) trials.push_back(c.it);
            if (c.at == DescentAt::FINAL) {
                ++finals;
                CHECK(c.kind == SOLVE && c.caller);   // the final solve writes the caller's buffer and has no gradient
            }
            if (c.kind != STEP && c.at != DescentAt::FINAL) CHECK(c.caller == (max_iters == 0));   // loop buffer while there are trials
        }
        CHECK(propose.size() == (size_t)max_iters + 1 && propose.front() == (max_iters > 0) && propose.back() == false);
        for (size_t i = 0; i + 1 < propose.size(); ++i) CHECK(propose[i] == true);
        // the trial indices 0 .. max_iters - 1, each once and in order: the callers derive `it & 1` from them
        CHECK(trials.size() == (size_t)max_iters);
        for (size_t i = 0; i < trials.size(); ++i) CHECK(trials[i] == (int)i);
        CHECK(finals == (max_iters > 0 ? 1 : 0));
        CHECK(log.back().kind == (max_iters > 0 ? SOLVE : STEP));
    }

    // an error of any of the 10 calls of max_iters = 2 is returned, and nothing is called behind it
    const std::vector<Call> e2 = expected(2);
    CHECK(e2.size() == 10);
    for (int fail_at = 0; fail_at < 10; ++fail_at) {
        const int error = -(fail_at + 1);
        CHECK(record(2, fail_at, error, log) == error);
        CHECK(log.size() == (size_t)fail_at + 1);
        for (size_t i = 0; i < log.size() && i < e2.size(); ++i) CHECK(same(log[i], e2[i]));
    }

    if (failures == 0) std::printf("descent_sequence OK\n");
    return failures == 0 ? 0 : 1;
}
