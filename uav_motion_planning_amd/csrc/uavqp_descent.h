// uavqp_descent.h -- the ONE launch order of the descent optimisers of include/uavqp.h (uavqp_time_optimize, _time_optimize_limits,
// _waypoint_optimize, _spacetime_optimize, _spacetime_lbfgs, _attitude_optimize, _swarm_optimize).  Plain C++, no
// HIP runtime: tests/cpp/test_descent_sequence.cpp pins the order on the CPU with recording hooks.
//     solve(start) -> gradient(start) -> step<INIT>
//       -> max_iters x { solve(trial it) -> gradient(trial it) -> step<ITER> } -> solve(final), if max_iters > 0
// What is enqueued at each point is the entry's business (its three hooks), as are the prologue before the sequence and the diagnostics
// behind it.  NO data-dependent control flow: the number of calls is fixed by max_iters.
#pragma once

enum class DescentAt { START, TRIAL, FINAL };

// Where a solve (and the gradient of its result) runs.  START and FINAL: the caller's arrays.  TRIAL: the trial arrays; where an entry
// keeps two trial arrays it reads `it & 1` and writes `(it + 1) & 1`.
struct DescentPoint {
    DescentAt at;
    int it;               // TRIAL: 0 .. max_iters - 1, each once and in order; otherwise -1
    bool caller_status;   // the status goes to the caller's array: the final solve, and the start where there is no trial at all.
                          // false: the workspace buffer of the loop, so that a rejected trial never shows in what is handed back
};

// solve(point), gradient(point) -- the penalty launches and the one backward pass, nothing where f has no penalty -- and
// step(init, it, propose), with propose = false on the last step: no further trial is written.  Each returns UAVQP_OK (0) or the error
// that ends the sequence at that call.  The hooks are template parameters (lambdas inline): nothing is allocated, nothing is virtual.
template <class Solve, class Gradient, class Step>
static inline int descent_sequence(int max_iters, Solve&& solve, Gradient&& gradient, Step&& step) {
    const DescentPoint start{DescentAt::START, -1, max_iters == 0};
    int rc = solve(start);
    if (rc == 0) rc = gradient(start);
    if (rc == 0) rc = step(true, -1, max_iters > 0);
    for (int it = 0; rc == 0 && it < max_iters; ++it) {
        const DescentPoint trial{DescentAt::TRIAL, it, false};
        rc = solve(trial);
        if (rc == 0) rc = gradient(trial);
        if (rc == 0) rc = step(false, it, it + 1 < max_iters);
    }
    // the coefficients on return are the solve AT the accepted point (the last trial of a trajectory may have been rejected, and a
    // trajectory that never took part must carry what a plain solve leaves there)
    if (rc == 0 && max_iters > 0) rc = solve(DescentPoint{DescentAt::FINAL, -1, true});
    return rc;
}
