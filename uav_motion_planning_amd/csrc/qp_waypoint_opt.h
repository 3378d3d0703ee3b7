// qp_waypoint_opt.h -- exact gradient of the control cost with respect to the waypoints, and the per-trajectory step of the waypoint
// optimiser (uavqp_cost_waypoint_gradient_device / uavqp_waypoint_optimize_device, include/uavqp.h).
//
// Gradient.  J = sum over axes and segments of integral_0^{T_i} (p_i^(r))^2 dt at the minimiser of the equality-constrained QP.  Vary the
// knot states (position and the r-1 derivatives of every knot); each segment stays the degree-(2r-1) interpolant of its two knot states, so
// p^(2r) = 0 and r integrations by parts leave only boundary terms, per axis and segment:
//     delta J_seg = 2 sum_{m=0}^{r-1} (-1)^m [ p^(r+m) delta p^(r-1-m) ]_0^{T_i}
// The terms with a knot DERIVATIVE (m < r-1) vanish when summed over the two segments that meet at a knot: at an interior knot the derivative
// is free and J is stationary in it (the envelope argument of qp_time_opt.h), at an end knot it is a boundary condition and is not varied.
// What survives is the position term m = r-1, and p^(2r-1) = (2r-1)! c_{2r-1} is constant along a segment:
//     dJ/dp_k = 2 (-1)^(r-1) (2r-1)! (c_{k-1,2r-1} - c_{k,2r-1})        per axis; at k = 0 only the second term, at k = M only the first.
//   r = 3: 240 (c_{k-1,5} - c_{k,5})          r = 4: -10080 (c_{k-1,7} - c_{k,7})
// The end rows are the true derivatives with respect to the end positions at fixed boundary derivatives: the central differences of the
// optimal cost in tests/test_waypoint_opt_contract.py and the backward pass with g = 2 P c (tests/test_gpu_waypoint_opt.py) confirm all M + 1 rows.
// This holds for the equality-constrained solve; NOT for corridor boxes that are active or for general rows.
//
// Lanes.  The lane groups of qp_poly.h: eight lanes per trajectory, sub-lane j owns knots j, j + 8, ... (and, for the cost, segments
// j, j + 8, ...); sums and maxima by the butterfly of topt_group_sum / topt_group_max -- a fixed order of additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"
#include "qp_time_opt.h"

namespace uavqp {

// dJ/dp_k of knot k of a trajectory with M >= 1 segments, three axes (c0: the trajectory's coefficients, axis stride in doubles)
template <int R>
__device__ inline void wpopt_knot_grad(const double* __restrict__ c0, size_t axis_stride, int M, int k, double* g) {
    constexpr int NC = 2 * R;
    constexpr double F = ((R & 1) ? 2.0 : -2.0) * topt_falling(NC - 1, NC - 1);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double* ca = c0 + (size_t)ax * axis_stride;
        const double before = k > 0 ? ca[(size_t)(k - 1) * NC + NC - 1] : 0.0;
        const double behind = k < M ? ca[(size_t)k * NC + NC - 1] : 0.0;
        g[ax] = F * (before - behind);
    }
}

// ---------------------------------------------------------------------------------------------------
// grad[s0_b + b + k][axis] = dJ_b / dp_k, all M_b + 1 knots; zeros for a trajectory that is not solved or has no segment
// ---------------------------------------------------------------------------------------------------
struct WaypointGradArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* coeff;
    const int32_t* status;   // or null: every trajectory counts as solved
    double* grad;
};

template <int R>
__global__ __launch_bounds__(64) void cost_waypoint_grad_kernel(WaypointGradArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        if (!live) return;   // (no shuffle in this kernel)
        const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
        if (M < 0) return;
        const bool solved = M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        const double* __restrict__ c0 = a.coeff + (size_t)3 * NC * s0;
        double* __restrict__ out = a.grad + 3 * ((size_t)s0 + b);
        for (int k = sub; k <= M; k += LPT) {
            double g[3] = {0.0, 0.0, 0.0};
            if (solved) wpopt_knot_grad<R>(c0, (size_t)NC * M, M, k, g);
            out[3 * (size_t)k] = g[0]; out[3 * (size_t)k + 1] = g[1]; out[3 * (size_t)k + 2] = g[2];
        }
    });
}

// ---------------------------------------------------------------------------------------------------
// Waypoint optimiser: minimise f(p) = smooth_weight J(p) + Phi(c*(p), T) over the interior waypoints inside the box
// |p - anchor| <= max_move per component, per trajectory, by projected gradient descent with Armijo backtracking along the projection
// arc.  Direction d_k = (df/dp_k) / s_k with s_k = T_{k-1}^-(2r-1) + T_k^-(2r-1) (J scales like T^-(2r-1): one step length then serves
// knots between short and between long segments; s_k > 0, so -d is a descent direction), a component zero where the box blocks it.
// The host enqueues solve, penalty, backward, step<INIT>, then max_iters x { solve at the trial waypoints, penalty, backward, step<ITER> };
// every decision is taken here, per trajectory.
//   INIT   status SOLVED and f finite -> the trajectory takes part: f_best = f, gradient stored, alpha = initial_step / max |d| (the first
//          trial moves the most sensitive component by initial_step metres; no direction -- no interior knot, or a zero gradient -- gives
//          alpha = 0: the trajectory proposes its own point and accepts nothing), first trial written
//          otherwise it does not: its trial waypoints are its own, so every later solve flags it the same way
//   ITER   the trial was solved into `coeff`, its penalty is phi[b], the penalty's gradient through the minimiser is `through`:
//          accepted iff alpha > 0, its status is SOLVED and f_trial <= f_best - armijo * sum (df/dp) . (p - p_trial)
//          -> waypoints, f_best, gradient replaced, alpha *= grow; else alpha *= shrink.  Then the next trial from the best point.
// The end knots are never moved: a trial carries the caller's bytes there.
// ---------------------------------------------------------------------------------------------------
struct WaypointOptArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    double* waypoints;        // the best (accepted) waypoints: the caller's array
    double* trial;            // [knots][3] trial waypoints (workspace)
    const double* anchor;     // [knots][3] the start: centre of the box
    double* gbest;            // [knots][3] df/dp at the best waypoints (workspace)
    const double* times;
    const double* coeff;      // the solve at `waypoints` (INIT) / at `trial` (ITER)
    const int32_t* status;    // its status
    const double* phi;        // [n_traj] penalty of that solve
    const double* through;    // [knots][3] dPhi/dp through the minimiser (backward pass of the penalty's coefficient gradient)
    double* fbest;            // [n_traj] workspace
    double* alpha;            // [n_traj] workspace
    double* need;             // [n_traj] workspace: the decrease the pending trial has to reach
    int32_t* active;          // [n_traj] workspace
    double* objective;        // [n_traj][2]: f at the start, f at the best point
    int32_t* accepted;        // [n_traj] or null
    double ws, max_move, initial_step, armijo, shrink, grow;
    int propose;              // 0: last step, no further trial
};

template <int R>
__device__ inline double wpopt_inv_pow(double T) {   // T^-(2r-1)
    double p = T;
#pragma unroll
    for (int j = 1; j < 2 * R - 1; ++j) p *= T;
    return 1.0 / p;
}

// the scaled direction of one component, zero where the box blocks the move p - alpha d
__device__ inline double wpopt_dir(double g, double s, double p, double lo, double hi) {
    const double d = g / s;
    return ((p <= lo && d > 0.0) || (p >= hi && d < 0.0)) ? 0.0 : d;
}

template <int R, bool INIT>
__global__ __launch_bounds__(64) void waypoint_opt_step_kernel(WaypointOptArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
        const size_t axs = (size_t)NC * M;
        const size_t k0 = 3 * ((size_t)s0 + b);   // the trajectory's first knot in the waypoint arrays
        const double* __restrict__ c0 = a.coeff + (size_t)3 * NC * s0;
        const bool solved = live && M > 0 && a.status[b] == UAVQP_SOLVED;
        bool act = INIT ? solved : (live && a.active[b] != 0);

        // f at the point the last solve ran at
        double J = 0.0;
        if (solved && act)
            for (int i = sub; i < M; i += LPT) J += topt_segment_cost<R>(c0 + (size_t)i * NC, axs, a.times[s0 + i]);
        J = topt_group_sum(J);
        const double f_new = (solved && act) ? fma(a.ws, J, a.phi[b]) : 0.0;

        double f_best, alpha = 0.0;
        bool accept;
        if (INIT) {
            act = act && f_new < INFINITY && f_new > -INFINITY;
            accept = act;
            f_best = act ? f_new : NAN;
        } else {
            f_best = live ? a.fbest[b] : 0.0;
            alpha = live ? a.alpha[b] : 0.0;
            accept = act && solved && alpha > 0.0 && f_new <= f_best - a.need[b];
            if (accept) f_best = f_new;
            alpha *= accept ? a.grow : a.shrink;
        }
        if (accept)
            for (int k = sub; k <= M; k += LPT) {
                double g[3];
                wpopt_knot_grad<R>(c0, axs, M, k, g);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const size_t at = k0 + 3 * (size_t)k + ax;
                    a.gbest[at] = fma(a.ws, g[ax], a.through[at]);
                    if (!INIT && k > 0 && k < M) a.waypoints[at] = a.trial[at];
                }
            }
        if (live && sub == 0) {
            if (INIT) {
                a.active[b] = act ? 1 : 0;
                a.objective[2 * (size_t)b] = f_best;
                if (a.accepted) a.accepted[b] = 0;
            } else if (accept && a.accepted) {
                a.accepted[b] += 1;
            }
            if (INIT || accept) {
                a.objective[2 * (size_t)b + 1] = f_best;
                a.fbest[b] = f_best;
            }
        }
        if (!a.propose) return;   // (uniform over the grid: no shuffle follows)

        // the next trial from the best point
        if (INIT) {
            double dmax = 0.0;
            if (act)
                for (int k = sub + (sub == 0 ? LPT : 0); k < M; k += LPT) {   // interior knots of this lane
                    const double s = wpopt_inv_pow<R>(a.times[s0 + k - 1]) + wpopt_inv_pow<R>(a.times[s0 + k]);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        const double c = a.anchor[at];
                        dmax = fmax(dmax, fabs(wpopt_dir(a.gbest[at], s, a.waypoints[at], c - a.max_move, c + a.max_move)));
                    }
                }
            dmax = topt_group_max(dmax);
            alpha = dmax > 0.0 && dmax < INFINITY ? a.initial_step / dmax : 0.0;
        }
        double need = 0.0;
        if (M > 0)
            for (int k = sub; k <= M; k += LPT) {
                const bool inner = act && k > 0 && k < M;
                const double s = inner ? wpopt_inv_pow<R>(a.times[s0 + k - 1]) + wpopt_inv_pow<R>(a.times[s0 + k]) : 1.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const size_t at = k0 + 3 * (size_t)k + ax;
                    const double p = a.waypoints[at];   // (own lane's store above, or untouched)
                    double pt = p;
                    if (inner) {
                        const double g = a.gbest[at], c = a.anchor[at], lo = c - a.max_move, hi = c + a.max_move;
                        const double d = wpopt_dir(g, s, p, lo, hi);
                        pt = fmin(fmax(p - alpha * d, lo), hi);
                        need = fma(g, p - pt, need);
                    }
                    a.trial[at] = pt;
                }
            }
        need = topt_group_sum(need);
        if (live && sub == 0) {
            a.alpha[b] = alpha;
            a.need[b] = a.armijo * need;
        }
    });
}

}  // namespace uavqp
