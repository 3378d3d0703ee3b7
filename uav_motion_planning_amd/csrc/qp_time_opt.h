// qp_time_opt.h -- control cost of solved trajectories, its exact gradient with respect to the segment durations, and the
// per-trajectory step of the duration optimiser (uavqp_cost_time_gradient_device / uavqp_time_optimize_device, include/uavqp.h).
//
// Cost.  J = sum over axes and segments of integral_0^{T_i} (p_i^(r)(t))^2 dt = c' P c with the reference's P (getHessian,
// minimum_control.cpp:5-19) -- TWICE the OSQP objective 1/2 x' P x.  Per segment and axis, with a_k = (r+k)!/k! c_{r+k} T^k, k = 0..r-1:
//     J_seg = T * sum_{k,l} a_k a_l / (k + l + 1)                                       (the closed-form block of P, no quadrature)
// Gradient.  In the knot-derivative (Hermite) variables the constraints of the equality QP do not depend on T and every segment is the
// unique degree-(2r-1) interpolant of its two knot states, so at the minimiser (envelope theorem)
//     dJ/dT_i = -H_i,   H_i = (p^(r))^2 + 2 sum_{m=1}^{r-1} (-1)^m p^(r+m) p^(r-m)   summed over the three axes,
// H being constant along a segment; at local time 0, p^(k)(0) = k! c_k: read straight from the stored coefficients.
//   r = 3: H = j^2 - 2 s a + 2 c v          r = 4: H = s^2 - 2 c j + 2 p a - 2 q v        (v a j s c p q = derivatives 1..7 at t = 0)
// This holds for the equality-constrained solve (and for knot boxes); NOT for rows placed at a fraction of T_i.
//
// Lanes.  The lane groups of qp_poly.h (topt_for_each_group, topt_group_sum / topt_group_max), as realloc_kernel (qp_samplers.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"

namespace uavqp {

// c' P c of one segment, three axes (c: the segment's coefficients of axis 0, axis stride in doubles)
template <int R>
__device__ inline double topt_segment_cost(const double* __restrict__ c, size_t axis_stride, double T) {
    double J = 0.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double* ca = c + (size_t)ax * axis_stride;
        double a[R];
        double tp = 1.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            a[k] = topt_falling(R + k, R) * ca[R + k] * tp;
            tp *= T;
        }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            s = fma(a[k] * a[k], 1.0 / (double)(2 * k + 1), s);
#pragma unroll
            for (int l = k + 1; l < R; ++l) s = fma(a[k] * a[l], 2.0 / (double)(k + l + 1), s);
        }
        J = fma(s, T, J);
    }
    return J;
}

// H of one segment, three axes: dJ/dT = -H
template <int R>
__device__ inline double topt_segment_H(const double* __restrict__ c, size_t axis_stride) {
    double H = 0.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double* ca = c + (size_t)ax * axis_stride;
        double d[2 * R];   // p^(k)(0) = k! c_k
#pragma unroll
        for (int k = 1; k < 2 * R; ++k) d[k] = topt_falling(k, k) * ca[k];
        double h = d[R] * d[R];
#pragma unroll
        for (int m = 1; m < R; ++m) h = fma((m & 1) ? -2.0 * d[R + m] : 2.0 * d[R + m], d[R - m], h);
        H += h;
    }
    return H;
}

// ---------------------------------------------------------------------------------------------------
// cost[b] = J_b, grad[s0_b + i] = dJ_b / dT_i of solved trajectories (either output may be null)
// ---------------------------------------------------------------------------------------------------
struct CostGradArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    double* cost;
    double* grad;
};

template <int R>
__global__ __launch_bounds__(64) void cost_grad_kernel(CostGradArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        double J = 0.0;
        for (int i = sub; i < M; i += LPT) {
            const double* __restrict__ c = a.coeff + (size_t)3 * NC * s0 + (size_t)i * NC;
            if (a.cost) J += topt_segment_cost<R>(c, axs, a.times[s0 + i]);
            if (a.grad) a.grad[s0 + i] = -topt_segment_H<R>(c, axs);
        }
        J = topt_group_sum(J);
        if (live && a.cost && sub == 0) a.cost[b] = J;
    });
}

// ---------------------------------------------------------------------------------------------------
// Duration optimiser: minimise f(T) = J(T) + w sum_i T_i over t_min <= T_i <= t_max, per trajectory, by a projected gradient method in
// u_i = log T_i (direction d_i = T_i (dJ/dT_i + w), zero where a bound blocks it) with Armijo backtracking.  The host enqueues
// clamp, solve, step<INIT>, then max_iters x { solve at the trial durations, step<ITER> }; every decision is taken here, per trajectory.
//   clamp  durations of a trajectory whose durations are all positive and finite are projected into the bounds (others: untouched)
//   INIT   status SOLVED and f finite -> the trajectory takes part: f_best = f, gradient stored, step length alpha = initial_step / max |d_i|
//          (the first trial changes the most sensitive duration by initial_step in log T), first trial written
//          otherwise it does not: its trial durations are its own, so every later solve flags it the same way
//   ITER   the trial was solved into `coeff`: accepted iff its status is SOLVED and f_trial <= f_best - armijo * sum_i d_i (u_i - u_trial_i)
//          (sufficient decrease along the projection arc) -> durations, f_best, gradient replaced, alpha *= grow; else alpha *= shrink.
//          Then the next trial from the best point (not after the last iteration).
// LIMITS (uavqp_time_optimize_limits_device; kernels of qp_limits.h run between the solve and the step): f gains the limit penalty
//          phi[b] of the point the last solve ran at, dJ/dT_i its two gradient parts there, lim_explicit[i] + lim_through[i] (the explicit
//          one and the one through c*(T), qp_adjoint.h).  LIMITS = false reads none of the three and is the code it was.
// ---------------------------------------------------------------------------------------------------
struct TimeOptArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    double* times;            // the best (accepted) durations: the caller's array
    double* trial;            // [total] trial durations (workspace)
    double* gbest;            // [total] dJ/dT at the best durations (workspace)
    const double* coeff;      // the solve at `times` (INIT) / at `trial` (ITER)
    const int32_t* status;    // its status
    double* fbest;            // [n_traj] workspace
    double* alpha;            // [n_traj] workspace
    double* need;             // [n_traj] workspace: the decrease the pending trial has to reach
    int32_t* active;          // [n_traj] workspace
    double* objective;        // [n_traj][2]: f at the start, f at the best point
    int32_t* accepted;        // [n_traj] or null
    double w, t_min, t_max, initial_step, armijo, shrink, grow;
    int propose;              // 0: last step, no further trial
    const double* phi;            // LIMITS only: [n_traj] penalty at the point of `coeff`
    const double* lim_explicit;   // LIMITS only: [total] dPhi/dT_i at fixed coefficients
    const double* lim_through;    // LIMITS only: [total] dPhi/dT_i through the minimiser
};

template <int R>
__global__ __launch_bounds__(64) void time_opt_clamp_kernel(TimeOptArgs a) {
    constexpr int LPT = TOPT_LPT;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        double bad = 0.0;
        for (int i = sub; i < M; i += LPT) {
            const double T = a.times[s0 + i];
            if (!(T > 0.0 && T < INFINITY)) bad = 1.0;
        }
        bad = topt_group_max(bad);
        if (bad == 0.0)
            for (int i = sub; i < M; i += LPT) a.times[s0 + i] = fmin(fmax(a.times[s0 + i], a.t_min), a.t_max);
    });
}

template <int R, bool INIT, bool LIMITS = false>
__global__ __launch_bounds__(64) void time_opt_step_kernel(TimeOptArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
        const size_t axs = (size_t)NC * M;
        const double* __restrict__ T_eval = INIT ? a.times : a.trial;
        const bool solved = live && M > 0 && a.status[b] == UAVQP_SOLVED;
        bool act = INIT ? solved : (live && a.active[b] != 0);

        // f at the point the last solve ran at
        double J = 0.0, sumT = 0.0;
        if (solved && act)
            for (int i = sub; i < M; i += LPT) {
                const double T = T_eval[s0 + i];
                J += topt_segment_cost<R>(a.coeff + (size_t)3 * NC * s0 + (size_t)i * NC, axs, T);
                sumT += T;
            }
        J = topt_group_sum(J);
        sumT = topt_group_sum(sumT);
        double f_new = fma(a.w, sumT, J);
        if (LIMITS) f_new += (solved && act) ? a.phi[b] : 0.0;

        double f_best, alpha = 0.0;
        bool accept;
        if (INIT) {
            act = act && f_new < INFINITY && f_new > -INFINITY;
            accept = act;
            f_best = act ? f_new : NAN;
        } else {
            f_best = live ? a.fbest[b] : 0.0;
            alpha = live ? a.alpha[b] : 0.0;
            accept = act && solved && f_new <= f_best - a.need[b];
            if (accept) f_best = f_new;
            alpha *= accept ? a.grow : a.shrink;
        }
        if (accept)
            for (int i = sub; i < M; i += LPT) {
                double gT = -topt_segment_H<R>(a.coeff + (size_t)3 * NC * s0 + (size_t)i * NC, axs);
                if (LIMITS) gT += a.lim_explicit[s0 + i] + a.lim_through[s0 + i];
                a.gbest[s0 + i] = gT;
                if (!INIT) a.times[s0 + i] = a.trial[s0 + i];
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
        double dmax = 0.0;
        if (INIT) {
            if (act)
                for (int i = sub; i < M; i += LPT) {
                    const double T = a.times[s0 + i];
                    double d = T * (a.gbest[s0 + i] + a.w);
                    if ((T <= a.t_min && d > 0.0) || (T >= a.t_max && d < 0.0)) d = 0.0;
                    dmax = fmax(dmax, fabs(d));
                }
            dmax = topt_group_max(dmax);
            alpha = dmax > 0.0 ? a.initial_step / dmax : 0.0;
        }
        double need = 0.0;
        for (int i = sub; i < M; i += LPT) {
            const double T = a.times[s0 + i];   // (own lane's store above, or untouched)
            double Tt = T;
            if (act) {
                double d = T * (a.gbest[s0 + i] + a.w);
                if ((T <= a.t_min && d > 0.0) || (T >= a.t_max && d < 0.0)) d = 0.0;
                Tt = fmin(fmax(T * exp(-alpha * d), a.t_min), a.t_max);
                need = fma(d, log(T / Tt), need);
            }
            a.trial[s0 + i] = Tt;
        }
        need = topt_group_sum(need);
        if (live && sub == 0) {
            a.alpha[b] = alpha;
            a.need[b] = a.armijo * need;
        }
    });
}

}  // namespace uavqp
