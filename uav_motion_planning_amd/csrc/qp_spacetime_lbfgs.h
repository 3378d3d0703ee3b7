// qp_spacetime_lbfgs.h -- the per-trajectory step of the joint waypoint / duration optimiser with limited-memory BFGS directions
// (uavqp_spacetime_lbfgs_device, include/uavqp.h: the method is written out there).  Translation unit: k_spacetime_lbfgs.hip.
// Objective, variables, bounds, the three launches in front of the step (solve, flight_penalty_kernel, backward pass) and the accept /
// reject rule are those of spacetime_step_kernel (qp_spacetime.h); only the direction differs.
//
// Lanes.  The lane groups of qp_poly.h: eight lanes per trajectory, sub-lane j owns knots and segments j, j + 8, ....  Every vector of the
// method (the best point, both gradients, the free set, the direction, every stored pair) is laid out like the waypoint array plus the
// durations array, so a lane reads and writes ONLY its own elements of all of them; what the lanes share are the sums, and those go through
// topt_group_sum / topt_group_max: every lane of the group ends with the same bits and takes the same decisions.  The one exception is the
// neighbour's duration in s_k, for which the trial durations alternate between two arrays exactly as in spacetime_step_kernel.  No LDS.
// History.  memory + 1 slots of (s, y) per trajectory: the slot at `head` is never one of the `count` live pairs (they end at head - 1), so
// an accepted trial writes its pair there BEFORE the curvature test, in the same pass that replaces the best point, and the test only
// decides whether head moves on.  head / count / mode / consecutive rejections: four ints per trajectory.
// Loops.  The pair count of a trajectory differs from its wave neighbours'.  Every loop with a shuffle in it runs `memory` trips (uniform
// over the grid) for every lane and a pair that does not exist is predicated out: its partial sum is zero and its update is skipped.  The
// trips are unrolled to UAVQP_LBFGS_MAX_MEMORY so that rho_j and alpha_j stay in registers.  The `memory` masked s.y of the first loop do
// not depend on q and are issued first, one after the other with nothing between them; only the q updates are a chain.
// Working vector.  q, then r, then d of the two-loop recursion: a lane keeps the FIRST round of its elements (knot `kin`, segment `sub`:
// four doubles, and all there is when M <= 8) and their free bits in registers, so that a trip of the chain is loads that do not depend on
// it, one butterfly and an fma per element; its elements of further rounds (M > 8) live in dir_p / dir_u and free_p / free_u.  With
// everything in memory a trip was a store and a dependent load of the same address: 59 us per step at 4096 x 8, r = 4, against 41 us so.
// The same elements of the UAVQP_LBFGS_PRELOAD newest pairs are loaded in ONE batch ahead of both loops: 32 us.
// d is written to dir_p / dir_u at the end either way: a rejected trial reuses it in the next launch.
// Registers (gfx950, `make resource-usage`): <R, false> 256 VGPRs + 85 AGPRs at r = 3 and r = 4, one wave per SIMD, no scratch, SGPRs
// spilled to VGPR lanes; <R, true> 118 / 121 VGPRs.  The step is bound by the latency of its chain, not by occupancy or bytes.
// The order of the additions is fixed by the element and pair indices alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qp_spacetime.h"

#define UAVQP_LBFGS_MAX_MEMORY 16
#define UAVQP_LBFGS_PRELOAD 8   // pairs (the newest) whose register-round elements are loaded ahead of the two loops: the default memory

namespace uavqp {

struct SpacetimeLbfgsArgs {
    SpacetimeArgs g;           // everything spacetime_step_kernel reads and writes, with the same meaning
    double* hist_sp;           // [memory + 1][knots][3]   s of the stored pairs, waypoint part
    double* hist_yp;           // [memory + 1][knots][3]   y
    double* hist_su;           // [memory + 1][total]      s, duration part
    double* hist_yu;           // [memory + 1][total]      y
    double* dir_p;             // [knots][3] the quasi-Newton direction in x (and, past a lane's first round, q and r of the two loops)
    double* dir_u;             // [total]
    double* free_p;            // [knots][3] past a lane's first round: 1.0: the component is free at the best point, 0.0: a bound blocks it
    double* free_u;            // [total]
    int32_t* state;            // [n_traj][4] head, count, mode (0 gradient, 1 quasi-Newton), consecutive rejections
    size_t wp_len, t_len;      // doubles per slot of the two parts
    int memory, max_backtracks;
    double curvature_eps;
};

template <int R, bool INIT>
__global__ __launch_bounds__(64) void spacetime_lbfgs_step_kernel(SpacetimeLbfgsArgs q) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT, MAXM = UAVQP_LBFGS_MAX_MEMORY;
    const SpacetimeArgs& a = q.g;
    topt_for_each_group(a.n_traj, [&](bool live, int b, int sub) {
        const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
        const size_t axs = (size_t)NC * M;
        const size_t k0 = 3 * ((size_t)s0 + b);   // the trajectory's first knot in the waypoint arrays
        const double* __restrict__ c0 = a.coeff + (size_t)3 * NC * s0;
        const bool solved = live && M > 0 && a.status[b] == UAVQP_SOLVED;
        bool act = INIT ? solved : (live && a.active[b] != 0);
        const int kin = sub == 0 ? LPT : sub;     // this lane's first interior knot
        const double sm = a.step_move, sl = a.step_log;

        // f at the point the last solve ran at (the sums of spacetime_step_kernel, in its order)
        double J = 0.0, sumT = 0.0;
        if (solved && act)
            for (int i = sub; i < M; i += LPT) {
                const double T = a.t_eval[s0 + i];
                J += topt_segment_cost<R>(c0 + (size_t)i * NC, axs, T);
                sumT += T;
            }
        J = topt_group_sum(J);
        sumT = topt_group_sum(sumT);
        const double f_new = (solved && act) ? fma(a.ws, J, fma(a.wt, sumT, a.phi[b])) : 0.0;

        double f_best, alpha = 0.0;
        int head = 0, count = 0, mode = 0, rej = 0;
        bool accept;
        if (INIT) {
            act = act && f_new < INFINITY && f_new > -INFINITY;
            accept = act;
            f_best = act ? f_new : NAN;
        } else {
            f_best = live ? a.fbest[b] : 0.0;
            alpha = live ? a.alpha[b] : 0.0;
            if (live) {
                head = q.state[4 * (size_t)b];
                count = q.state[4 * (size_t)b + 1];
                mode = q.state[4 * (size_t)b + 2];
                rej = q.state[4 * (size_t)b + 3];
            }
            accept = act && solved && alpha > 0.0 && f_new <= f_best - a.need[b];
            if (accept) f_best = f_new;
        }
        const int slots = q.memory + 1;

        // An accepted trial: the gradient there, the pair (s, y) = (x_t - x, g_t - g) into the slot at head, the best point replaced --
        // one pass, every element by the lane that owns it.
        double sy = 0.0, ss = 0.0, yy = 0.0;
        if (accept) {
            double* __restrict__ Sp = q.hist_sp + (size_t)head * q.wp_len;
            double* __restrict__ Yp = q.hist_yp + (size_t)head * q.wp_len;
            double* __restrict__ Su = q.hist_su + (size_t)head * q.t_len;
            double* __restrict__ Yu = q.hist_yu + (size_t)head * q.t_len;
            for (int k = sub; k <= M; k += LPT) {
                double g[3];
                wpopt_knot_grad<R>(c0, axs, M, k, g);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const size_t at = k0 + 3 * (size_t)k + ax;
                    const double g_t = fma(a.ws, g[ax], a.through_p[at]);
                    if (!INIT && k > 0 && k < M) {
                        const double p = a.waypoints[at], pt = a.wp_trial[at];
                        const double s = (pt - p) / sm, y = sm * (g_t - a.gp_best[at]);
                        Sp[at] = s;
                        Yp[at] = y;
                        sy = fma(s, y, sy);
                        ss = fma(s, s, ss);
                        yy = fma(y, y, yy);
                        a.waypoints[at] = pt;
                    }
                    a.gp_best[at] = g_t;
                }
            }
            for (int i = sub; i < M; i += LPT) {
                const double H = topt_segment_H<R>(c0 + (size_t)i * NC, axs);
                const double g_t = fma(-a.ws, H, a.wt) + (a.explicit_t[s0 + i] + a.through_t[s0 + i]);
                if (!INIT) {
                    const double T = a.times[s0 + i], Tt = a.t_eval[s0 + i];
                    const double s = log(Tt / T) / sl, y = sl * (Tt * g_t - T * a.gt_best[s0 + i]);
                    Su[s0 + i] = s;
                    Yu[s0 + i] = y;
                    sy = fma(s, y, sy);
                    ss = fma(s, s, ss);
                    yy = fma(y, y, yy);
                    a.times[s0 + i] = Tt;
                }
                a.gt_best[s0 + i] = g_t;
            }
        }
        if (!INIT) {
            sy = topt_group_sum(sy);
            ss = topt_group_sum(ss);
            yy = topt_group_sum(yy);
            if (accept && sy > q.curvature_eps * (sqrt(ss) * sqrt(yy))) {   // the pair is kept: the ring moves on, the oldest pair drops out
                head = head + 1 == slots ? 0 : head + 1;
                count = count < q.memory ? count + 1 : q.memory;
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

        // the best durations are in t_eval after an accepted trial, else in `times` (INIT: the same array); a lane's OWN durations are
        // in `times` either way (its store above)
        const double* __restrict__ Tb = (!INIT && accept) ? a.t_eval : a.times;

        // which direction comes next
        bool new_qn = false, enter_gd = INIT;
        if (!INIT) {
            if (accept) {
                rej = 0;
                new_qn = count > 0;
                if (!new_qn) alpha *= a.grow;        // gradient mode goes on
            } else {
                alpha *= a.shrink;
                if (mode == 1 && ++rej >= q.max_backtracks) {
                    count = 0;
                    enter_gd = true;
                }
            }
        }

        if (!INIT) {
            // ---- quasi-Newton direction: the two-loop recursion over the stored pairs on the free set of the best point
            double w[4] = {0.0, 0.0, 0.0, 0.0};   // the working vector at knot kin (three axes) and segment sub
            unsigned fm = 0;                      // bit c: component c of w is free
            const bool has_k = kin < M, has_i = sub < M;
            // g_F of one component, and whether it is free
            auto g_free_p = [&](size_t at, bool& fr) {
                const double g = a.gp_best[at], p = a.waypoints[at], c = a.anchor[at];
                fr = !((p <= c - a.max_move && g > 0.0) || (p >= c + a.max_move && g < 0.0));
                return fr ? sm * g : 0.0;
            };
            auto g_free_u = [&](size_t at, bool& fr) {
                const double T = a.times[at], g = T * a.gt_best[at];
                fr = !((T <= a.t_min && g > 0.0) || (T >= a.t_max && g < 0.0));
                return fr ? sl * g : 0.0;
            };
            // fn(v, free, index, is_u) over the lane's elements, the round in registers first: v the working value (a register, or the
            // element of dir_p / dir_u), index into the waypoint layout (is_u false) or the durations layout (is_u true)
            // and the component of the register round (0 .. 2: axis of knot kin, 3: segment sub) or -1
            const size_t at_k = k0 + 3 * (size_t)kin, at_i = (size_t)s0 + sub;
            auto each = [&](auto&& fn) {
                if (has_k) {
                    fn(w[0], (fm & 1u) != 0, at_k, std::false_type{}, std::integral_constant<int, 0>{});
                    fn(w[1], (fm & 2u) != 0, at_k + 1, std::false_type{}, std::integral_constant<int, 1>{});
                    fn(w[2], (fm & 4u) != 0, at_k + 2, std::false_type{}, std::integral_constant<int, 2>{});
                }
                if (has_i) fn(w[3], (fm & 8u) != 0, at_i, std::true_type{}, std::integral_constant<int, 3>{});
                for (int k = kin + LPT; k < M; k += LPT)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        fn(q.dir_p[at], q.free_p[at] != 0.0, at, std::false_type{}, std::integral_constant<int, -1>{});
                    }
                for (int i = sub + LPT; i < M; i += LPT)
                    fn(q.dir_u[s0 + i], q.free_u[s0 + i] != 0.0, (size_t)s0 + i, std::true_type{}, std::integral_constant<int, -1>{});
            };
            // The pairs' elements of the register round, ages 0 .. PRE - 1, loaded ONCE and all at a time, before anything waits for them:
            // neither loop then has a load in its chain (M <= 8, memory <= PRE).  A slot past `count` holds stale bytes; it is never used.
            constexpr int PRE = UAVQP_LBFGS_PRELOAD;
            double Sr[PRE][4], Yr[PRE][4];
#pragma unroll
            for (int j = 0; j < PRE; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) Sr[j][c] = Yr[j][c] = 0.0;
            if (new_qn && has_k)
#pragma unroll
                for (int j = 0; j < PRE; ++j)
                    if (j < q.memory) {
                        const int s = head - 1 - j;
                        const size_t o = (size_t)(s < 0 ? s + slots : s) * q.wp_len + at_k;
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            Sr[j][ax] = q.hist_sp[o + ax];
                            Yr[j][ax] = q.hist_yp[o + ax];
                        }
                    }
            if (new_qn && has_i)
#pragma unroll
                for (int j = 0; j < PRE; ++j)
                    if (j < q.memory) {
                        const int s = head - 1 - j;
                        const size_t o = (size_t)(s < 0 ? s + slots : s) * q.t_len + at_i;
                        Sr[j][3] = q.hist_su[o];
                        Yr[j][3] = q.hist_yu[o];
                    }
            // s_j / y_j of one element: from the registers where they were preloaded
#define UAVQP_LBFGS_S(j, at, u, c) ((decltype(c)::value >= 0 && (j) < PRE) ? Sr[(j) < PRE ? (j) : 0][decltype(c)::value >= 0 ? decltype(c)::value : 0] : (decltype(u)::value ? Su[at] : Sp[at]))
#define UAVQP_LBFGS_Y(j, at, u, c) ((decltype(c)::value >= 0 && (j) < PRE) ? Yr[(j) < PRE ? (j) : 0][decltype(c)::value >= 0 ? decltype(c)::value : 0] : (decltype(u)::value ? Yu[at] : Yp[at]))
            double gg = 0.0;
            if (new_qn) {   // q = g_F, and the free set
                bool fr;
                if (has_k)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        w[ax] = g_free_p(k0 + 3 * (size_t)kin + ax, fr);
                        fm |= (fr ? 1u : 0u) << ax;
                        gg = fma(w[ax], w[ax], gg);
                    }
                if (has_i) {
                    w[3] = g_free_u((size_t)s0 + sub, fr);
                    fm |= (fr ? 1u : 0u) << 3;
                    gg = fma(w[3], w[3], gg);
                }
                for (int k = kin + LPT; k < M; k += LPT)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        const double v = g_free_p(at, fr);
                        q.free_p[at] = fr ? 1.0 : 0.0;
                        q.dir_p[at] = v;
                        gg = fma(v, v, gg);
                    }
                for (int i = sub + LPT; i < M; i += LPT) {
                    const double v = g_free_u((size_t)s0 + i, fr);
                    q.free_u[s0 + i] = fr ? 1.0 : 0.0;
                    q.dir_u[s0 + i] = v;
                    gg = fma(v, v, gg);
                }
            }
            // pair of age j (0: the newest) sits in slot head - 1 - j
            auto slot_of = [&](int j) { const int s = head - 1 - j; return (size_t)(s < 0 ? s + slots : s); };
            double rho[MAXM], al[MAXM], yy0 = 0.0;
            // the masked s.y of every pair: independent of q and of each other
#pragma unroll
            for (int j = 0; j < MAXM; ++j) {
                rho[j] = 0.0;
                al[j] = 0.0;
                if (j < q.memory) {
                    double part = 0.0, part_y = 0.0;
                    if (new_qn && j < count) {
                        const size_t sl_ = slot_of(j);
                        const double* __restrict__ Sp = q.hist_sp + sl_ * q.wp_len;
                        const double* __restrict__ Yp = q.hist_yp + sl_ * q.wp_len;
                        const double* __restrict__ Su = q.hist_su + sl_ * q.t_len;
                        const double* __restrict__ Yu = q.hist_yu + sl_ * q.t_len;
                        each([&](double&, bool fr, size_t at, auto u, auto c) {
                            if (fr) {
                                const double s = UAVQP_LBFGS_S(j, at, u, c), y = UAVQP_LBFGS_Y(j, at, u, c);
                                part = fma(s, y, part);
                                if (j == 0) part_y = fma(y, y, part_y);
                            }
                        });
                    }
                    rho[j] = topt_group_sum(part);
                    if (j == 0) yy0 = topt_group_sum(part_y);
                }
            }
            // first loop, newest to oldest: alpha_j = s_j . q / s_j . y_j, q -= alpha_j y_j
#pragma unroll
            for (int j = 0; j < MAXM; ++j)
                if (j < q.memory) {
                    const bool on = new_qn && j < count && rho[j] > 0.0;
                    const size_t sl_ = slot_of(j);
                    const double* __restrict__ Sp = q.hist_sp + sl_ * q.wp_len;
                    const double* __restrict__ Yp = q.hist_yp + sl_ * q.wp_len;
                    const double* __restrict__ Su = q.hist_su + sl_ * q.t_len;
                    const double* __restrict__ Yu = q.hist_yu + sl_ * q.t_len;
                    double part = 0.0;
                    if (on)   // (q is zero where a bound blocks it)
                        each([&](double& v, bool, size_t at, auto u, auto c) { part = fma(UAVQP_LBFGS_S(j, at, u, c), v, part); });
                    part = topt_group_sum(part);
                    if (on) {
                        const double aj = part / rho[j];
                        al[j] = aj;
                        each([&](double& v, bool fr, size_t at, auto u, auto c) {
                            if (fr) v = fma(-aj, UAVQP_LBFGS_Y(j, at, u, c), v);
                        });
                    }
                }
            // r = gamma q, gamma = s.y / y.y of the newest pair on the free set
            const double gamma = yy0 > 0.0 ? rho[0] / yy0 : 0.0;
            const bool gamma_ok = gamma > 0.0 && gamma < INFINITY;
            if (new_qn) each([&](double& v, bool, size_t, auto, auto) { v *= gamma; });
            // second loop, oldest to newest: r += s_j (alpha_j - y_j . r / s_j . y_j)
#pragma unroll
            for (int j = MAXM - 1; j >= 0; --j)
                if (j < q.memory) {
                    const bool on = new_qn && j < count && rho[j] > 0.0;
                    const size_t sl_ = slot_of(j);
                    const double* __restrict__ Sp = q.hist_sp + sl_ * q.wp_len;
                    const double* __restrict__ Yp = q.hist_yp + sl_ * q.wp_len;
                    const double* __restrict__ Su = q.hist_su + sl_ * q.t_len;
                    const double* __restrict__ Yu = q.hist_yu + sl_ * q.t_len;
                    double part = 0.0;
                    if (on) each([&](double& v, bool, size_t at, auto u, auto c) { part = fma(UAVQP_LBFGS_Y(j, at, u, c), v, part); });
                    part = topt_group_sum(part);
                    if (on) {
                        const double wj = al[j] - part / rho[j];
                        each([&](double& v, bool fr, size_t at, auto u, auto c) {
                            if (fr) v = fma(wj, UAVQP_LBFGS_S(j, at, u, c), v);
                        });
                    }
                }
            // d = -r into dir_p / dir_u, and whether it descends: g_F . d < -1e-10 |g_F| |d|
            double gd = 0.0, dd = 0.0;
            if (new_qn)
                each([&](double& v, bool fr, size_t at, auto u, auto) {
                    const double d = -v;
                    double g = 0.0;
                    if (decltype(u)::value) {
                        if (fr) g = sl * (a.times[at] * a.gt_best[at]);
                        q.dir_u[at] = d;
                    } else {
                        if (fr) g = sm * a.gp_best[at];
                        q.dir_p[at] = d;
                    }
                    gd = fma(g, d, gd);
                    dd = fma(d, d, dd);
                });
#undef UAVQP_LBFGS_S
#undef UAVQP_LBFGS_Y
            gd = topt_group_sum(gd);
            dd = topt_group_sum(dd);
            gg = topt_group_sum(gg);
            if (new_qn) {
                if (gamma_ok && gd < -1e-10 * (sqrt(gg) * sqrt(dd))) {
                    mode = 1;
                    alpha = 1.0;
                    rej = 0;
                } else {   // the memory is cleared and the gradient direction takes over
                    count = 0;
                    enter_gd = true;
                }
            }
        }

        // ---- gradient mode: the direction of spacetime_step_kernel, its two scales renewed at the best point whenever the mode is entered
        double sig_p, sig_u;
        {
            double dmax_p = 0.0, dmax_u = 0.0;
            if (act && enter_gd) {
                for (int k = kin; k < M; k += LPT) {
                    const double s = wpopt_inv_pow<R>(Tb[s0 + k - 1]) + wpopt_inv_pow<R>(Tb[s0 + k]);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        const double c = a.anchor[at];
                        dmax_p = fmax(dmax_p, fabs(wpopt_dir(a.gp_best[at], s, a.waypoints[at], c - a.max_move, c + a.max_move)));
                    }
                }
                for (int i = sub; i < M; i += LPT) dmax_u = fmax(dmax_u, fabs(spacetime_dir_u(a.gt_best[s0 + i], Tb[s0 + i], a.t_min, a.t_max)));
            }
            dmax_p = topt_group_max(dmax_p);
            dmax_u = topt_group_max(dmax_u);
            if (enter_gd) {
                sig_p = dmax_p > 0.0 && dmax_p < INFINITY ? a.step_move / dmax_p : 0.0;
                sig_u = dmax_u > 0.0 && dmax_u < INFINITY ? a.step_log / dmax_u : 0.0;
                alpha = (sig_p > 0.0 || sig_u > 0.0) ? 1.0 : 0.0;
                mode = 0;
                rej = 0;
            } else {
                sig_p = live ? a.sigma[2 * (size_t)b] : 0.0;
                sig_u = live ? a.sigma[2 * (size_t)b + 1] : 0.0;
            }
        }

        // ---- the next trial from the best point, and the decrease it has to reach: armijo g . (x - x_t)
        double need = 0.0;
        if (M > 0)
            for (int k = sub; k <= M; k += LPT) {
                const bool inner = act && k > 0 && k < M;
                const double s = (inner && mode == 0) ? wpopt_inv_pow<R>(Tb[s0 + k - 1]) + wpopt_inv_pow<R>(Tb[s0 + k]) : 1.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const size_t at = k0 + 3 * (size_t)k + ax;
                    const double p = a.waypoints[at];   // (own lane's store above, or untouched)
                    double pt = p;
                    if (inner) {
                        const double g = a.gp_best[at], c = a.anchor[at], lo = c - a.max_move, hi = c + a.max_move;
                        if (mode == 0) {
                            const double d = wpopt_dir(g, s, p, lo, hi);
                            pt = fmin(fmax(p - alpha * sig_p * d, lo), hi);
                        } else {
                            pt = fmin(fmax(fma(alpha * sm, q.dir_p[at], p), lo), hi);
                        }
                        need = fma(g, p - pt, need);
                    }
                    a.wp_trial[at] = pt;
                }
            }
        for (int i = sub; i < M; i += LPT) {
            const double T = Tb[s0 + i];
            double Tt = T;
            if (act) {
                if (mode == 0) {
                    const double d = spacetime_dir_u(a.gt_best[s0 + i], T, a.t_min, a.t_max);
                    Tt = fmin(fmax(T * exp(-alpha * sig_u * d), a.t_min), a.t_max);
                    need = fma(d, log(T / Tt), need);
                } else {
                    Tt = fmin(fmax(T * exp(alpha * sl * q.dir_u[s0 + i]), a.t_min), a.t_max);
                    need = fma(T * a.gt_best[s0 + i], log(T / Tt), need);
                }
            }
            a.t_next[s0 + i] = Tt;
        }
        need = topt_group_sum(need);
        if (live && sub == 0) {
            a.alpha[b] = alpha;
            a.need[b] = a.armijo * need;
            if (enter_gd) {
                a.sigma[2 * (size_t)b] = sig_p;
                a.sigma[2 * (size_t)b + 1] = sig_u;
            }
            q.state[4 * (size_t)b] = head;
            q.state[4 * (size_t)b + 1] = count;
            q.state[4 * (size_t)b + 2] = mode;
            q.state[4 * (size_t)b + 3] = rej;
        }
    });
}

}  // namespace uavqp
