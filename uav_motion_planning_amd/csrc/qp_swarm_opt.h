// qp_swarm_opt.h -- the per-SWARM step of the swarm optimiser (uavqp_swarm_optimize_device, include/uavqp.h: the objective, the method and
// the rules are there).  Translation unit: k_swarm_opt.hip.
//
// spacetime_step_kernel (qp_spacetime.h) with every per-trajectory quantity made per swarm: one f_g = sum_b f_b + Phi_swarm,g, one alpha,
// three scales (waypoints, log durations, departures) and ONE accept / reject per swarm and trial.  The per-vehicle arithmetic is that of
// spacetime_step_kernel through the same helpers (wpopt_knot_grad, wpopt_dir, wpopt_inv_pow, spacetime_dir_u, topt_segment_cost,
// topt_segment_H).
// Work.  One workgroup of SWOPT_BLOCK lanes takes one swarm (grid-stride over the swarms).  Its SWOPT_BLOCK / TOPT_LPT lane groups
// (qp_poly.h) loop over the swarm's vehicles: vehicle v always goes to lane group v % SWOPT_GROUPS and, inside it, knot k and segment i to
// sub-lane k % TOPT_LPT, i % TOPT_LPT -- in every phase.  Phases, separated by __syncthreads():
//   1. f_b of every vehicle into LDS; lane 0 adds them in vehicle order, adds Phi_swarm,g, decides and broadcasts the decision.
//   2. accepted: every vehicle's best point and gradients are replaced.  INIT: the per-vehicle direction maxima go into LDS and lane 0
//      takes the swarm's three scales from them (a maximum does not depend on the order).
//   3. the next trial of every vehicle; need_b (and the departure's share) into LDS, lane 0 adds them in vehicle order.
// Who reads what.  As in spacetime_step_kernel the trial durations alternate between two arrays and an accepting swarm reads its best
// durations from t_eval, so no lane reads an element another lane writes in the same launch; everything else a lane reads back (best
// waypoints, both best gradients) it has written itself.  A departure time, its trial and its gradient belong to sub-lane 0 of the
// vehicle's group alone.  The per-swarm scalars in memory are read and written by lane 0 only and reach the others through LDS.
// Order of the additions: segments within a vehicle (the butterfly of qp_poly.h), vehicles within the swarm -- indices inside the swarm
// alone: the same bytes run to run, for any grid, and for a swarm alone or in the middle of a batch.  No atomics.
// A swarm of one vehicle with the departures fixed computes, bit for bit, what spacetime_step_kernel computes for that trajectory
// (0 + f_b + 0 and armijo (0 + need_b + 0) are exact).
// A swarm of more than SWARM_MAX vehicles (offsets on the device are trusted; the _host entry refuses it) takes no part: its objective
// is NaN, every trial of its vehicles is their own point, nothing of it goes through LDS.
// Resources (gfx950, `make resource-usage`): DESIGN.md section 5.23.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"
#include "qp_spacetime.h"
#include "qp_swarm.h"

namespace uavqp {

constexpr int SWOPT_BLOCK = 128;                       // two waves
constexpr int SWOPT_GROUPS = SWOPT_BLOCK / TOPT_LPT;   // vehicles in flight per workgroup

struct SwarmOptArgs {
    int n_traj, uniform, n_groups;
    const int32_t* seg_offsets;
    const int32_t* group_offsets;   // null: one swarm, the whole batch
    // per vehicle: the arrays of SpacetimeArgs, same meaning
    double* waypoints;
    double* wp_trial;
    const double* anchor;
    double* gp_best;
    double* times;
    const double* t_eval;
    double* t_next;
    double* gt_best;
    const double* coeff;
    const int32_t* status;
    const double* phi;              // [n_traj] flight penalty of the last solve
    const double* explicit_t;       // [total] explicit dPhi/dT_i, flight + swarm
    const double* through_p;        // [knots][3] d(Phi_flight + Phi_swarm)/dp through the minimiser
    const double* through_t;        // [total] the same in the durations
    int32_t* active;                // [n_traj] workspace: the vehicle takes part
    // departures (start == null: fixed at zero, none of the five arrays is touched)
    double* start;                  // [n_traj] the best (accepted) departures: the caller's array
    double* start_trial;            // [n_traj] what the last swarm penalty ran at / the next trial (one owner lane per element)
    const double* start_anchor;     // [n_traj] the start: centre of the window
    const double* grad_start;       // [n_traj] dPhi_swarm/dstart of the last swarm penalty
    double* gs_best;                // [n_traj] the same at the best point
    // per swarm
    const double* phi_swarm;        // [n_groups] swarm penalty of the last solve
    double* fbest;                  // [n_groups] workspace
    double* alpha;                  // [n_groups] workspace
    double* need;                   // [n_groups] workspace
    double* sigma;                  // [n_groups][3] workspace: waypoints, log durations, departures
    int32_t* g_active;              // [n_groups] workspace
    double* objective;              // [n_groups][2]
    int32_t* accepted;              // [n_groups] or null
    double ws, wt, t_min, t_max, max_move, step_move, step_log, armijo, shrink, grow;
    double window, step_start;
    int propose;                    // 0: last step, no further trial
};

// the departure direction of one vehicle, zero where the window blocks the move
__device__ inline double swarm_dir_s(double g, double s, double lo, double hi) {
    return ((s <= lo && g > 0.0) || (s >= hi && g < 0.0)) ? 0.0 : g;
}

template <int R, bool INIT>
__global__ __launch_bounds__(SWOPT_BLOCK) void swarm_step_kernel(SwarmOptArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT, NG = SWOPT_GROUPS;
    __shared__ double sh_f[SWARM_MAX];        // f_b, then need_b
    __shared__ double sh_s[SWARM_MAX];        // the departure's share of need
    __shared__ double sh_d[3][SWARM_MAX];     // INIT: max |d| of the three blocks per vehicle
    __shared__ int sh_flag[SWARM_MAX];        // bit 0: takes part, bit 1: solved at the point the last solve ran at
    __shared__ double sh_sc[4];               // alpha, sigma_p, sigma_u, sigma_s
    __shared__ int sh_dec[2];                 // accepted, swarm active
    const int tid = threadIdx.x, sub = tid % LPT, grp = tid / LPT;

    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int b0 = a.group_offsets ? a.group_offsets[g] : 0;
        const int A_all = (a.group_offsets ? a.group_offsets[g + 1] : a.n_traj) - b0;
        const bool fits = A_all <= SWARM_MAX;
        const int A = fits ? A_all : 0;
        const int A_round = (A + NG - 1) / NG * NG;               // whole lane groups reach the shuffles
        const int A_all_round = A_all > 0 ? (A_all + NG - 1) / NG * NG : 0;
        __syncthreads();   // (the previous swarm's LDS has been read)

        // ---- phase 1: f_b at the point the last solve ran at
        for (int v = grp; v < A_round; v += NG) {
            const bool live = v < A;
            const int b = b0 + (live ? v : 0);
            const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
            const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
            const size_t axs = (size_t)NC * M;
            const double* __restrict__ c0 = a.coeff + (size_t)3 * NC * s0;
            const bool solved = live && M > 0 && a.status[b] == UAVQP_SOLVED;
            const bool act = INIT ? solved : (live && a.active[b] != 0);
            double J = 0.0, sumT = 0.0;
            if (solved && act)
                for (int i = sub; i < M; i += LPT) {
                    const double T = a.t_eval[s0 + i];
                    J += topt_segment_cost<R>(c0 + (size_t)i * NC, axs, T);
                    sumT += T;
                }
            J = topt_group_sum(J);
            sumT = topt_group_sum(sumT);
            if (live && sub == 0) {
                sh_f[v] = (solved && act) ? fma(a.ws, J, fma(a.wt, sumT, a.phi[b])) : 0.0;
                sh_flag[v] = (act ? 1 : 0) | (solved ? 2 : 0);
            }
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            int n_act = 0;
            bool all_solved = true;
            for (int v = 0; v < A; ++v)
                if (sh_flag[v] & 1) {
                    s += sh_f[v];
                    ++n_act;
                    all_solved = all_solved && (sh_flag[v] & 2) != 0;
                }
            const double f_new = s + a.phi_swarm[g];
            double f_best, alpha = 0.0;
            bool active, accept;
            if (INIT) {
                active = fits && n_act > 0 && f_new < INFINITY && f_new > -INFINITY;
                accept = active;
                f_best = active ? f_new : NAN;
                a.g_active[g] = active ? 1 : 0;
                a.objective[2 * (size_t)g] = f_best;
                if (a.accepted) a.accepted[g] = 0;
            } else {
                active = a.g_active[g] != 0;
                f_best = a.fbest[g];
                alpha = a.alpha[g];
                accept = active && all_solved && alpha > 0.0 && f_new <= f_best - a.need[g];
                if (accept) f_best = f_new;
                alpha *= accept ? a.grow : a.shrink;
                if (accept && a.accepted) a.accepted[g] += 1;
                sh_sc[1] = a.sigma[3 * (size_t)g];
                sh_sc[2] = a.sigma[3 * (size_t)g + 1];
                sh_sc[3] = a.sigma[3 * (size_t)g + 2];
            }
            if (INIT || accept) {
                a.objective[2 * (size_t)g + 1] = f_best;
                a.fbest[g] = f_best;
            }
            sh_sc[0] = alpha;
            sh_dec[0] = accept ? 1 : 0;
            sh_dec[1] = active ? 1 : 0;
        }
        __syncthreads();
        const bool accept = sh_dec[0] != 0, active = sh_dec[1] != 0;

        // ---- phase 2: an accepted swarm replaces the best point and the gradients of every vehicle that takes part
        if (INIT) {
            // (an oversize swarm too: its vehicles are marked as taking no part)
            for (int v = grp; v < A_all_round; v += NG)
                if (v < A_all && sub == 0) a.active[b0 + v] = (active && (sh_flag[fits ? v : 0] & 1)) ? 1 : 0;   // (active implies fits)
        }
        if (accept)
            for (int v = grp; v < A; v += NG) {
                if (!(sh_flag[v] & 1)) continue;
                const int b = b0 + v;
                const PolySpan sp = poly_span(a.uniform, a.seg_offsets, b);
                const int s0 = sp.s0, M = sp.M;
                const size_t axs = (size_t)NC * M;
                const size_t k0 = 3 * ((size_t)s0 + b);
                const double* __restrict__ c0 = a.coeff + (size_t)3 * NC * s0;
                for (int k = sub; k <= M; k += LPT) {
                    double gk[3];
                    wpopt_knot_grad<R>(c0, axs, M, k, gk);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        a.gp_best[at] = fma(a.ws, gk[ax], a.through_p[at]);
                        if (!INIT && k > 0 && k < M) a.waypoints[at] = a.wp_trial[at];
                    }
                }
                for (int i = sub; i < M; i += LPT) {
                    const double H = topt_segment_H<R>(c0 + (size_t)i * NC, axs);
                    a.gt_best[s0 + i] = fma(-a.ws, H, a.wt) + (a.explicit_t[s0 + i] + a.through_t[s0 + i]);
                    if (!INIT) a.times[s0 + i] = a.t_eval[s0 + i];
                }
                if (a.start && sub == 0) {
                    a.gs_best[b] = a.grad_start[b];
                    if (!INIT) a.start[b] = a.start_trial[b];
                }
            }
        if (!a.propose) continue;   // (uniform over the grid)

        if (INIT) {
            // the swarm's scales: initial step / the largest direction component over ALL its vehicles
            for (int v = grp; v < A_round; v += NG) {
                const bool live = v < A;
                const int b = b0 + (live ? v : 0);
                const bool act = live && active && (sh_flag[v] & 1);
                const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
                const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
                const size_t k0 = 3 * ((size_t)s0 + b);
                const double* __restrict__ Tb = a.times;
                double dmax_p = 0.0, dmax_u = 0.0;
                if (act) {
                    for (int k = sub + (sub == 0 ? LPT : 0); k < M; k += LPT) {   // interior knots of this lane
                        const double s = wpopt_inv_pow<R>(Tb[s0 + k - 1]) + wpopt_inv_pow<R>(Tb[s0 + k]);
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const size_t at = k0 + 3 * (size_t)k + ax;
                            const double c = a.anchor[at];
                            dmax_p = fmax(dmax_p, fabs(wpopt_dir(a.gp_best[at], s, a.waypoints[at], c - a.max_move, c + a.max_move)));
                        }
                    }
                    for (int i = sub; i < M; i += LPT)
                        dmax_u = fmax(dmax_u, fabs(spacetime_dir_u(a.gt_best[s0 + i], Tb[s0 + i], a.t_min, a.t_max)));
                }
                dmax_p = topt_group_max(dmax_p);
                dmax_u = topt_group_max(dmax_u);
                if (live && sub == 0) {
                    double ds = 0.0;
                    if (act && a.start) {
                        const double c = a.start_anchor[b];
                        ds = fabs(swarm_dir_s(a.gs_best[b], a.start[b], c - a.window, c + a.window));
                    }
                    sh_d[0][v] = dmax_p;
                    sh_d[1][v] = dmax_u;
                    sh_d[2][v] = ds;
                }
            }
            __syncthreads();
            if (tid == 0) {
                double m[3] = {0.0, 0.0, 0.0};
                for (int v = 0; v < A; ++v)
#pragma unroll
                    for (int q = 0; q < 3; ++q) m[q] = fmax(m[q], sh_d[q][v]);
                const double sig_p = m[0] > 0.0 && m[0] < INFINITY ? a.step_move / m[0] : 0.0;
                const double sig_u = m[1] > 0.0 && m[1] < INFINITY ? a.step_log / m[1] : 0.0;
                const double sig_s = m[2] > 0.0 && m[2] < INFINITY ? a.step_start / m[2] : 0.0;
                sh_sc[0] = (sig_p > 0.0 || sig_u > 0.0 || sig_s > 0.0) ? 1.0 : 0.0;
                sh_sc[1] = sig_p;
                sh_sc[2] = sig_u;
                sh_sc[3] = sig_s;
            }
            __syncthreads();
        }
        const double alpha = sh_sc[0], sig_p = sh_sc[1], sig_u = sh_sc[2], sig_s = sh_sc[3];

        // ---- phase 3: the next trial from the best point; its durations are in t_eval after an accepted trial, else in `times`
        const double* __restrict__ Tb = (!INIT && accept) ? a.t_eval : a.times;
        for (int v = grp; v < A_all_round; v += NG) {
            const bool live = v < A_all;
            const int b = b0 + (live ? v : 0);
            const bool act = live && active && (sh_flag[fits ? v : 0] & 1);   // (active implies fits)
            const PolySpan sp = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
            const int s0 = sp.s0, M = sp.M > 0 ? sp.M : 0;
            const size_t k0 = 3 * ((size_t)s0 + b);
            double need = 0.0;
            if (M > 0)
                for (int k = sub; k <= M; k += LPT) {
                    const bool inner = act && k > 0 && k < M;
                    const double s = inner ? wpopt_inv_pow<R>(Tb[s0 + k - 1]) + wpopt_inv_pow<R>(Tb[s0 + k]) : 1.0;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t at = k0 + 3 * (size_t)k + ax;
                        const double p = a.waypoints[at];   // (own lane's store above, or untouched)
                        double pt = p;
                        if (inner) {
                            const double gq = a.gp_best[at], c = a.anchor[at], lo = c - a.max_move, hi = c + a.max_move;
                            const double d = wpopt_dir(gq, s, p, lo, hi);
                            pt = fmin(fmax(p - alpha * sig_p * d, lo), hi);
                            need = fma(gq, p - pt, need);
                        }
                        a.wp_trial[at] = pt;
                    }
                }
            for (int i = sub; i < M; i += LPT) {
                const double T = Tb[s0 + i];
                double Tt = T;
                if (act) {
                    const double d = spacetime_dir_u(a.gt_best[s0 + i], T, a.t_min, a.t_max);
                    Tt = fmin(fmax(T * exp(-alpha * sig_u * d), a.t_min), a.t_max);
                    need = fma(d, log(T / Tt), need);
                }
                a.t_next[s0 + i] = Tt;
            }
            need = topt_group_sum(need);
            if (live && sub == 0) {
                double need_s = 0.0;
                if (a.start) {
                    const double st = a.start[b];   // (own store above, or untouched)
                    double stt = st;
                    if (act) {
                        const double c = a.start_anchor[b], lo = c - a.window, hi = c + a.window;
                        const double d = swarm_dir_s(a.gs_best[b], st, lo, hi);
                        stt = fmin(fmax(st - alpha * sig_s * d, lo), hi);
                        need_s = d * (st - stt);
                    }
                    a.start_trial[b] = stt;
                }
                if (fits) {
                    sh_f[v] = act ? need : 0.0;
                    sh_s[v] = need_s;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            double nb = 0.0, ns = 0.0;
            for (int v = 0; v < A; ++v) {
                nb += sh_f[v];
                ns += sh_s[v];
            }
            a.alpha[g] = active ? alpha : 0.0;
            a.need[g] = a.armijo * (nb + ns);
            if (INIT) {
                a.sigma[3 * (size_t)g] = sig_p;
                a.sigma[3 * (size_t)g + 1] = sig_u;
                a.sigma[3 * (size_t)g + 2] = sig_s;
            }
        }
    }
}

}  // namespace uavqp
