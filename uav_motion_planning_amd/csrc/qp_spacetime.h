// qp_spacetime.h -- the fused flight penalty (velocity / acceleration limits + clearance against a distance field in ONE launch) and the
// per-trajectory step of the joint waypoint / duration optimiser (uavqp_flight_penalty_device / uavqp_spacetime_optimize_device,
// include/uavqp.h).  Translation unit: k_spacetime.hip.
//
// Penalty.  Phi = Phi_lim + Phi_clr, the two formulas of qp_limits.h and qp_esdf.h, each with its own samples per segment K_l, K_c.
// Lanes: the lane groups of qp_poly.h, eight lanes per trajectory, sub-lane j owns segments j, j + 8, ....  A lane loads the 3 * 2r
// coefficients and the duration of its segment ONCE, runs the K_l + 1 limit samples and then the K_c + 1 clearance samples over the same
// registers, and keeps ONE set of 3 * 2r partial sums of dPhi/dc: every sample adds its term already weighted with its own (T / K) om_s,
// so the set is stored as it stands, once per segment.  The two scalar sums per part (penalty and explicit time derivative) stay apart
// until the segment ends: Phi_i / T_i is each part's own sum over K.  Every output element is written exactly once, zeros included; the
// order of the additions is fixed by the sample and segment indices alone.
// A part none of whose outputs is asked for and whose weights are zero is not sampled (uniform over the grid).
// Registers (gfx950, `make resource-usage`): 247 VGPRs at r = 3 and ALL 256 at r = 4 (one wave per SIMD), no scratch, some SGPRs spilled to
// VGPR lanes.  r = 4 sits on the ceiling: anything added to the two sample functions goes to scratch without a word from the compiler, so
// look at the resource report after touching them.
//
// Step.  waypoint_opt_step_kernel (qp_waypoint_opt.h) and time_opt_step_kernel (qp_time_opt.h) joined: one f, one accept / reject per
// trajectory, two blocks of variables with a scale each.  See the comment above spacetime_step_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"
#include "qp_time_opt.h"
#include "qp_limits.h"
#include "qp_esdf.h"
#include "qp_waypoint_opt.h"

namespace uavqp {

struct FlightArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    double* penalty;          // [n_traj] or null
    double* grad_coeff;       // layout of coeff, or null
    double* grad_times;       // [sum M] or null
    double* peak;             // [n_traj][2] or null
    double* min_dist;         // [n_traj] or null
    int32_t* outside;         // [n_traj] or null
    int K_lim, K_clr;         // samples per segment of the two parts
    int al16;                 // coeff and grad_coeff are 16-byte aligned
    int do_lim, do_clr;       // 0: the part is not sampled (weights zero and none of its diagnostics asked for)
    double v_max, a_max, inv_v2, inv_a2, wv, wa;
    double d_safe, inv_safe, weight;
    EsdfView map;
};

// One limit sample of a segment at local time t = tau T: the term of limit_penalty_kernel, its coefficient gradient weighted with w = (T / K) om.
template <int NC>
__device__ __forceinline__ void flight_limit_sample(const double (&c)[3][NC], double t, double tau, double om, double w, const FlightArgs& a,
                                                    double& phi, double& dT, double& vv_max, double& aa_max, double (&gc)[3][NC]) {
    double v[3], ac[3], jk[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        v[ax] = poly_deriv<NC, 1>(c[ax], t);
        ac[ax] = poly_deriv<NC, 2>(c[ax], t);
        jk[ax] = poly_deriv<NC, 3>(c[ax], t);
    }
    const double vv = fma(v[0], v[0], fma(v[1], v[1], v[2] * v[2]));
    const double aa = fma(ac[0], ac[0], fma(ac[1], ac[1], ac[2] * ac[2]));
    vv_max = fmax(vv_max, vv);
    aa_max = fmax(aa_max, aa);
    const double pv = fmax(0.0, fma(vv, a.inv_v2, -1.0)), pa = fmax(0.0, fma(aa, a.inv_a2, -1.0));
    phi = fma(om, fma(a.wv * pv, pv * pv, a.wa * pa * (pa * pa)), phi);
    const double cv = 6.0 * a.wv * (pv * pv) * a.inv_v2, ca = 6.0 * a.wa * (pa * pa) * a.inv_a2;
    if (cv != 0.0 || ca != 0.0) {
        const double va = fma(v[0], ac[0], fma(v[1], ac[1], v[2] * ac[2]));
        const double aj = fma(ac[0], jk[0], fma(ac[1], jk[1], ac[2] * jk[2]));
        dT = fma(om * tau, fma(cv, va, ca * aj), dT);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double gv = w * cv * v[ax], ga = w * ca * ac[ax];
            double p2 = 1.0, p1 = t;   // t^(k-2), t^(k-1)
            gc[ax][1] += gv;
#pragma unroll
            for (int k = 2; k < NC; ++k) {
                gc[ax][k] = fma(gv * topt_falling(k, 1), p1, fma(ga * topt_falling(k, 2), p2, gc[ax][k]));
                p2 = p1;
                p1 *= t;
            }
        }
    }
}

// One clearance sample: the term of clearance_penalty_kernel, weighted likewise.  false: the sample lies outside the map.
template <int NC>
__device__ __forceinline__ bool flight_clearance_sample(const double (&c)[3][NC], double t, double tau, double om, double w, const FlightArgs& a,
                                                        double& phi, double& dT, double& neg_min, double (&gc)[3][NC]) {
    double p[3], v[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        p[ax] = poly_deriv<NC, 0>(c[ax], t);
        v[ax] = poly_deriv<NC, 1>(c[ax], t);
    }
    double d, gd[3];
    if (!esdf_sample(a.map, p[0], p[1], p[2], d, gd)) return false;
    neg_min = fmax(neg_min, -d);
    const double x = fmax(0.0, (a.d_safe - d) * a.inv_safe);
    if (x > 0.0) {
        phi = fma(om, a.weight * x * (x * x), phi);
        const double e = -3.0 * a.weight * (x * x) * a.inv_safe;
        dT = fma(om * tau, e * fma(gd[0], v[0], fma(gd[1], v[1], gd[2] * v[2])), dT);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double wg = w * e * gd[ax];
            double pk = t;
            gc[ax][0] += wg;
#pragma unroll
            for (int k = 1; k < NC; ++k) {
                gc[ax][k] = fma(wg, pk, gc[ax][k]);
                pk *= t;
            }
        }
    }
    return true;
}

template <int R>
__global__ __launch_bounds__(64) void flight_penalty_kernel(FlightArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    // (the loop of topt_for_each_group written out, as in the two kernels this one fuses)
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;  // whole waves take part in the shuffles
    const double inv_Kl = 1.0 / (double)a.K_lim, inv_Kc = 1.0 / (double)a.K_clr;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = live && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        double Phi_l = 0.0, Phi_c = 0.0, vv_max = 0.0, aa_max = 0.0, neg_min = -INFINITY;   // (the minimum as a maximum of negatives)
        int n_out = 0;
        for (int i = sub; i < M; i += LPT) {
            const size_t at = (size_t)3 * NC * s0 + (size_t)i * NC;
            double gc[3][NC];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int k = 0; k < NC; ++k) gc[ax][k] = 0.0;
            double phi_l = 0.0, dT_l = 0.0, phi_c = 0.0, dT_c = 0.0, T = 0.0;
            if (solved) {
                T = a.times[s0 + i];
                double c[3][NC];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_load<NC>(a.coeff + at + (size_t)ax * axs, c[ax], a.al16 != 0);
                if (a.do_lim) {
                    const double h = T * inv_Kl;
                    for (int s = 0; s <= a.K_lim; ++s) {
                        const double tau = (double)s * inv_Kl;
                        const double om = (s == 0 || s == a.K_lim) ? 0.5 : 1.0;
                        flight_limit_sample<NC>(c, tau * T, tau, om, h * om, a, phi_l, dT_l, vv_max, aa_max, gc);
                    }
                }
                if (a.do_clr) {
                    const double h = T * inv_Kc;
                    for (int s = 0; s <= a.K_clr; ++s) {
                        const double tau = (double)s * inv_Kc;
                        const double om = (s == 0 || s == a.K_clr) ? 0.5 : 1.0;
                        if (!flight_clearance_sample<NC>(c, tau * T, tau, om, h * om, a, phi_c, dT_c, neg_min, gc)) ++n_out;
                    }
                }
            }
            const double hl = T * inv_Kl, hc = T * inv_Kc;
            Phi_l = fma(hl, phi_l, Phi_l);
            Phi_c = fma(hc, phi_c, Phi_c);
            if (a.grad_times) a.grad_times[s0 + i] = fma(hl, dT_l, phi_l * inv_Kl) + fma(hc, dT_c, phi_c * inv_Kc);
            if (a.grad_coeff)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, gc[ax], 1.0, a.al16 != 0);
        }
        Phi_l = topt_group_sum(Phi_l);
        Phi_c = topt_group_sum(Phi_c);
        vv_max = topt_group_max(vv_max);
        aa_max = topt_group_max(aa_max);
        neg_min = topt_group_max(neg_min);
#pragma unroll
        for (int dl = 1; dl < LPT; dl <<= 1) n_out += __shfl_xor(n_out, dl, 64);
        if (live && sub == 0) {
            if (a.penalty) a.penalty[b] = Phi_l + Phi_c;
            if (a.peak) {
                a.peak[2 * (size_t)b] = sqrt(vv_max) / a.v_max;
                a.peak[2 * (size_t)b + 1] = sqrt(aa_max) / a.a_max;
            }
            if (a.min_dist) a.min_dist[b] = neg_min == -INFINITY ? a.map.max_dist : -neg_min;
            if (a.outside) a.outside[b] = n_out;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Joint optimiser: minimise f(p, T) = smooth_weight J + time_weight sum_i T_i + Phi(c*(p, T), T) over the interior waypoints inside the box
// |p - anchor| <= max_move and the durations inside [t_min, t_max], per trajectory, by projected gradient descent with Armijo backtracking
// along the projection arc, in p and in u_i = log T_i.
//   g^p_k = smooth_weight dJ/dp_k (wpopt_knot_grad) + through_p_k          g^T_i = -smooth_weight H_i (topt_segment_H) + time_weight
//                                                                                  + explicit_T_i + through_T_i
//   (through_*: ONE backward pass of the penalty's coefficient gradient, explicit_T: the penalty's own dPhi/dT_i at fixed coefficients)
//   d^p_k = g^p_k / s_k, s_k = T_{k-1}^-(2r-1) + T_k^-(2r-1) at the best durations, zero where the box blocks it; d^u_i = T_i g^T_i, zero
//   where a bound blocks it.  The blocks have different units: each has a scale fixed at INIT, sigma_p = step_move / max |d^p|,
//   sigma_u = step_log / max |d^u| (0 when the maximum is 0 or not finite); a positive diagonal scaling keeps -(sigma_p d^p, sigma_u d^u) a
//   descent direction.  alpha starts at 1 (0 when both scales are 0: the trajectory proposes its own point and accepts nothing).
//   trial: p_t = clamp(p - alpha sigma_p d^p), T_t = clamp(T exp(-alpha sigma_u d^u))
// The host enqueues clamp, solve, penalty, backward, step<INIT>, then max_iters x { solve at the trial point, penalty, backward, step<ITER> }.
//   INIT   status SOLVED and f finite -> the trajectory takes part; otherwise its trial point is its own, so every later solve flags it
//          the same way
//   ITER   accepted iff alpha > 0, the trial's status is SOLVED and
//              f_trial <= f_best - armijo [ sum g^p . (p - p_t) + sum d^u_i log(T_i / T_t,i) ]
//          -> waypoints, durations, f_best, both gradients replaced, alpha *= grow; else alpha *= shrink.  Then the next trial from the best point.
// Durations in flight.  s_k reads the duration of the NEIGHBOUR's segment, which another lane owns: the trial durations alternate between
// two arrays (t_eval: what the last solve ran at, read only here; t_next: written here), and the best durations are read from t_eval by a
// group that accepts and from `times` by one that does not -- so no lane reads an element another lane writes in the same launch.
// A trajectory with one segment has no interior knot and takes part through its duration alone.  The end knots are never moved.
// ---------------------------------------------------------------------------------------------------
struct SpacetimeArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    double* waypoints;         // the best (accepted) waypoints: the caller's array
    double* wp_trial;          // [knots][3] trial waypoints (workspace)
    const double* anchor;      // [knots][3] the start: centre of the box
    double* gp_best;           // [knots][3] df/dp at the best point (workspace)
    double* times;             // the best (accepted) durations: the caller's array
    const double* t_eval;      // [total] the durations the last solve ran at (INIT: `times`)
    double* t_next;            // [total] the durations of the next trial
    double* gt_best;           // [total] df/dT at the best point (workspace)
    const double* coeff;       // the last solve
    const int32_t* status;     // its status
    const double* phi;         // [n_traj] flight penalty of that solve
    const double* explicit_t;  // [total] its explicit dPhi/dT_i
    const double* through_p;   // [knots][3] dPhi/dp through the minimiser
    const double* through_t;   // [total] dPhi/dT through the minimiser
    double* fbest;             // [n_traj] workspace
    double* alpha;             // [n_traj] workspace
    double* need;              // [n_traj] workspace: the decrease the pending trial has to reach
    double* sigma;             // [n_traj][2] workspace: the scales of the two blocks
    int32_t* active;           // [n_traj] workspace
    double* objective;         // [n_traj][2]: f at the start, f at the best point
    int32_t* accepted;         // [n_traj] or null
    double ws, wt, t_min, t_max, max_move, step_move, step_log, armijo, shrink, grow;
    int propose;               // 0: last step, no further trial
};

// the duration direction of one segment, zero where a bound blocks the move
__device__ inline double spacetime_dir_u(double gT, double T, double t_min, double t_max) {
    const double d = T * gT;
    return ((T <= t_min && d > 0.0) || (T >= t_max && d < 0.0)) ? 0.0 : d;
}

template <int R, bool INIT>
__global__ __launch_bounds__(64) void spacetime_step_kernel(SpacetimeArgs a) {
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
        if (accept) {
            for (int k = sub; k <= M; k += LPT) {
                double g[3];
                wpopt_knot_grad<R>(c0, axs, M, k, g);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const size_t at = k0 + 3 * (size_t)k + ax;
                    a.gp_best[at] = fma(a.ws, g[ax], a.through_p[at]);
                    if (!INIT && k > 0 && k < M) a.waypoints[at] = a.wp_trial[at];
                }
            }
            for (int i = sub; i < M; i += LPT) {
                const double H = topt_segment_H<R>(c0 + (size_t)i * NC, axs);
                a.gt_best[s0 + i] = fma(-a.ws, H, a.wt) + (a.explicit_t[s0 + i] + a.through_t[s0 + i]);
                if (!INIT) a.times[s0 + i] = a.t_eval[s0 + i];
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

        // the next trial from the best point; its durations are in t_eval after an accepted trial, else in `times` (INIT: the same array)
        const double* __restrict__ Tb = (!INIT && accept) ? a.t_eval : a.times;
        double sig_p, sig_u;
        if (INIT) {
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
                for (int i = sub; i < M; i += LPT) dmax_u = fmax(dmax_u, fabs(spacetime_dir_u(a.gt_best[s0 + i], Tb[s0 + i], a.t_min, a.t_max)));
            }
            dmax_p = topt_group_max(dmax_p);
            dmax_u = topt_group_max(dmax_u);
            sig_p = dmax_p > 0.0 && dmax_p < INFINITY ? a.step_move / dmax_p : 0.0;
            sig_u = dmax_u > 0.0 && dmax_u < INFINITY ? a.step_log / dmax_u : 0.0;
            alpha = (sig_p > 0.0 || sig_u > 0.0) ? 1.0 : 0.0;
        } else {
            sig_p = live ? a.sigma[2 * (size_t)b] : 0.0;
            sig_u = live ? a.sigma[2 * (size_t)b + 1] : 0.0;
        }
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
                        const double g = a.gp_best[at], c = a.anchor[at], lo = c - a.max_move, hi = c + a.max_move;
                        const double d = wpopt_dir(g, s, p, lo, hi);
                        pt = fmin(fmax(p - alpha * sig_p * d, lo), hi);
                        need = fma(g, p - pt, need);
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
            a.alpha[b] = alpha;
            a.need[b] = a.armijo * need;
            if (INIT) {
                a.sigma[2 * (size_t)b] = sig_p;
                a.sigma[2 * (size_t)b + 1] = sig_u;
            }
        }
    });
}

}  // namespace uavqp
