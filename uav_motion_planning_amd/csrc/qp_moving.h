// qp_moving.h -- the penalty of solved trajectories against MOVING obstacles (tracks in the library's own trajectory format that are not
// this batch's to move) with its gradients in the coefficients, the durations and the departure (uavqp_moving_penalty_device,
// include/uavqp.h: the definition, the formulas and the rules are there; the accumulating variant serves uavqp_moving_optimize_device).
//
// Per sample s of segment m of trajectory b (departure S): local time t = tau_s T_m, clock time t_abs = fma(tau_s, T_m, K_m) with the knot
// clock K_0 = S, K_{m+1} = fl(K_m + T_m).  Obstacle o of the trajectory's set is located at u = t_abs - start_o by the rule of
// swarm_penalty_kernel (qp_swarm.h: waiting, the segment rule of qp_poly.h, arrived with the cap on the last segment); delta = q(t) - o,
// D_o = d_safe + radius_o, rho2 = (dx^2 + dy^2 + dz^2 / downwash^2) / D_o^2, x = max(0, 1 - rho2):
//     phi = weight sum_o x^3        e_o = -6 weight x^2 / D_o^2 diag(1, 1, 1 / downwash^2) delta        G = sum_o e_o        Gt = -sum_o e_o . o'
//     dPhi/dc_{axis,m,n} = (T_m / K) sum_s om_s G[axis] t^n                                                             (durations fixed)
//     dPhi/dT_l = Phi_l / T_l + (T_l / K) sum_s om_s tau_s (G . v + Gt) + sum_{m > l} (T_m / K) Q_m,   Q_m = sum_s om_s Gt  (coefficients fixed)
//     dPhi/dS   = sum_m (T_m / K) Q_m
//
// Lanes, memory: those of limit_penalty_kernel / attitude_penalty_kernel -- eight lanes per trajectory, sub-lane j owns segments j, j + 8,
// ..., a lane loads the 3 * 2r coefficients of its segment once (16-byte vectors when aligned), keeps the 3 * 2r partial sums in registers
// and stores them once per segment.  New here:
//   * the knot clock: a lane sums the durations before its segment in index order, from S -- every lane the same additions in the same
//     order, so all agree on the doubles (the durations of a trajectory are a few cache lines the eight lanes read together);
//   * the suffix sum of W_m = (T_m / K) Q_m: the rounds of eight segments are walked from the LAST to the first; inside a round the eight
//     lanes' W are read by eight shuffles in falling segment index and added to the total carried in from the later rounds, a lane
//     keeping what the sum held when its own segment came up.  So sum_{m > l} W_m is ((W_{M-1} + W_{M-2}) + ...) + W_{l+1}, an order
//     fixed by the segment index alone, and what is carried out of round 0 is dPhi/dS.  grad_times is stored once per segment by its lane.
//     The shuffles stay inside a lane group and every lane of a group runs the same number of rounds: groups of different length in one
//     wave do not meet in them.
// Obstacle data (durations, 2r coefficients per axis of the located segment, start, radius) comes through the ordinary load path: the
// lanes of a group, and all groups that avoid the same set, read the same few lines.
// Every output element is written exactly once (zeros included); the order of the additions is fixed by sample, obstacle and segment
// indices alone.  min_gap / nearest: a lexicographic (gap, index) minimum, exact, so its order does not matter.
// ACC = true ADDS to penalty, grad_coeff and grad_times instead (what the arrays hold is the flight penalty's): a segment without an
// active sample and without a later active one, and a trajectory without an obstacle, touch nothing.
// Registers (gfx950): no scratch at r = 3 or r = 4, in either variant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_limits.h"

namespace uavqp {

struct MovingArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;        // null: every trajectory counts as solved
    // the obstacle batch and who avoids what
    int n_obs, o_uniform, n_sets;
    const int32_t* o_seg_offsets;
    const double* o_times;
    const double* o_coeff;
    const double* o_start;        // null: all zero
    const double* o_radius;       // null: all zero
    const int32_t* set_offsets;   // null: one set, the whole obstacle batch
    const int32_t* traj_set;      // null: every trajectory avoids set 0
    const double* traj_start;     // null: all zero
    double* penalty;              // [n_traj] or null
    double* grad_coeff;           // layout of coeff, or null
    double* grad_times;           // [sum M] or null
    double* grad_start;           // [n_traj] or null
    double* min_gap;              // [n_traj] or null
    int32_t* nearest;             // [n_traj] or null
    int K;                        // samples per segment
    int al16;                     // coeff and grad_coeff are 16-byte aligned
    double d_safe;
    double inv_dw2;               // 1 / downwash^2
    double weight;
};

template <int R, bool ACC = false>
__global__ __launch_bounds__(64) void moving_penalty_kernel(MovingArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    // (the loop of topt_for_each_group written out, as in limit_penalty_kernel)
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;  // whole waves take part in the shuffles
    const double inv_K = 1.0 / (double)a.K;
    const bool want_gap = a.min_gap != nullptr || a.nearest != nullptr;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = live && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        // the obstacles of the trajectory's set: [o0, o1)
        int o0 = 0, o1 = 0;
        if (solved) {
            const int k = a.traj_set ? a.traj_set[b] : 0;
            if (k >= 0 && k < a.n_sets) {
                o0 = a.set_offsets ? a.set_offsets[k] : 0;
                o1 = a.set_offsets ? a.set_offsets[k + 1] : a.n_obs;
            }
        }
        const bool act = solved && o1 > o0;   // (the same in the eight lanes of a group)
        const double S = (act && a.traj_start) ? a.traj_start[b] : 0.0;
        double Phi = 0.0, carry = 0.0, gap_min = INFINITY;
        int near = -1;
        const int rounds = M > 0 ? (M + LPT - 1) / LPT : 0;
        for (int rd = rounds - 1; rd >= 0; --rd) {
            if (ACC && !act) break;
            const int i = rd * LPT + sub;
            const bool own = i < M;
            const size_t at = (size_t)3 * NC * s0 + (size_t)(own ? i : 0) * NC;
            double gc[3][NC];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int n = 0; n < NC; ++n) gc[ax][n] = 0.0;
            double phi = 0.0, dT = 0.0, Q = 0.0, T = 0.0;
            bool any = false;
            if (own && act) {
                T = a.times[s0 + i];
                double Kc = S;   // the knot clock at the head of segment i
                for (int m = 0; m < i; ++m) Kc += a.times[s0 + m];
                double c[3][NC];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_load<NC>(a.coeff + at + (size_t)ax * axs, c[ax], a.al16 != 0);
                for (int s = 0; s <= a.K; ++s) {
                    const double tau = (double)s * inv_K, t = tau * T, t_abs = fma(tau, T, Kc);
                    const double om = (s == 0 || s == a.K) ? 0.5 : 1.0;
                    double q[3], v[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        // Horner twice over (synthetic division): w[0] = p(t), w[1] = p'(t)
                        double w[NC];
#pragma unroll
                        for (int n = 0; n < NC; ++n) w[n] = c[ax][n];
#pragma unroll
                        for (int d = 0; d < 2; ++d)
#pragma unroll
                            for (int n = NC - 2; n >= d; --n) w[n] = fma(w[n + 1], t, w[n]);
                        q[ax] = w[0]; v[ax] = w[1];
                    }
                    double G0 = 0.0, G1 = 0.0, G2 = 0.0, Gt = 0.0, x3 = 0.0;
                    for (int o = o0; o < o1; ++o) {
                        const auto [os0, Mo] = poly_span(a.o_uniform, a.o_seg_offsets, o);
                        if (Mo < 1) continue;   // (a track without a segment is nowhere)
                        const double* To = a.o_times + os0;
                        const double u = t_abs - (a.o_start ? a.o_start[o] : 0.0);
                        int idx = 0;
                        double tl = 0.0;
                        bool held = true;   // waiting or arrived: the position does not move with the clock
                        if (!(u < 0.0)) {
                            const PolySeg ps = poly_segment(To, Mo, u);
                            const double T_last = To[Mo - 1];
                            const bool arrived = ps.past || (ps.idx == Mo - 1 && ps.t >= T_last);
                            idx = arrived ? Mo - 1 : ps.idx;
                            tl = arrived ? T_last : ps.t;
                            held = arrived;
                        }
                        const double* oc = a.o_coeff + (size_t)3 * NC * os0 + (size_t)idx * NC;
                        double d[3], ov[3];
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const double* ca = oc + (size_t)ax * NC * Mo;
                            double w[NC];
#pragma unroll
                            for (int n = 0; n < NC; ++n) w[n] = ca[n];
#pragma unroll
                            for (int dd = 0; dd < 2; ++dd)
#pragma unroll
                                for (int n = NC - 2; n >= dd; --n) w[n] = fma(w[n + 1], tl, w[n]);
                            d[ax] = q[ax] - w[0];
                            ov[ax] = held ? 0.0 : w[1];
                        }
                        const double rad = a.o_radius ? a.o_radius[o] : 0.0;
                        const double dd2 = fma(d[0], d[0], fma(d[1], d[1], d[2] * d[2] * a.inv_dw2));
                        if (want_gap) {
                            const double gap = sqrt(dd2) - rad;
                            if (gap < gap_min || (gap == gap_min && o < near)) {
                                gap_min = gap;
                                near = o;
                            }
                        }
                        const double D = a.d_safe + rad, inv_D2 = 1.0 / (D * D);
                        const double x = fmax(0.0, fma(-dd2, inv_D2, 1.0));
                        if (x > 0.0) {
                            const double f = -6.0 * a.weight * inv_D2 * (x * x);
                            const double e0 = f * d[0], e1 = f * d[1], e2 = f * a.inv_dw2 * d[2];
                            G0 += e0; G1 += e1; G2 += e2;
                            Gt -= fma(e0, ov[0], fma(e1, ov[1], e2 * ov[2]));
                            x3 = fma(x, x * x, x3);
                        }
                    }
                    phi = fma(om * a.weight, x3, phi);
                    if (G0 != 0.0 || G1 != 0.0 || G2 != 0.0 || Gt != 0.0) {
                        any = true;
                        const double Gv = fma(G0, v[0], fma(G1, v[1], G2 * v[2]));
                        dT = fma(om * tau, Gv + Gt, dT);
                        Q = fma(om, Gt, Q);
                        const double Gw[3] = {om * G0, om * G1, om * G2};
                        double p = 1.0;
#pragma unroll
                        for (int n = 0; n < NC; ++n) {
#pragma unroll
                            for (int ax = 0; ax < 3; ++ax) gc[ax][n] = fma(Gw[ax], p, gc[ax][n]);
                            p *= t;
                        }
                    }
                }
            }
            const double h = T * inv_K;
            const double W = h * Q;
            // sum_{m > i} W_m: the carried total of the later rounds, then this round's W in falling segment index
            double tail = 0.0, run = carry;
#pragma unroll
            for (int k = LPT - 1; k >= 0; --k) {
                if (k == sub) tail = run;
                run += __shfl(W, k, LPT);
            }
            carry = run;
            if (!own) continue;
            Phi = fma(h, phi, Phi);
            const double gt = fma(h, dT, phi * inv_K) + tail;
            if (ACC) {
                if (a.grad_times && gt != 0.0) a.grad_times[s0 + i] += gt;
                if (a.grad_coeff && any)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double old[NC];
                        lim_load<NC>(a.grad_coeff + at + (size_t)ax * axs, old, a.al16 != 0);
#pragma unroll
                        for (int n = 0; n < NC; ++n) old[n] = fma(h, gc[ax][n], old[n]);
                        lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, old, 1.0, a.al16 != 0);
                    }
            } else {
                if (a.grad_times) a.grad_times[s0 + i] = gt;
                if (a.grad_coeff)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, gc[ax], h, a.al16 != 0);
            }
        }
        Phi = topt_group_sum(Phi);
        if (want_gap) {
            // the lexicographic minimum of (gap, obstacle) over the group
#pragma unroll
            for (int d = 1; d < LPT; d <<= 1) {
                const double og = __shfl_xor(gap_min, d, 64);
                const int on = __shfl_xor(near, d, 64);
                if (on >= 0 && (near < 0 || og < gap_min || (og == gap_min && on < near))) {
                    gap_min = og;
                    near = on;
                }
            }
        }
        if (live && sub == 0) {
            if (ACC) {
                if (a.penalty && act && Phi != 0.0) a.penalty[b] += Phi;
            } else {
                if (a.penalty) a.penalty[b] = Phi;
                if (a.grad_start) a.grad_start[b] = carry;
                if (a.min_gap) a.min_gap[b] = near >= 0 ? gap_min : INFINITY;
                if (a.nearest) a.nearest[b] = near;
            }
        }
    }
}

}  // namespace uavqp
