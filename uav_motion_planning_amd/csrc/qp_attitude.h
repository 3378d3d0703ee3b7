// qp_attitude.h -- the attitude penalty of solved trajectories (specific thrust, tilt, body rate of the multirotor that flies them) and its
// two partial gradients (uavqp_attitude_penalty_device, include/uavqp.h; the accumulating variant serves uavqp_attitude_optimize_device).
//
// Penalty.  Per sample at segment-local time t: a, j, s the acceleration, jerk and snap of the three axes, z = a + gravity e_z the specific
// thrust vector, f2 = |z|^2, zj = z.j, jj = |j|^2, x = z x j.  With pos(u) = max(0, u) and kappa = tan^2(tilt_max):
//     u_hi   = f2 / f_max^2 - 1                                  u_lo = 1 - f2 / f_min^2   (absent when f_min = 0)
//     u_tilt = (z_x^2 + z_y^2 - kappa z_z |z_z|) / gravity^2     u_rate = (|x|^2 - rate_max^2 f2^2) / (rate_max^2 gravity^4)
//     phi    = w_thrust (pos(u_hi)^3 + pos(u_lo)^3) + w_tilt pos(u_tilt)^3 + w_rate pos(u_rate)^3
//     Phi    = sum_i (T_i / K) sum_{s=0..K} om_s phi(tau_s T_i)            (the weights and sample points of qp_limits.h)
// Nothing divides by |z|: free fall (z = 0) is an ordinary input, costs w_thrust per unit of weight and has zero gradient.  |x|^2 is taken
// from the cross product itself, not from f2 jj - zj^2: it cannot come out negative and loses nothing when z and j are nearly parallel.
// Gradients, with A = 6 w_thrust (pos(u_hi)^2 / f_max^2 - pos(u_lo)^2 / f_min^2) + C (jj - 2 rate_max^2 f2),
// B = 6 w_tilt pos(u_tilt)^2 / gravity^2, C = 6 w_rate pos(u_rate)^2 / (rate_max^2 gravity^4)  (d|x|^2/dz = 2 (jj z - zj j), d|x|^2/dj = 2 (f2 j - zj z)):
//     G_a = A z + B (z_x, z_y, -kappa |z_z|) - C zj j          G_j = C (f2 j - zj z)
//     dPhi/dc_{axis,k} = (T_i / K) sum_s om_s [ G_a[axis] k (k-1) t^(k-2) + G_j[axis] k (k-1) (k-2) t^(k-3) ]     (durations fixed)
//     dPhi/dT_i        = Phi_i / T_i + (T_i / K) sum_s om_s tau_s [ G_a . j + G_j . s ]                             (coefficients fixed)
//
// Lanes, memory: those of limit_penalty_kernel (qp_limits.h) -- eight lanes per trajectory, sub-lane j owns segments j, j + 8, ..., a lane
// loads the 3 * 2r coefficients of its segment once (16-byte vectors when aligned) and keeps them as the 2r - 2 coefficients of the
// acceleration polynomial; a, j, s at a sample are Horner on it three times over (synthetic division: no products with constants that the
// compiler would hoist out of the sample loop into 90 registers); the 3 * (2r - 2) partial sums that can be non-zero stay in registers and
// are stored once per segment; sums across the group by the xor butterfly.  Every output
// element is written exactly once (zeros included) and the order of the additions is fixed by the sample and segment indices alone.
// The peaks (atan2, a square root and a division per sample) are taken only when the peak output is asked for.
// ACC = true ADDS to penalty, grad_coeff and grad_times instead (what the arrays hold is the flight penalty's): a segment without an
// active sample, and a trajectory that is not solved, then touch nothing.  Registers (gfx950): no scratch at r = 3
// or r = 4, in either variant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_limits.h"

namespace uavqp {

struct AttitudeArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    double* penalty;          // [n_traj] or null
    double* grad_coeff;       // layout of coeff, or null
    double* grad_times;       // [sum M] or null
    double* peak;             // [n_traj][4] or null
    int K;                    // samples per segment
    int al16;                 // coeff and grad_coeff are 16-byte aligned
    double gravity, inv_g2;   // 1 / gravity^2
    double inv_fmax2;         // 1 / f_max^2
    double lo_one, inv_fmin2; // u_lo = lo_one - f2 inv_fmin2: (1, 1 / f_min^2), or (0, 0) when f_min = 0
    double kappa;             // tan^2(tilt_max)
    double rate2, inv_rg4;    // rate_max^2, 1 / (rate_max^2 gravity^4)
    double w_thrust, w_tilt, w_rate;
};

__device__ inline double topt_group_min(double x) {
#pragma unroll
    for (int d = 1; d < TOPT_LPT; d <<= 1) x = fmin(x, __shfl_xor(x, d, 64));
    return x;
}

template <int R, bool ACC = false>
__global__ __launch_bounds__(64) void attitude_penalty_kernel(AttitudeArgs a) {
    constexpr int NC = 2 * R, NA = NC - 2, LPT = TOPT_LPT;
    // (the loop of topt_for_each_group written out, as in limit_penalty_kernel)
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;  // whole waves take part in the shuffles
    const double inv_K = 1.0 / (double)a.K;
    const bool want_peak = a.peak != nullptr;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = live && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        double Phi = 0.0, f2_max = 0.0, f2_min = INFINITY, tilt_max = 0.0, rate_max = 0.0;
        for (int i = sub; i < M; i += LPT) {
            if (ACC && !solved) break;
            const size_t at = (size_t)3 * NC * s0 + (size_t)i * NC;
            double ga_[3][NA];   // the sums in the coefficients of the ACCELERATION polynomial: dPhi/dc_k = k (k-1) ga_[k-2]
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int m = 0; m < NA; ++m) ga_[ax][m] = 0.0;
            double phi = 0.0, dT = 0.0, T = 0.0;
            bool any = false;
            if (solved) {
                T = a.times[s0 + i];
                // the acceleration polynomial A(t) = sum_m (m+2)(m+1) c_{m+2} t^m, scaled once: the sample loop holds no constant products
                double ca[3][NA];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    double c[NC];
                    lim_load<NC>(a.coeff + at + (size_t)ax * axs, c, a.al16 != 0);
#pragma unroll
                    for (int m = 0; m < NA; ++m) ca[ax][m] = topt_falling(m + 2, 2) * c[m + 2];
                }
                for (int s = 0; s <= a.K; ++s) {
                    const double tau = (double)s * inv_K, t = tau * T;
                    const double om = (s == 0 || s == a.K) ? 0.5 : 1.0;
                    double z[3], j[3], sn[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        // Horner three times over (synthetic division): w[0] = A(t), w[1] = A'(t), w[2] = A''(t) / 2
                        double w[NA];
#pragma unroll
                        for (int m = 0; m < NA; ++m) w[m] = ca[ax][m];
#pragma unroll
                        for (int d = 0; d < 3; ++d)
#pragma unroll
                            for (int m = NA - 2; m >= d; --m) w[m] = fma(w[m + 1], t, w[m]);
                        z[ax] = w[0]; j[ax] = w[1]; sn[ax] = 2.0 * w[2];
                    }
                    z[2] += a.gravity;
                    const double hh = fma(z[0], z[0], z[1] * z[1]);
                    const double f2 = fma(z[2], z[2], hh);
                    const double jj = fma(j[0], j[0], fma(j[1], j[1], j[2] * j[2]));
                    const double zj = fma(z[0], j[0], fma(z[1], j[1], z[2] * j[2]));
                    const double x0 = z[1] * j[2] - z[2] * j[1], x1 = z[2] * j[0] - z[0] * j[2], x2 = z[0] * j[1] - z[1] * j[0];
                    const double xx = fma(x0, x0, fma(x1, x1, x2 * x2));
                    const double az = fabs(z[2]);
                    if (want_peak) {
                        f2_max = fmax(f2_max, f2);
                        f2_min = fmin(f2_min, f2);
                        tilt_max = fmax(tilt_max, atan2(sqrt(hh), z[2]));
                        if (f2 > 0.0) rate_max = fmax(rate_max, sqrt(xx) / f2);
                    }
                    const double ph = fmax(0.0, fma(f2, a.inv_fmax2, -1.0));
                    const double pl = fmax(0.0, fma(-f2, a.inv_fmin2, a.lo_one));
                    const double pt = fmax(0.0, (hh - a.kappa * z[2] * az) * a.inv_g2);
                    const double pr = fmax(0.0, fma(-a.rate2 * f2, f2, xx) * a.inv_rg4);
                    phi = fma(om, fma(a.w_thrust, fma(ph * ph, ph, pl * pl * pl), fma(a.w_tilt * pt, pt * pt, a.w_rate * pr * (pr * pr))), phi);
                    const double Ct = 6.0 * a.w_thrust * (ph * ph * a.inv_fmax2 - pl * pl * a.inv_fmin2);
                    const double B = 6.0 * a.w_tilt * (pt * pt) * a.inv_g2;
                    const double C = 6.0 * a.w_rate * (pr * pr) * a.inv_rg4;
                    if (Ct != 0.0 || B != 0.0 || C != 0.0) {
                        any = true;
                        const double A = fma(C, fma(-2.0 * a.rate2, f2, jj), Ct);
                        const double Czj = C * zj;
                        double Ga[3], Gj[3];
                        Ga[0] = fma(A + B, z[0], -Czj * j[0]);
                        Ga[1] = fma(A + B, z[1], -Czj * j[1]);
                        Ga[2] = fma(A, z[2], fma(-B * a.kappa, az, -Czj * j[2]));
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) Gj[ax] = C * fma(f2, j[ax], -zj * z[ax]);
                        const double gaj = fma(Ga[0], j[0], fma(Ga[1], j[1], Ga[2] * j[2]));
                        const double gjs = fma(Gj[0], sn[0], fma(Gj[1], sn[1], Gj[2] * sn[2]));
                        dT = fma(om * tau, gaj + gjs, dT);
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const double ga = om * Ga[ax], gj = om * Gj[ax];
                            double p1 = 1.0, p0 = t;   // t^(m-1), t^m
                            ga_[ax][0] += ga;
#pragma unroll
                            for (int m = 1; m < NA; ++m) {
                                ga_[ax][m] = fma(ga, p0, fma(gj * (double)m, p1, ga_[ax][m]));
                                p1 = p0;
                                p0 *= t;
                            }
                        }
                    }
                }
            }
            const double h = T * inv_K;
            Phi = fma(h, phi, Phi);
            if (ACC) {
                if (!any && phi == 0.0) continue;   // (nothing to add)
                if (a.grad_times) a.grad_times[s0 + i] += fma(h, dT, phi * inv_K);
                if (a.grad_coeff && any)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double old[NC];
                        lim_load<NC>(a.grad_coeff + at + (size_t)ax * axs, old, a.al16 != 0);
#pragma unroll
                        for (int k = 2; k < NC; ++k) old[k] = fma(h * topt_falling(k, 2), ga_[ax][k - 2], old[k]);
                        lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, old, 1.0, a.al16 != 0);
                    }
            } else {
                if (a.grad_times) a.grad_times[s0 + i] = fma(h, dT, phi * inv_K);
                if (a.grad_coeff)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double gc[NC];
                        gc[0] = gc[1] = 0.0;
#pragma unroll
                        for (int k = 2; k < NC; ++k) gc[k] = topt_falling(k, 2) * ga_[ax][k - 2];
                        lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, gc, h, a.al16 != 0);
                    }
            }
        }
        Phi = topt_group_sum(Phi);
        if (want_peak) {
            f2_max = topt_group_max(f2_max);
            f2_min = topt_group_min(f2_min);
            tilt_max = topt_group_max(tilt_max);
            rate_max = topt_group_max(rate_max);
        }
        if (live && sub == 0) {
            if (a.penalty) {
                if (ACC) {
                    if (solved) a.penalty[b] += Phi;
                } else {
                    a.penalty[b] = Phi;
                }
            }
            if (want_peak) {
                double* pk = a.peak + 4 * (size_t)b;
                pk[0] = sqrt(f2_max);
                pk[1] = sqrt(f2_min);
                pk[2] = tilt_max;
                pk[3] = rate_max;
            }
        }
    }
}

}  // namespace uavqp
