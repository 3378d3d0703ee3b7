// qp_limits.h -- the velocity / acceleration limit penalty of solved trajectories, its two partial gradients, and the steps of the
// limit-aware duration optimiser (uavqp_limit_penalty_device / uavqp_time_optimize_limits_device, include/uavqp.h).
//
// Penalty.  Per trajectory, K = samples_per_seg, tau_s = s / K, trapezoid weights om_0 = om_K = 1/2, om_s = 1 otherwise:
//     Phi = sum_i (T_i / K) sum_{s=0..K} om_s [ w_v pos(|v_i(tau_s T_i)|^2 / v_max^2 - 1)^3 + w_a pos(|a_i(tau_s T_i)|^2 / a_max^2 - 1)^3 ]
// pos(x) = max(0, x), |.| the 3-axis norm of the segment's own polynomial at segment-local time.  With pv, pa the two pos() terms,
// c_v = 6 w_v pv^2 / v_max^2 and c_a = 6 w_a pa^2 / a_max^2 (the derivative of the cube times that of the squared norm):
//     dPhi/dc_{axis,k}  = (T_i / K) sum_s om_s [ c_v v_axis k t^(k-1) + c_a a_axis k (k-1) t^(k-2) ]        (durations fixed)
//     dPhi/dT_i         = Phi_i / T_i + (T_i / K) sum_s om_s tau_s [ c_v v.a + c_a a.j ]                      (coefficients fixed)
// The total gradient in the durations adds the part through c*(T): uavqp_solve_backward_device with g = dPhi/dc.
//
// Lanes.  The lane groups of qp_poly.h: eight lanes per trajectory, sub-lane j owns segments j, j + 8, ..., sums by the xor butterfly, whole
// waves take part.  A lane loads the 3 * 2r coefficients of its segment once, evaluates v, a, j of the three axes at the K + 1 points by
// Horner, keeps the 3 * 2r partial sums of dPhi/dc in registers and stores them once per segment: every output element is written exactly
// once (zeros included), and the order of the additions is fixed by the sample and segment indices alone.
// Memory.  A lane reads and writes 2r consecutive doubles per axis, the eight lanes of a group 8 * 2r consecutive ones ([axis][segment][2r]);
// with 16-byte aligned arrays (al16) the accesses are 16-byte vectors, so a group's store instruction covers whole 64-byte lines after
// 2r / 2 instructions.  Registers (gfx950): no scratch at r = 3 or r = 4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_time_opt.h"

namespace uavqp {

struct LimitArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    double* penalty;          // [n_traj] or null
    double* grad_coeff;       // layout of coeff, or null
    double* grad_times;       // [sum M] or null
    double* peak;             // [n_traj][2] or null
    int K;                    // samples per segment
    int al16;                 // coeff and grad_coeff are 16-byte aligned
    double v_max, a_max, inv_v2, inv_a2, wv, wa;
};

template <int NC>
__device__ inline void lim_load(const double* __restrict__ p, double (&x)[NC], bool al16) {
    if (al16) {
        const double2* __restrict__ q = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int k = 0; k < NC / 2; ++k) {
            const double2 w = q[k];
            x[2 * k] = w.x;
            x[2 * k + 1] = w.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) x[k] = p[k];
    }
}
template <int NC>
__device__ inline void lim_store(double* __restrict__ p, const double (&x)[NC], double scale, bool al16) {
    if (al16) {
        double2* __restrict__ q = reinterpret_cast<double2*>(p);
#pragma unroll
        for (int k = 0; k < NC / 2; ++k) q[k] = make_double2(scale * x[2 * k], scale * x[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) p[k] = scale * x[k];
    }
}

template <int R>
__global__ __launch_bounds__(64) void limit_penalty_kernel(LimitArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    // (the loop of topt_for_each_group written out, as in clearance_penalty_kernel: through the lambda the compiler shapes the sample loop
    // differently -- docs/measurement_log.md)
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;  // whole waves take part in the shuffles
    const double inv_K = 1.0 / (double)a.K;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = live && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        double Phi = 0.0, vv_max = 0.0, aa_max = 0.0;
        for (int i = sub; i < M; i += LPT) {
            const size_t at = (size_t)3 * NC * s0 + (size_t)i * NC;
            double gc[3][NC];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int k = 0; k < NC; ++k) gc[ax][k] = 0.0;
            double phi = 0.0, dT = 0.0, T = 0.0;
            if (solved) {
                T = a.times[s0 + i];
                double c[3][NC];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_load<NC>(a.coeff + at + (size_t)ax * axs, c[ax], a.al16 != 0);
                for (int s = 0; s <= a.K; ++s) {
                    const double tau = (double)s * inv_K, t = tau * T;
                    const double om = (s == 0 || s == a.K) ? 0.5 : 1.0;
                    double v[3], ac[3], jk[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double pv = topt_falling(NC - 1, 1) * c[ax][NC - 1], pa = topt_falling(NC - 1, 2) * c[ax][NC - 1],
                               pj = topt_falling(NC - 1, 3) * c[ax][NC - 1];
#pragma unroll
                        for (int k = NC - 2; k >= 1; --k) {
                            pv = fma(pv, t, topt_falling(k, 1) * c[ax][k]);
                            if (k >= 2) pa = fma(pa, t, topt_falling(k, 2) * c[ax][k]);
                            if (k >= 3) pj = fma(pj, t, topt_falling(k, 3) * c[ax][k]);
                        }
                        v[ax] = pv; ac[ax] = pa; jk[ax] = pj;
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
                            const double gv = om * cv * v[ax], ga = om * ca * ac[ax];
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
            }
            const double h = T * inv_K;
            Phi = fma(h, phi, Phi);
            if (a.grad_times) a.grad_times[s0 + i] = fma(h, dT, phi * inv_K);
            if (a.grad_coeff)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, gc[ax], h, a.al16 != 0);
        }
        Phi = topt_group_sum(Phi);
        vv_max = topt_group_max(vv_max);
        aa_max = topt_group_max(aa_max);
        if (live && sub == 0) {
            if (a.penalty) a.penalty[b] = Phi;
            if (a.peak) {
                a.peak[2 * (size_t)b] = sqrt(vv_max) / a.v_max;
                a.peak[2 * (size_t)b + 1] = sqrt(aa_max) / a.a_max;
            }
        }
    }
}

}  // namespace uavqp
