// qp_adjoint.h -- backward pass of the equality-constrained batched solve (uavqp_solve_backward_device, include/uavqp.h): for a given
// g = dPhi/dc in the layout of the coefficients, the vector-Jacobian products dPhi/dT, dPhi/dwaypoints, dPhi/dbc THROUGH the minimiser.
//
// Variables.  Per axis the minimiser is c_i = B(T_i) [x_i; x_{i+1}] (segment_coeffs) with knot states x_k = (p_k, y_k); the interior y_k solve
//     F_k(y; p, bc, T) = A01(k-1)' y_{k-1} + (A11(k-1) + A00(k)) y_k + A01(k) y_{k+1} - gv(k) dp_k + gw(k-1) dp_{k-1} = 0,   k = 1..M-1
// (SegBlocks of segment k-1 / k, dp_i = p_{i+1} - p_i, y_0 / y_M from bc): the forward's SPD block-tridiagonal system H y = z.
//   1. pull-back at fixed T: e_i = B(T_i)' g_i, split into a start and an end knot state and summed per knot: q_k = (q_k^p, q_k^y);
//      on the way the explicit term  tex_i = g_i' (dB/dT_i) [x_i; x_{i+1}]  (every T-dependent entry is a power of T_i).
//   2. H lambda = q^y on the interior knots: block-Thomas sweep, one factorisation, three right-hand sides (H is symmetric: the adjoint
//      system IS the forward's matrix).
//   3. local assembly, with G_i = lambda_i' F^start_i + lambda_{i+1}' F^end_i the part of lambda' F that segment i contributes:
//        grad T_i     = tex_i - dG_i/dT_i                        (entries T^e: derivative = entry * e / T)
//        grad p_k     = q_k^p + w_{k-1} - w_k,   w_i = lambda_i' gv(i) - lambda_{i+1}' gw(i)      (w_{-1} = w_M = 0)
//        grad y_0     = q_0^y - A01(0) lambda_1,     grad y_M = q_M^y - A01(M-1)' lambda_{M-1}     (lambda_0 = lambda_M = 0)
// The knot derivatives are read from the coefficients the caller passes in (y_k[d] = d! c_d of segment k), positions from the waypoints.
//
// Lanes.  One lane per trajectory carries the three axes (they share the factorisation).  Sweep state per segment -- tex_i, and for the knot
// in front of it E = S^-1 A01, h = S^-1 z (three columns) and q^p -- lives in an HBM workspace ws[wave][segment][field][lane] (every access a
// coalesced 512-byte row of the wave), written by the forward sweep over the segments and re-read by the backward one.  Every output element
// is written once, by the lane of its trajectory, and every sum has a fixed order: the same bytes run to run and for any grid.
// A trajectory that is invalid (M < 1, M > max_segments, a duration that is not positive and finite) or whose passed status is not
// UAVQP_SOLVED gets zeros in all three outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/uavqp.h"
#include "qp_device.h"

namespace uavqp {

struct AdjointArgs {
    int n_traj;
    int uniform;       // > 0: uniform segment count
    int max_segments;  // ragged upper bound = records per lane in ws
    const int32_t* seg_offsets;
    const double* waypoints;
    const double* times;
    const double* bc;
    const double* coeff;
    const int32_t* status;      // may be null
    const double* grad_coeff;
    double* grad_times;         // each output may be null
    double* grad_waypoints;
    double* grad_bc;
    double* ws;
};

__device__ __forceinline__ constexpr double adjoint_fact(int k) {
    double f = 1.0;
    for (int j = 2; j <= k; ++j) f *= (double)j;
    return f;
}

template <int R>
struct AdjointRec {
    static constexpr int ND = R - 1;
    static constexpr int TEX = 0, E = 1, H = E + ND * ND, QP = H + 3 * ND, F = QP + 3;   // doubles per (segment, lane)
};

// Pull-back of one segment of one axis.  g: the 2R entries of dPhi/dc of the segment; ip[j] = T^-j, tp[d] = T^d; dp = p1 - p0; ys / ye the
// derivatives 1..R-1 at the two knots.  Out: (sp, sy) / (ep, ey) = dPhi/d(start state) / d(end state) at fixed T, and T * tex.
template <int R>
__device__ __forceinline__ void adjoint_pullback(const double (&g)[2 * R], const double (&ip)[2 * R], const double (&tp)[R], double dp,
                                                 const double (&ys)[R - 1], const double (&ye)[R - 1], double& sp, double (&sy)[R - 1],
                                                 double& ep, double (&ey)[R - 1], double& texT) {
    // c[R + j] = T^-(R+j) sum_d K(j, d) e[d]:  h[d] = dPhi/de[d],  h2[d] = -T * (the part of dPhi/dT through the power T^-(R+j))
    double h[R], h2[R];
#pragma unroll
    for (int d = 0; d < R; ++d) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const double gj = g[R + j] * ip[R + j] * Tab<R>::K(j, d);
            a += gj;
            b += (double)(R + j) * gj;
        }
        h[d] = a;
        h2[d] = b;
    }
    // e[d] = s1[d] - sum_{k >= max(d, 1)} s0[k] / (k - d)!,  s*_d = T^d y_d (s1[0] = dp, s0[0] = 0);  T de[d]/dT: every s_d scales by d
    double s0[R], s1[R];
    s0[0] = 0.0;
    s1[0] = dp;
#pragma unroll
    for (int d = 1; d < R; ++d) {
        s0[d] = tp[d] * ys[d - 1];
        s1[d] = tp[d] * ye[d - 1];
    }
    double t = 0.0;
#pragma unroll
    for (int d = 0; d < R; ++d) {
        double e = s1[d], de = (double)d * s1[d];
#pragma unroll
        for (int k = (d > 1 ? d : 1); k < R; ++k) {
            e -= s0[k] * inv_fact(k - d);
            de -= (double)k * s0[k] * inv_fact(k - d);
        }
        t += h[d] * de - h2[d] * e;
    }
    texT = t;
    ep = h[0];
    sp = g[0] - h[0];
#pragma unroll
    for (int k = 1; k < R; ++k) {
        ey[k - 1] = tp[k] * h[k];
        double a = 0.0;
#pragma unroll
        for (int d = 0; d <= k; ++d) a += h[d] * inv_fact(k - d);
        sy[k - 1] = g[k] * inv_fact(k) - tp[k] * a;
    }
}

template <int R>
__global__ __launch_bounds__(64) void solve_backward_kernel(AdjointArgs a) {
    using Rec = AdjointRec<R>;
    constexpr int ND = R - 1, NC = 2 * R, F = Rec::F;
    const int lane = threadIdx.x;
    const int kmax = a.max_segments > 1 ? a.max_segments : 1;
    double* __restrict__ ws = a.ws + (size_t)blockIdx.x * kmax * F * 64 + lane;
    constexpr size_t wstride = 64;
    const int n_items = gridDim.x * 64;
    const int n_round = (a.n_traj + n_items - 1) / n_items;
    for (int round = 0; round < n_round; ++round) {
        const int b = round * n_items + blockIdx.x * 64 + lane;
        if (b >= a.n_traj) continue;
        int s0, M;
        if (a.uniform > 0) {
            M = a.uniform;
            s0 = b * M;
        } else {
            s0 = a.seg_offsets[b];
            M = a.seg_offsets[b + 1] - s0;
        }
        const double* __restrict__ wp = a.waypoints + 3 * (size_t)(s0 + b);
        const double* __restrict__ T = a.times + s0;
        const double* __restrict__ bc = a.bc + (size_t)b * 2 * ND * 3;
        const double* __restrict__ cf = a.coeff + (size_t)3 * NC * s0;
        const double* __restrict__ gc = a.grad_coeff + (size_t)3 * NC * s0;
        double* __restrict__ gT = a.grad_times ? a.grad_times + s0 : nullptr;
        double* __restrict__ gW = a.grad_waypoints ? a.grad_waypoints + 3 * (size_t)(s0 + b) : nullptr;
        double* __restrict__ gB = a.grad_bc ? a.grad_bc + (size_t)b * 2 * ND * 3 : nullptr;

        bool ok = (M >= 1) && (a.uniform > 0 || M <= a.max_segments);
        if (ok)
            for (int i = 0; i < M; ++i) ok = ok && (T[i] > 0.0) && (T[i] < INFINITY);
        if (ok && a.status) ok = a.status[b] == UAVQP_SOLVED;
        if (!ok) {
            if (gT)
                for (int i = 0; i < M; ++i) gT[i] = 0.0;
            if (gW)
                for (int i = 0; i < 3 * (M + 1); ++i) gW[i] = 0.0;
            if (gB)
                for (int i = 0; i < 2 * ND * 3; ++i) gB[i] = 0.0;
            continue;
        }

        // knot derivatives of knot k, three axes: from the coefficients (k < M) or the end boundary values (k = M)
        auto load_y = [&](int k, double (&y)[ND][3]) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int d = 0; d < ND; ++d)
                    y[d][ax] = k < M ? cf[((size_t)ax * M + k) * NC + d + 1] * adjoint_fact(d + 1) : bc[(ND + d) * 3 + ax];
        };

        // ---------------- forward sweep over the segments: pull-back, knot sums, block elimination ----------------
        double q0p[3], q0y[ND][3];   // q of knot 0
        double qep[3], qey[ND][3];   // end part of the segment behind the current knot (after the loop: q of knot M)
        double Eprev[ND][ND], hprev[ND][3];
        SegBlocks<R> sa;
        double ycur[ND][3], ynext[ND][3], pcur[3], pnext[3];
        load_y(0, ycur);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) pcur[ax] = wp[ax];
        for (int i = 0; i < M; ++i) {
            load_y(i + 1, ynext);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) pnext[ax] = wp[3 * (i + 1) + ax];
            const double Ti = T[i];
            SegBlocks<R> sb;
            double ip[NC], tp[R];
            sb.build(Ti, ip);
            tp[0] = 1.0;
#pragma unroll
            for (int d = 1; d < R; ++d) tp[d] = tp[d - 1] * Ti;
            double qp[3], qy[ND][3], tex = 0.0;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double g[NC], ys[ND], ye[ND], sp, sy[ND], ep, ey[ND], tx;
#pragma unroll
                for (int j = 0; j < NC; ++j) g[j] = gc[((size_t)ax * M + i) * NC + j];
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    ys[d] = ycur[d][ax];
                    ye[d] = ynext[d][ax];
                }
                adjoint_pullback<R>(g, ip, tp, pnext[ax] - pcur[ax], ys, ye, sp, sy, ep, ey, tx);
                tex += tx;
                if (i == 0) {
                    q0p[ax] = sp;
#pragma unroll
                    for (int d = 0; d < ND; ++d) q0y[d][ax] = sy[d];
                } else {
                    qp[ax] = qep[ax] + sp;
#pragma unroll
                    for (int d = 0; d < ND; ++d) qy[d][ax] = qey[d][ax] + sy[d];
                }
                qep[ax] = ep;
#pragma unroll
                for (int d = 0; d < ND; ++d) qey[d][ax] = ey[d];
            }
            double* w = ws + (size_t)i * F * wstride;
            w[(size_t)Rec::TEX * wstride] = tex * ip[1];
            if (i >= 1) {
                // knot i between segment i-1 (sa) and segment i (sb)
                double S[ND][ND], z[ND][3];
#pragma unroll
                for (int r_ = 0; r_ < ND; ++r_) {
#pragma unroll
                    for (int c = 0; c < ND; ++c) S[r_][c] = sa.A11[r_][c] + sb.A00(r_, c);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) z[r_][ax] = qy[r_][ax];
                }
                if (i >= 2) {
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_)
#pragma unroll
                        for (int j = 0; j < ND; ++j) {
#pragma unroll
                            for (int c = 0; c < ND; ++c) S[r_][c] -= sa.A01[j][r_] * Eprev[j][c];
#pragma unroll
                            for (int ax = 0; ax < 3; ++ax) z[r_][ax] -= sa.A01[j][r_] * hprev[j][ax];
                        }
                }
                SmallLDL<ND> ldl;
                ldl.factor(S);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    double col[ND];
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_) col[r_] = z[r_][ax];
                    ldl.solve(col);
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_) hprev[r_][ax] = col[r_];
                }
#pragma unroll
                for (int c = 0; c < ND; ++c) {
                    double col[ND];
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_) col[r_] = sb.A01[r_][c];
                    ldl.solve(col);
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_) Eprev[r_][c] = col[r_];
                }
#pragma unroll
                for (int r_ = 0; r_ < ND; ++r_) {
#pragma unroll
                    for (int c = 0; c < ND; ++c) w[(size_t)(Rec::E + r_ * ND + c) * wstride] = Eprev[r_][c];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) w[(size_t)(Rec::H + r_ * 3 + ax) * wstride] = hprev[r_][ax];
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) w[(size_t)(Rec::QP + ax) * wstride] = qp[ax];
            }
            sa = sb;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                pcur[ax] = pnext[ax];
#pragma unroll
                for (int d = 0; d < ND; ++d) ycur[d][ax] = ynext[d][ax];
            }
        }

        // ---------------- backward sweep: lambda, then the local terms of segment i and of knot i + 1 ----------------
        // here: ycur = y_M, pcur = p_M, (qep, qey) = q of knot M
        double lam_n[ND][3], w_n[3], qp_n[3];   // lambda_{i+1}, w_{i+1}, q^p_{i+1}
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            w_n[ax] = 0.0;
            qp_n[ax] = qep[ax];
#pragma unroll
            for (int d = 0; d < ND; ++d) lam_n[d][ax] = 0.0;
        }
        for (int i = M - 1; i >= 0; --i) {
            const double* w = ws + (size_t)i * F * wstride;
            const double tex = w[(size_t)Rec::TEX * wstride];
            double lam[ND][3], qp_i[3];
            if (i >= 1) {
#pragma unroll
                for (int r_ = 0; r_ < ND; ++r_)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) lam[r_][ax] = w[(size_t)(Rec::H + r_ * 3 + ax) * wstride];
                if (i < M - 1) {
#pragma unroll
                    for (int r_ = 0; r_ < ND; ++r_)
#pragma unroll
                        for (int c = 0; c < ND; ++c) {
                            const double e = w[(size_t)(Rec::E + r_ * ND + c) * wstride];
#pragma unroll
                            for (int ax = 0; ax < 3; ++ax) lam[r_][ax] -= e * lam_n[c][ax];
                        }
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) qp_i[ax] = w[(size_t)(Rec::QP + ax) * wstride];
            } else {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    qp_i[ax] = q0p[ax];
#pragma unroll
                    for (int d = 0; d < ND; ++d) lam[d][ax] = 0.0;
                }
            }
            // ynext = y_{i+1}, pnext = p_{i+1} (kept from the iteration before); ycur = y_i, pcur = p_i
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                pnext[ax] = pcur[ax];
                pcur[ax] = wp[3 * i + ax];
#pragma unroll
                for (int d = 0; d < ND; ++d) ynext[d][ax] = ycur[d][ax];
            }
            load_y(i, ycur);
            const double Ti = T[i];
            SegBlocks<R> sb;
            double ip[NC];
            sb.build(Ti, ip);
            double GT = 0.0;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double dp = pnext[ax] - pcur[ax];
                double wi = 0.0;
#pragma unroll
                for (int r_ = 0; r_ < ND; ++r_) {
                    // T * d/dT of row r_ of F^start_i and F^end_i
                    const double eg = (double)(r_ + 2 - 2 * R);
                    double dFs = -eg * sb.gv(r_) * dp, dFe = eg * sb.gw[r_] * dp;
#pragma unroll
                    for (int c = 0; c < ND; ++c) {
                        const double ex = (double)(r_ + c + 3 - 2 * R);
                        dFs += ex * (sb.A00(r_, c) * ycur[c][ax] + sb.A01[r_][c] * ynext[c][ax]);
                        dFe += ex * (sb.A01[c][r_] * ycur[c][ax] + sb.A11[r_][c] * ynext[c][ax]);
                    }
                    GT += lam[r_][ax] * dFs + lam_n[r_][ax] * dFe;
                    wi += lam[r_][ax] * sb.gv(r_) - lam_n[r_][ax] * sb.gw[r_];
                }
                if (gW) gW[3 * (i + 1) + ax] = qp_n[ax] + wi - w_n[ax];
                w_n[ax] = wi;
                qp_n[ax] = qp_i[ax];
            }
            if (gT) gT[i] = tex - GT * ip[1];
            if (gB && i == M - 1) {
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double v = qey[d][ax];
#pragma unroll
                        for (int c = 0; c < ND; ++c) v -= sb.A01[c][d] * lam[c][ax];
                        gB[(ND + d) * 3 + ax] = v;
                    }
            }
            if (gB && i == 0) {
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double v = q0y[d][ax];
#pragma unroll
                        for (int c = 0; c < ND; ++c) v -= sb.A01[d][c] * lam_n[c][ax];
                        gB[d * 3 + ax] = v;
                    }
            }
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int d = 0; d < ND; ++d) lam_n[d][ax] = lam[d][ax];
        }
        if (gW) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) gW[ax] = qp_n[ax] - w_n[ax];
        }
    }
}

}  // namespace uavqp
