// qp_samplers.h -- the kernels that sample solved trajectories and need no obstacle grid: batched evaluation / length (N1), the exhaustive
// SE(3) ellipsoid check (N4) and the time re-allocation.  Emitted by the host translation unit (uavqp.hip).  The segment rule, Horner and
// the body frame they share live in qp_poly.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "qp_poly.h"

namespace uavqp {

// ---------------------------------------------------------------------------------------------------
// N1: batched evaluation on a uniform time grid.  One lane per (trajectory, sample); consecutive lanes are
// consecutive samples of one trajectory, so coefficient reads hit the same few cache lines and the
// output (the dominant traffic: 24 B x K per sample) is fully coalesced.
// ---------------------------------------------------------------------------------------------------
struct EvalArgs {
    int n_traj, uniform, n_samples, what;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    double t0, dt;
    double* out;
};

template <int R>
__global__ __launch_bounds__(256) void eval_kernel(EvalArgs a) {
    constexpr int NC = 2 * R;
    // the 256 lanes of a block own 256 consecutive (trajectory, sample) rows = one contiguous piece of the output: the rows go
    // through LDS (row stride 9 doubles: conflict-free) and leave as 16-byte-per-lane linear stores instead of nine 8-byte stores
    // at a 72-byte lane stride
    __shared__ __attribute__((aligned(16))) double s_o[256 * 9];
    const long long total = (long long)a.n_traj * a.n_samples;
    const int K = __popc(a.what & 7);
    const int tid = threadIdx.x;
    for (long long g0 = (long long)blockIdx.x * 256; g0 < total; g0 += (long long)gridDim.x * 256) {
        const long long g = g0 + tid;
        double res[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) res[k] = 0.0;
        if (g < total) {
            const int b = (int)(g / a.n_samples), s = (int)(g - (long long)b * a.n_samples);
            const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
            if (M >= 1) {
                const double* __restrict__ T = a.times + s0;
                const PolySeg at = poly_segment<true>(T, M, a.t0 + s * a.dt);   // (the form whose loads of T[i] do not wait for the comparisons)
                const double* __restrict__ c = a.coeff + (size_t)3 * NC * s0 + (size_t)at.idx * NC;
                int k = 0;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    if (!((a.what >> d) & 1)) continue;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double* ca = c + (size_t)ax * NC * M;
                        res[k * 3 + ax] = d == 0 ? poly_deriv<NC, 0>(ca, at.t) : d == 1 ? poly_deriv<NC, 1>(ca, at.t) : poly_deriv<NC, 2>(ca, at.t);
                    }
                    ++k;
                }
            }
        }
        const int row = 3 * K;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (k < row) s_o[tid * row + k] = res[k];
        __syncthreads();
        const long long left = total - g0;
        const int n_rows = left < 256 ? (int)left : 256;
        const int n_d = n_rows * row;                          // doubles of this block's piece (even: 256 rows, or handled below)
        double* o = a.out + (size_t)g0 * row;
        const bool al16 = ((reinterpret_cast<uintptr_t>(o)) & 15u) == 0;
        if (al16) {
            for (int i = tid; 2 * i + 1 < n_d; i += 256) *reinterpret_cast<double2*>(o + 2 * i) = *reinterpret_cast<const double2*>(s_o + 2 * i);
            if ((n_d & 1) && tid == 0) o[n_d - 1] = s_o[n_d - 1];
        } else {
            for (int i = tid; i < n_d; i += 256) o[i] = s_o[i];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// N1 (continued): PolyTraj::getTraj + getLength + getMeanVel (traj_utils/poly_traj.hpp:175-207) for a whole batch.
// One wave per trajectory.  Lane 0 repeats the reference's sampling loop to COUNT the samples -- the reference accumulates
// t += dt in floating point and stops at t >= total_time, so for a total time that is a multiple of dt (its own constant
// 1.0 s per segment) the rounding of that accumulation decides whether the last sample exists; the count has to be exact.
// The 64 lanes then evaluate the chords in parallel at t_s = s dt (differs from the accumulated t by ~1e-16 s relative:
// rounding-level differences in the positions) and the wave sums them.
// ---------------------------------------------------------------------------------------------------
struct LengthArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    double dt;
    double* length;
    double* mean_vel;
    int32_t* n_samples;
};

template <int R>
__global__ __launch_bounds__(64) void traj_length_kernel(LengthArgs a) {
    constexpr int NC = 2 * R;
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < a.n_traj; b += gridDim.x) {
        const PolySpan sp = poly_span(a.uniform, a.seg_offsets, b);
        const int M = sp.M;
        const double* __restrict__ T = a.times + sp.s0;
        const double* __restrict__ c = a.coeff + (size_t)3 * NC * sp.s0;
        double total = 0.0;
        int n = 0;
        if (lane == 0) {
            for (int i = 0; i < M; ++i) total += T[i];                      // PolyTraj::init :64-72
            double t = 0.0;
            while (t < total && n < (1 << 24)) { t += a.dt; ++n; }          // getTraj :180-184 (accumulated t)
        }
        total = __shfl(total, 0, 64);
        n = __shfl(n, 0, 64);
        auto pos = [&](int s, double (&p)[3]) {
            const PolySeg at = poly_segment(T, M, (double)s * a.dt);         // evaluatePos :77-88
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) p[ax] = poly_deriv<NC, 0>(c + ((size_t)ax * M + at.idx) * NC, at.t);
        };
        double acc = 0.0;
        if (M >= 1)
            for (int s = lane; s + 1 < n; s += 64) {                        // getLength :189-202: chords between consecutive samples
                double p0[3], p1[3];
                pos(s, p0);
                pos(s + 1, p1);
                const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
                acc += sqrt(dx * dx + dy * dy + dz * dz);
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) {
            if (a.length) a.length[b] = acc;
            if (a.mean_vel) a.mean_vel[b] = acc / total;                    // getMeanVel :204-207
            if (a.n_samples) a.n_samples[b] = n;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// N4: SE(3) ellipsoid collision check.  One lane per (trajectory, sample); obstacle points stream through LDS
// in tiles shared by the 256 samples of a block.
// ---------------------------------------------------------------------------------------------------
struct EllipsoidArgs {
    int n_traj, uniform, n_samples, n_obs;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const double* obs;
    double t0, dt, robot_r, robot_h;
    int32_t* first_hit;
    uint8_t* flags;
};

template <int R>
__global__ __launch_bounds__(256) void ellipsoid_kernel(EllipsoidArgs a) {
    constexpr int NC = 2 * R, TILE = 1024;
    __shared__ double s_obs[TILE * 3];
    const long long total = (long long)a.n_traj * a.n_samples;
    const long long n_round = (total + 255) / 256 * 256;  // every thread of a block joins the LDS tile loads
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_round; g += (long long)gridDim.x * 256) {
        bool live = g < total;
        const int b = live ? (int)(g / a.n_samples) : 0, s = live ? (int)(g - (long long)b * a.n_samples) : 0;
        double p[3] = {0, 0, 0}, b1[3] = {1, 0, 0}, b2[3] = {0, 1, 0}, b3[3] = {0, 0, 1};
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        if (live && M < 1) {  // zero-segment trajectory (flagged invalid by the solver): nothing to sample, reported collision-free
            if (a.flags) a.flags[g] = 0;
            live = false;  // still joins the LDS tile loads below
        }
        if (live) {
            const PolySeg at = poly_segment(a.times + s0, M, a.t0 + s * a.dt);
            double acc[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double* ca = a.coeff + (size_t)3 * NC * s0 + ((size_t)ax * M + at.idx) * NC;
                p[ax] = poly_deriv<NC, 0>(ca, at.t);
                acc[ax] = poly_deriv<NC, 2>(ca, at.t);
            }
            poly_body_frame(acc, b1, b2, b3);
        }
        const double rad2 = (a.robot_r + 1e-1) * (a.robot_r + 1e-1);
        const double ir = 1.0 / a.robot_r, ih = 1.0 / a.robot_h;
        bool hit = false;
        for (int o0 = 0; o0 < a.n_obs; o0 += TILE) {
            const int nt = min(TILE, a.n_obs - o0);
            __syncthreads();
            for (int i = threadIdx.x; i < nt * 3; i += 256) s_obs[i] = a.obs[(size_t)o0 * 3 + i];
            __syncthreads();
            if (live && !hit) {
                for (int i = 0; i < nt; ++i) {
                    const double dx = s_obs[3 * i] - p[0], dy = s_obs[3 * i + 1] - p[1], dz = s_obs[3 * i + 2] - p[2];
                    if (dx * dx + dy * dy + dz * dz <= rad2) {  // the reference's radius search (r + 0.1)
                        const double e1 = (b1[0] * dx + b1[1] * dy + b1[2] * dz) * ir;
                        const double e2 = (b2[0] * dx + b2[1] * dy + b2[2] * dz) * ir;
                        const double e3 = (b3[0] * dx + b3[1] * dy + b3[2] * dz) * ih;
                        if (e1 * e1 + e2 * e2 + e3 * e3 <= 1.0) { hit = true; break; }  // |E^-1 d| <= 1
                    }
                }
            }
        }
        if (live) {
            if (a.flags) a.flags[g] = hit ? 1 : 0;
            if (hit) atomicMin(&a.first_hit[b], s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Time re-allocation: eight lanes per trajectory; peak |v|, |a| by sampling, stretch-only update of T by one factor per trajectory.
// ---------------------------------------------------------------------------------------------------
struct ReallocArgs {
    int n_traj, uniform, samples;
    const int32_t* seg_offsets;
    double* times;
    const double* coeff;
    double v_max, a_max, max_stretch;
    double dead_band, overshoot;  // uavqp_settings.realloc_dead_band / realloc_overshoot
    int32_t* changed;
    double* scale_acc;            // optional [n_traj]: multiplied by the factor applied (the pipeline's record of how far a trajectory was stretched)
    const int32_t* list;          // optional: only these trajectories, *n_list of them (the pipeline's later rounds: a trajectory the last round
    const int* n_list;            // did not stretch was not re-solved -- its peaks, and so its verdict, are what they were)
};

template <int R>
__global__ __launch_bounds__(64) void realloc_kernel(ReallocArgs a) {
    // The whole trajectory is scaled by ONE factor.  (Stretching single segments diverges: a long segment next to short
    // ones inherits their knot acceleration and overshoots more the longer it gets; under uniform scaling T -> sT speeds
    // drop ~1/s and accelerations ~1/s^2.)  Eight lanes per trajectory: sub-lane j samples segments j, j + 8, ..., the
    // peaks are combined with three xor-shuffles (max is order-independent: same result as a single lane), every lane
    // then scales its own segments.
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    topt_for_each_group(a.list ? *a.n_list : a.n_traj, [&](bool live, int k, int sub) {
        const int b = live && a.list ? a.list[k] : k;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        double v2 = 0.0, a2 = 0.0;
        for (int i = sub; i < M; i += LPT) {
            const double T = a.times[s0 + i];
            const double* __restrict__ c = a.coeff + (size_t)3 * NC * s0 + (size_t)i * NC;
            for (int s = 0; s <= a.samples; ++s) {
                const double t = T * (double)s / (double)a.samples;
                double vs = 0.0, as = 0.0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double* ca = c + (size_t)ax * NC * M;
                    const double v = poly_deriv<NC, 1>(ca, t), ac = poly_deriv<NC, 2>(ca, t);
                    vs += v * v;
                    as += ac * ac;
                }
                // a NaN sample marks the peak with +Inf (fmax alone would drop it and let the other samples decide): the mark travels
                // through the maxima and the shuffles below like any peak, and an infinite ratio leaves the whole trajectory alone
                v2 = fmax(v2, vs == vs ? vs : INFINITY);
                a2 = fmax(a2, as == as ? as : INFINITY);
            }
        }
        v2 = topt_group_max(v2);
        a2 = topt_group_max(a2);
        if (!live) return;
        const double ratio = fmax(sqrt(v2) / a.v_max, sqrt(sqrt(a2) / a.a_max));
        int ch = 0;
        // dead band (default 1 %) and overshoot (default 2 %) so that the loop settles instead of creeping towards the limit
        if (ratio > a.dead_band && ratio < INFINITY) {
            const double s = fmin(a.overshoot * ratio, a.max_stretch);
            for (int i = sub; i < M; i += LPT) a.times[s0 + i] *= s;
            ch = M;
            if (a.scale_acc && sub == 0) a.scale_acc[b] *= s;
        }
        if (a.changed && sub == 0) a.changed[b] = ch;
    });
}

}  // namespace uavqp
