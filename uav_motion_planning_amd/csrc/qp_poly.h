// qp_poly.h -- what every kernel that samples a solved trajectory shares: the span of a trajectory in the segment arrays, the segment
// rule of PolyTraj::evaluatePos, Horner on a derivative, the body frame of an acceleration, and the eight-lanes-per-trajectory loop.
// No state; compiles without the HIP runtime too (tests/cpp/test_poly_rule.cpp pins the rule, Horner and the frame on the CPU).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define UAVQP_HD __host__ __device__
#define UAVQP_UNROLL _Pragma("unroll")
#else
#define UAVQP_HD
#define UAVQP_UNROLL
#endif
#include <math.h>
#include <stdint.h>

namespace uavqp {

// first segment and segment count of trajectory b
struct PolySpan {
    int s0, M;
};
UAVQP_HD inline PolySpan poly_span(int uniform, const int32_t* seg_offsets, int b) {
    if (uniform > 0) return {b * uniform, uniform};
    const int s0 = seg_offsets[b];
    return {s0, seg_offsets[b + 1] - s0};
}

// The walk of PolyTraj::evaluatePos (traj_utils/poly_traj.hpp:77-88) leaves a segment only when t is past its end by more than the
// slack: on a knot the earlier segment answers.
UAVQP_HD inline bool poly_past_segment(double t, double Ti) { return t > Ti + 1e-4; }

struct PolySeg {
    int idx;     // segment of t
    double t;    // segment-local time
    bool past;   // t lay past the end of the trajectory: idx, t are the end point of the last segment
};
// Segment and segment-local time of trajectory time t over the durations T[0..M), M >= 1 (the caller handles M < 1).
// EVERY = true reads every duration whatever the comparisons say, so that the loads do not wait for them (eval_kernel); it does the same
// subtractions in the same order as the early exit and returns the same bits (pinned by tests/cpp/test_poly_rule.cpp).
template <bool EVERY = false>
UAVQP_HD inline PolySeg poly_segment(const double* T, int M, double t) {
    int idx = 0;
    double Tlast = 0.0;
    if (EVERY) {
        bool going = true;
        for (int i = 0; i < M; ++i) {
            Tlast = T[i];
            going = going & poly_past_segment(t, Tlast);
            t = going ? t - Tlast : t;
            idx += going ? 1 : 0;
        }
    } else {
        while (idx < M && poly_past_segment(t, T[idx])) t -= T[idx++];
    }
    const bool past = idx == M;
    if (past) {
        --idx;
        t = EVERY ? Tlast : T[idx];
    }
    return {idx, t, past};
}

UAVQP_HD constexpr double topt_falling(int k, int d) {   // k! / (k - d)!
    double f = 1.0;
    for (int j = 0; j < d; ++j) f *= (double)(k - j);
    return f;
}

// D-th derivative at t of the polynomial with coefficients c[0..NC), by Horner
template <int NC, int D>
UAVQP_HD inline double poly_deriv(const double* c, double t) {
    double v = 0.0;
    UAVQP_UNROLL
    for (int j = NC - 1; j >= D; --j) v = fma(v, t, D == 0 ? c[j] : topt_falling(j, D) * c[j]);
    return v;
}

// Body axes of the attitude that produces acceleration acc against gravity (kino_astar.cpp:724-727): b3 along the thrust, b2 = b3 x e_x
// normalised, b1 = b2 x b3 normalised.  Free fall, or a thrust along e_x, has no such attitude: the axes are NaN, every test against
// them is false and the sample counts as collision-free, as in the reference.
UAVQP_HD inline void poly_body_frame(const double* acc, double* b1, double* b2, double* b3) {
    const double n3 = sqrt(acc[0] * acc[0] + acc[1] * acc[1] + (acc[2] + 9.81) * (acc[2] + 9.81));
    b3[0] = acc[0] / n3; b3[1] = acc[1] / n3; b3[2] = (acc[2] + 9.81) / n3;
    const double c2[3] = {0.0, b3[2], -b3[1]};
    const double n2 = sqrt(c2[1] * c2[1] + c2[2] * c2[2]);
    b2[0] = 0.0; b2[1] = c2[1] / n2; b2[2] = c2[2] / n2;
    const double c1[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
    const double n1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    b1[0] = c1[0] / n1; b1[1] = c1[1] / n1; b1[2] = c1[2] / n1;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------------
// Lane groups: eight lanes per trajectory, sub-lane j takes segments j, j + 8, ..., values are combined with three xor-shuffles (a
// butterfly: every lane of the group ends with the same bits, and the order of the additions is fixed by the segment index alone -- the
// same result run to run and for any grid).
// ---------------------------------------------------------------------------------------------------
constexpr int TOPT_LPT = 8;   // lanes per trajectory

__device__ inline double topt_group_sum(double x) {
#pragma unroll
    for (int d = 1; d < TOPT_LPT; d <<= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ inline double topt_group_max(double x) {
#pragma unroll
    for (int d = 1; d < TOPT_LPT; d <<= 1) x = fmax(x, __shfl_xor(x, d, 64));
    return x;
}

// body(live, k, sub) for every group k < n_groups, grid-stride; the count is rounded up to whole waves so that every lane reaches the
// shuffles of the body: the lanes of the surplus get live = false and k = 0.  `return` in the body is the loop's `continue`.
template <class Body>
__device__ __forceinline__ void topt_for_each_group(long long n_groups, Body&& body) {
    const int sub = threadIdx.x % TOPT_LPT;
    const long long n_lanes = n_groups * TOPT_LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        body(live, live ? (int)(g / TOPT_LPT) : 0, sub);
    }
}
#endif  // __HIPCC__

}  // namespace uavqp
