// qp_clearance_cert.h -- certified continuous-time clearance of solved trajectories against the distance field
// (uavqp_clearance_certificate_device, include/uavqp.h): for every segment a LOWER bound of min_t dist(p(t), O) that holds for every t in
// [0, T_i] and an UPPER bound taken at a known t, and a verdict against a required clearance d_req.  The clearance penalty, the ellipsoid
// checks and the pipeline's grid check SAMPLE; a thin pillar between two samples passes them.  This bounds.
//
// Obstacle set.  O = the union of the CLOSED cubes of the occupied voxels, plus everything outside the map (unknown space counts as
// occupied).  res the voxel edge, c_v = origin + (v + 0.5) res the centre of voxel v, sq_pos[v] the exact integer squared voxel distance
// from v to the nearest occupied voxel (uavqp_esdf_update_device, qp_esdf.h), s_v = res sqrt(sq_pos[v]), +inf where sq_pos[v] = INT32_MAX.
//
// The two inequalities, for a point p and ANY voxel v (the kernel takes the voxel of p, floor((p - origin) / res) clamped into the grid,
// which makes |p - c_v| small; which voxel a rounded index picks does not touch soundness):
//     lower   dist(p, occupied cubes) >= s_v - (sqrt(3)/2) res - |p - c_v|
//             every occupied centre c_o has |c_o - c_v| >= s_v; every point q of that cube has |q - c_o| <= (sqrt(3)/2) res; so
//             |p - q| >= |c_v - c_o| - |c_o - q| - |p - c_v|.
//     upper   dist(p, occupied cubes) <= s_v + |p - c_v| - res/2, and 0 when sq_pos[v] = 0
//             the nearest occupied cube has its centre at s_v from c_v and contains the ball of radius res/2 about that centre.
//
// Leaves (tests/clearance_cert_reference.py restates all of this line by line in numpy).  The D = 0 Bernstein coefficients of the three
// axes (env_bernstein, qp_envelope.h) and depth levels of midpoint de Casteljau (env_split) give 2^depth leaves, the sub-curves over
// [l, l + 1] T_i / 2^depth.  By the convex hull property the curve over a leaf stays in the axis-aligned box of that leaf's coefficients,
// widened per axis by the envelope's guard G_x = 16 (n + 1) 2^-53 S_x (n + 1 = 2r coefficients, S_x = sum_k |c_k T^k|):
//     lo_x = min_i w_{x,i} - G_x,  hi_x = max_i w_{x,i} + G_x,  m = (lo + hi) / 2,  h = |(hi - lo) / 2|  (half diagonal),  v = voxel of m
//     L_leaf = min( s_v - (sqrt(3)/2) res - |m - c_v| - h ,  min_x min(lo_x - origin_x, top_x - hi_x) ) - R
// (every point of the box is within h of m; the second term is the distance from the box to the nearest face of the map, negative when
// the box crosses a face: such a box cannot be certified).
// Witness points are the leaf END coefficients, p_l = the curve at t = l T_i / 2^depth, l = 0..2^depth (each computed value is within
// G_x of the true one per axis, that is within sqrt(3) max_x G_x in distance), v the voxel of p_l:
//     U_l = s_v + |p_l - c_v| - res/2 + sqrt(3) max_x G_x + R          p_l inside the map and sq_pos[v] > 0
//     U_l =                             sqrt(3) max_x G_x + R          p_l outside the map (a coordinate below origin or above top) or sq_pos[v] = 0
// Per segment:  lower = max(0, min over leaves of L_leaf),  upper = min_l U_l,  witness = the smallest l that attains it.  The true
// min_t dist(p(t), O) lies in [lower, upper].
//
// R, the rounding allowance of the field arithmetic:  R = 64 2^-53 (max_x S_x + A),  A = max_x max(|origin_x|, |top_x|) + res |dims|
// (the largest coordinate of the map plus its diagonal, computed once on the host).  Every operand of the formulas above -- a leaf
// coefficient, a box corner, a voxel centre, s_v where it is finite, their differences -- is at most max_x S_x + A in magnitude, each of
// the about twenty roundings from the guarded box to L_leaf or U_l loses at most 2^-53 of that, and the guard G_x already covers the
// subdivision: 64 leaves room.  A non-finite S_x makes lower and upper NaN, the witness 0 and the verdict 0.
//
// Verdict per segment: UAVQP_CLEARANCE_CERTIFIED lower >= d_req (holds for ALL t), UAVQP_CLEARANCE_VIOLATED upper < d_req (broken at
// the witness), UAVQP_CLEARANCE_OUTSIDE some witness point lies outside the map.  A trajectory: AND of the certified bits, OR of the other two.
//
// Lanes.  The scheme of qp_envelope.h: eight lanes per trajectory walk its segments together; on a segment, lane j takes the dyadic piece
// given by the top three bits of the leaf index and loops over the leaves below it; at depth < 3 lanes repeat a leaf.  Only the three
// D = 0 polynomials are subdivided (2 x 3 x 2r doubles live: no scratch).  A leaf costs one gathered int32 load from sq_pos for its box
// and one for its left end; the last leaf of the segment adds its right end.  min is exact and a tie between witnesses goes to the
// smallest l, so the bytes are the same for any grid.  Both halves of a split have constant indices (env_split); nothing is indexed at run time.
// One launch, no LDS, no scratch, no workspace, no atomics; every output element is written exactly once (zeros included).
//
// Out of scope: a tighter bound from a scan of the voxel's neighbourhood (the field alone leaves an undecided band of about
// 2 res + 2 h between lower and upper), adaptive subdivision, a body-rate certificate, and wiring the verdict into uavqp_corridor_pipeline_*.
// Registers and what bounds the kernel: DESIGN.md section 5.26.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_envelope.h"

namespace uavqp {

struct ClearanceCertArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    const int32_t* sq_pos;    // [nx][ny][nz] of the map, z fastest
    int nx, ny, nz;
    double ox, oy, oz;        // origin
    double hx, hy, hz;        // top = origin + dims * res
    double res, inv_res;
    double mag;               // A of the header: largest |coordinate| of the map + its diagonal
    double d_req;
    int depth;
    double* clear;            // [sum M][2] or null
    int32_t* witness;         // [sum M] or null
    double* peak;             // [n_traj][2] or null
    int32_t* seg_verdict;     // [sum M] or null
    int32_t* verdict;         // [n_traj] or null
};

constexpr double CC_SQRT3 = 1.7320508075688772;
constexpr double CC_HALF_SQRT3 = 0.8660254037844386;

// the voxel of p (clamped into the grid; a NaN coordinate gives index 0): s_v, |p - c_v| and sq_pos[v]
__device__ __forceinline__ void cc_lookup(const ClearanceCertArgs& a, double px, double py, double pz, double& s, double& off, int32_t& sq) {
    const double fx = fmin(fmax(floor((px - a.ox) * a.inv_res), 0.0), (double)(a.nx - 1));
    const double fy = fmin(fmax(floor((py - a.oy) * a.inv_res), 0.0), (double)(a.ny - 1));
    const double fz = fmin(fmax(floor((pz - a.oz) * a.inv_res), 0.0), (double)(a.nz - 1));
    sq = a.sq_pos[((int)fx * a.ny + (int)fy) * a.nz + (int)fz];
    const double dx = px - (a.ox + (fx + 0.5) * a.res), dy = py - (a.oy + (fy + 0.5) * a.res), dz = pz - (a.oz + (fz + 0.5) * a.res);
    off = sqrt(dx * dx + dy * dy + dz * dz);
    s = sq == INT32_MAX ? INFINITY : a.res * sqrt((double)sq);
}

// U_l - (sqrt(3) max G + R) of one witness point; out: it lies outside the map
__device__ __forceinline__ double cc_witness(const ClearanceCertArgs& a, double px, double py, double pz, bool& out) {
    double s, off;
    int32_t sq;
    cc_lookup(a, px, py, pz, s, off, sq);
    out = !(px >= a.ox && px <= a.hx && py >= a.oy && py <= a.hy && pz >= a.oz && pz <= a.hz);
    return out || sq == 0 ? 0.0 : s + off - 0.5 * a.res;
}

// (u, l) <- the smaller of (u, l) and (ou, ol): by u, a tie by l
__device__ __forceinline__ void cc_take(double& u, int& l, double ou, int ol) {
    if (ou < u || (ou == u && ol < l)) {
        u = ou;
        l = ol;
    }
}

template <int R>
__global__ __launch_bounds__(64) void clearance_cert_kernel(ClearanceCertArgs a) {
    constexpr int NC = 2 * R, M1 = NC - 1, LPT = TOPT_LPT;
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int top = a.depth < 3 ? a.depth : 3, rest = a.depth - top;
    const int piece = sub >> (3 - top);
    const int last = (1 << a.depth) - 1;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_lanes; g += stride) {
        // (the shuffles below stay inside a group, whose eight lanes are live together and walk the same segments)
        const int b = (int)(g / LPT);
        const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        const bool lead = sub == 0;
        double pk_lo = INFINITY, pk_hi = INFINITY;
        bool pk_bad = false;
        int cert = UAVQP_CLEARANCE_CERTIFIED, other = 0;
        for (int i = 0; i < M; ++i) {
            const size_t seg = (size_t)s0 + i;
            if (!solved) {
                if (lead) {
                    if (a.clear) a.clear[seg * 2] = a.clear[seg * 2 + 1] = 0.0;
                    if (a.witness) a.witness[seg] = 0;
                    if (a.seg_verdict) a.seg_verdict[seg] = 0;
                }
                continue;
            }
            const double T = a.times[seg];
            double p[3][NC], G[3], Smax = 0.0, Gmax = 0.0;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double c[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) c[k] = a.coeff[(size_t)3 * NC * s0 + (size_t)ax * axs + (size_t)i * NC + k];
                const double S = env_bernstein<NC, 0>(c, T, p[ax]);
                G[ax] = 16.0 * (double)NC * ENV_EPS * S;
                Smax = S > Smax || S != S ? S : Smax;   // (a NaN stays)
                Gmax = G[ax] > Gmax || G[ax] != G[ax] ? G[ax] : Gmax;
            }
            const double Rr = 64.0 * ENV_EPS * (Smax + a.mag);
            const double pad = CC_SQRT3 * Gmax + Rr;
            for (int s = top - 1; s >= 0; --s) {
                const bool right = ((piece >> s) & 1) != 0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) env_split<M1>(p[ax], right);
            }
            double low = INFINITY, up = INFINITY;
            int wit = INT32_MAX;
            bool outside = false;
            for (int l = 0; l < (1 << rest); ++l) {
                double w[3][NC];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int k = 0; k < NC; ++k) w[ax][k] = p[ax][k];
                for (int s = rest - 1; s >= 0; --s) {
                    const bool right = ((l >> s) & 1) != 0;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) env_split<M1>(w[ax], right);
                }
                // the guarded box of the leaf: centre m, half extents e
                double m[3], e[3], face = INFINITY;
                const double o3[3] = {a.ox, a.oy, a.oz}, h3[3] = {a.hx, a.hy, a.hz};
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    double lo = w[ax][0], hi = w[ax][0];
#pragma unroll
                    for (int k = 1; k < NC; ++k) {
                        lo = fmin(lo, w[ax][k]);
                        hi = fmax(hi, w[ax][k]);
                    }
                    lo -= G[ax];
                    hi += G[ax];
                    m[ax] = 0.5 * (lo + hi);
                    e[ax] = 0.5 * (hi - lo);
                    face = fmin(face, fmin(lo - o3[ax], h3[ax] - hi));
                }
                const double h = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
                double sv, off;
                int32_t sq;
                cc_lookup(a, m[0], m[1], m[2], sv, off, sq);
                low = fmin(low, fmin(sv - CC_HALF_SQRT3 * a.res - off - h, face) - Rr);
                // the witnesses: this leaf's left end, and the right end of the segment's last leaf
                const int leaf = (piece << rest) | l;
                bool out;
                cc_take(up, wit, cc_witness(a, w[0][0], w[1][0], w[2][0], out) + pad, leaf);
                outside = outside || out;
                if (leaf == last) {
                    cc_take(up, wit, cc_witness(a, w[0][M1], w[1][M1], w[2][M1], out) + pad, leaf + 1);
                    outside = outside || out;
                }
            }
            low = env_group_min(low);
#pragma unroll
            for (int d = 1; d < LPT; d <<= 1) cc_take(up, wit, __shfl_xor(up, d, 64), __shfl_xor(wit, d, 64));
            outside = topt_group_max(outside ? 1.0 : 0.0) != 0.0;
            const bool bad = !(Rr < INFINITY);   // (a NaN too)
            const double lower = bad ? NAN : fmax(0.0, low), upper = bad ? NAN : up;
            const int bits = bad ? 0
                                 : (lower >= a.d_req ? UAVQP_CLEARANCE_CERTIFIED : 0) | (upper < a.d_req ? UAVQP_CLEARANCE_VIOLATED : 0) |
                                       (outside ? UAVQP_CLEARANCE_OUTSIDE : 0);
            cert &= bits;
            other |= bits;
            pk_bad = pk_bad || bad;
            pk_lo = fmin(pk_lo, lower);
            pk_hi = fmin(pk_hi, upper);
            if (lead) {
                if (a.clear) {
                    a.clear[seg * 2] = lower;
                    a.clear[seg * 2 + 1] = upper;
                }
                if (a.witness) a.witness[seg] = bad ? 0 : wit;
                if (a.seg_verdict) a.seg_verdict[seg] = bits;
            }
        }
        if (lead) {
            if (a.peak) {
                a.peak[(size_t)b * 2] = !solved ? 0.0 : pk_bad ? NAN : pk_lo;
                a.peak[(size_t)b * 2 + 1] = !solved ? 0.0 : pk_bad ? NAN : pk_hi;
            }
            if (a.verdict)
                a.verdict[b] = solved ? ((cert & UAVQP_CLEARANCE_CERTIFIED) | (other & (UAVQP_CLEARANCE_VIOLATED | UAVQP_CLEARANCE_OUTSIDE))) : 0;
        }
    }
}

}  // namespace uavqp
