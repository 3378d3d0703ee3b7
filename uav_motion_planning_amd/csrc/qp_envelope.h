// qp_envelope.h -- certified continuous-time bounds of solved trajectories (uavqp_envelope_device, include/uavqp.h): for every segment an
// OUTER range that the quantity cannot leave for any t in [0, T_i] and an INNER range of values it does take, for each axis of position,
// velocity, acceleration and jerk, for |v|, |a|, |j|, the specific thrust |a + g e_z| and the tilt polynomial w; a three-valued verdict
// per segment and per trajectory against optional limits.  The penalties and optimisers SAMPLE; this bounds.
//
// Method (tests/envelope_reference.py restates it line by line in numpy).  n = 2r - 1, derivative order D = 0..3, m = n - D, u = t / T:
//     a_k = falling(k + D, D) c[k + D] T^k                           monomials in u, k = 0..m            S = sum_k |a_k|
//     b_i = sum_{k <= i} C(i,k) / C(m,k) a_k                         Bernstein coefficients on [0, 1]
//     depth levels of midpoint de Casteljau, w <- (w_j + w_{j+1}) / 2: 2^depth leaves, no pruning
//     outer = [min over leaves and i of b_i - G, max + G]            G = 16 (m + 1) 2^-53 S
//     inner = [min, max] over the leaf END coefficients b_0, b_m     (values of the polynomial at t = l T / 2^depth)
// The steps are convex combinations, so their rounding stays a small multiple of 2^-53 S; G is that multiple with room.
// Squared norms, degree 2m, from the UNDIVIDED b of the three axes, then subdivided in the same way:
//     q_k = 1 / C(2m,k) sum_{i+j=k} C(m,i) C(m,j) sum_x b_{x,i} b_{x,j}          Gq = 32 (2m + 1) 2^-53 sum_x S_x^2
// Thrust: q of D = 2 with g = 9.81 added to every z coefficient (the basis sums to one: that shifts the polynomial by g); S_z after the
// shift.  Tilt, c = cos(tilt_max): w = z_z^2 - c^2 |z|^2 from the same products, guard Gq of the thrust; tilt <= tilt_max for all t iff
// w >= 0 and z_z > 0 throughout.  Reported norms are sqrt(max(0, .)) of the guarded squares; w is reported unrooted.
// A non-finite S (or Gq) makes the four numbers of that quantity NaN: no verdict bit can then be set.
//
// Verdict, tests k = 0..6 = v_max, a_max, j_max, f_min, f_max, tilt_max, box: bit 2k certified (the outer bound, guard included, satisfies
// the limit), bit 2k + 1 violated (the inner bound moved TOWARDS the limit by the guard still breaks it), neither = undecided.  Norms are
// tested on the squares against limit * limit.  A trajectory: AND of the certified bits, OR of the violated bits of its segments.
//
// Lanes.  Eight lanes per trajectory (the groups of qp_poly.h), which walk its segments together: on a segment, lane j takes the dyadic
// piece given by the top three bits of the leaf index (three splits, each keeping the left or the right half) and loops over the leaves
// below it; at depth < 3 lanes repeat a leaf.  A leaf's coefficients depend on its path alone and min / max are exact, so the bytes are
// the same for any grid.  The 17 polynomials of a segment have degrees from m = 2 to 2m = 12; every lane takes its eighth of EACH, so no
// lane waits for a longer polynomial.  Both halves of a split are written out with constant indices (a run-time index into the at most 13
// coefficients would put them in scratch); which half is a branch, uniform over the wave below the third level.
// One launch, no scratch memory, no workspace; every output element is written exactly once (zeros included).
//
// Out of scope of this kernel: body-rate and clearance certificates (rational / not polynomial in t) -- clearance against the distance
// field is certified by qp_clearance_cert.h on this kernel's leaves --, pruned or adaptive subdivision, and wiring the verdict into
// uavqp_corridor_pipeline_*.  Registers: DESIGN.md section 5.25.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"

namespace uavqp {

struct EnvelopeArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    const double* box_lo;     // [sum M][3] or null (both or neither)
    const double* box_hi;
    double* range;            // [sum M][4][3][4] or null
    double* norm;             // [sum M][5][4] or null
    double* peak;             // [n_traj][5][4] or null
    int32_t* seg_verdict;     // [sum M] or null
    int32_t* verdict;         // [n_traj] or null
    int depth;
    double v2, a2, j2, fmin2, fmax2;   // limits squared, 0 = test off
    double cos2;                       // cos^2(tilt_max)
    int tilt_on;
};

constexpr double ENV_EPS = 1.1102230246251565e-16;   // 2^-53
constexpr double ENV_GRAVITY = 9.81;                 // the constant of poly_body_frame (qp_poly.h)

UAVQP_HD constexpr double env_binom(int n, int k) {
    double c = 1.0;
    for (int j = 1; j <= k; ++j) c = c * (double)(n - k + j) / (double)j;   // (every intermediate is an integer)
    return c;
}

struct EnvQuad {
    double olo, ilo, ihi, ohi;
};

// One level of midpoint de Casteljau in place, keeping the right half (position j ends as level M - j, element j) or the left half
// (position j ends as level j, element 0).  Both do the same additions.
template <int M>
__device__ __forceinline__ void env_split(double (&w)[M + 1], bool right) {
    if (right) {
#pragma unroll
        for (int k = 1; k <= M; ++k)
#pragma unroll
            for (int j = 0; j <= M - k; ++j) w[j] = 0.5 * (w[j] + w[j + 1]);
    } else {
#pragma unroll
        for (int k = 1; k <= M; ++k)
#pragma unroll
            for (int j = M; j >= k; --j) w[j] = 0.5 * (w[j - 1] + w[j]);
    }
}

__device__ inline double env_group_min(double x) {
#pragma unroll
    for (int d = 1; d < TOPT_LPT; d <<= 1) x = fmin(x, __shfl_xor(x, d, 64));
    return x;
}

// min / max over every coefficient (olo, ohi) and over the end coefficients (ilo, ihi) of all 2^depth leaves of b: this lane's eighth,
// then the group's.  No guard yet.
template <int M>
__device__ __forceinline__ EnvQuad env_scan(const double (&b)[M + 1], int sub, int depth) {
    const int top = depth < 3 ? depth : 3, rest = depth - top;
    const int piece = sub >> (3 - top);
    double p[M + 1];
#pragma unroll
    for (int i = 0; i <= M; ++i) p[i] = b[i];
    for (int s = top - 1; s >= 0; --s) env_split<M>(p, ((piece >> s) & 1) != 0);
    EnvQuad q{INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (int l = 0; l < (1 << rest); ++l) {
        double w[M + 1];
#pragma unroll
        for (int i = 0; i <= M; ++i) w[i] = p[i];
        for (int s = rest - 1; s >= 0; --s) env_split<M>(w, ((l >> s) & 1) != 0);
#pragma unroll
        for (int i = 0; i <= M; ++i) {
            q.olo = fmin(q.olo, w[i]);
            q.ohi = fmax(q.ohi, w[i]);
        }
        q.ilo = fmin(q.ilo, fmin(w[0], w[M]));
        q.ihi = fmax(q.ihi, fmax(w[0], w[M]));
    }
    q.olo = env_group_min(q.olo);
    q.ilo = env_group_min(q.ilo);
    q.ihi = topt_group_max(q.ihi);
    q.ohi = topt_group_max(q.ohi);
    return q;
}

__device__ __forceinline__ EnvQuad env_guarded(EnvQuad q, double G) {
    if (!(G < INFINITY)) return EnvQuad{NAN, NAN, NAN, NAN};   // (a NaN guard too)
    q.olo -= G;
    q.ohi += G;
    return q;
}

// Bernstein coefficients b and S of the D-th derivative of one axis (c: the 2r coefficients of the segment, T its duration)
template <int NC, int D>
__device__ __forceinline__ double env_bernstein(const double (&c)[NC], double T, double (&b)[NC - D]) {
    constexpr int M = NC - 1 - D;
    double a[M + 1], Tk = 1.0, S = 0.0;
#pragma unroll
    for (int k = 0; k <= M; ++k) {
        a[k] = topt_falling(k + D, D) * c[k + D] * Tk;
        S += fabs(a[k]);
        Tk *= T;
    }
#pragma unroll
    for (int i = 0; i <= M; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k <= i; ++k) s = fma(env_binom(i, k) / env_binom(M, k), a[k], s);
        b[i] = s;
    }
    return S;
}

// q_k = 1 / C(2M,k) sum_{i+j=k} C(M,i) C(M,j) (x_i x_j + y_i y_j + z_i z_j); ZZ: the z products alone
template <int M, bool ZZ>
__device__ __forceinline__ void env_square(const double (&b)[3][M + 1], double (&q)[2 * M + 1]) {
#pragma unroll
    for (int k = 0; k <= 2 * M; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = (k > M ? k - M : 0); i <= (k < M ? k : M); ++i) {
            const double wgt = env_binom(M, i) * env_binom(M, k - i) / env_binom(2 * M, k);
            const double d = ZZ ? b[2][i] * b[2][k - i] : fma(b[0][i], b[0][k - i], fma(b[1][i], b[1][k - i], b[2][i] * b[2][k - i]));
            s = fma(wgt, d, s);
        }
        q[k] = s;
    }
}

// the certified / violated bits of test k for "x <= lim" (UPPER) or "x >= lim" on a guarded quad; lim = 0: off
template <bool UPPER>
__device__ __forceinline__ int env_bits(int k, const EnvQuad& q, double G, double lim) {
    if (!(lim > 0.0)) return 0;
    const bool cert = UPPER ? q.ohi <= lim : q.olo >= lim;
    const bool viol = UPPER ? q.ihi - G > lim : q.ilo + G < lim;
    return ((cert ? 1 : 0) | (viol ? 2 : 0)) << (2 * k);
}

__device__ __forceinline__ double env_root(double x) { return sqrt(fmax(0.0, x)); }
__device__ __forceinline__ EnvQuad env_rooted(const EnvQuad& q) {
    if (q.olo != q.olo) return q;   // NaN quad (env_guarded) stays NaN: fmax(0, NaN) would be 0
    return EnvQuad{env_root(q.olo), env_root(q.ilo), env_root(q.ihi), env_root(q.ohi)};
}

__device__ __forceinline__ void env_store(double* p, const EnvQuad& q) {
    p[0] = q.olo; p[1] = q.ilo; p[2] = q.ihi; p[3] = q.ohi;
}

// running min / max of a reported quad over the segments of a trajectory; a NaN quad makes the result NaN
struct EnvPeak {
    EnvQuad q{INFINITY, INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    __device__ __forceinline__ void add(const EnvQuad& s) {
        bad = bad || s.olo != s.olo;
        q.olo = fmin(q.olo, s.olo); q.ilo = fmin(q.ilo, s.ilo);
        q.ihi = fmax(q.ihi, s.ihi); q.ohi = fmax(q.ohi, s.ohi);
    }
    __device__ __forceinline__ EnvQuad get() const { return bad ? EnvQuad{NAN, NAN, NAN, NAN} : q; }
};

// the per-axis part of order D: Bernstein coefficients into b, S into S, the guarded ranges stored and (D = 0) tested against the box
template <int NC, int D>
__device__ __forceinline__ void env_axes(const EnvelopeArgs& a, const double (&c)[3][NC], double T, int sub, size_t seg, bool lead,
                                         double (&b)[3][NC - D], double (&S)[3], EnvQuad (&rq)[3], double (&G)[3]) {
    constexpr int M = NC - 1 - D;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        S[ax] = env_bernstein<NC, D>(c[ax], T, b[ax]);
        G[ax] = 16.0 * (double)(M + 1) * ENV_EPS * S[ax];
        rq[ax] = env_guarded(env_scan<M>(b[ax], sub, a.depth), G[ax]);
        if (a.range && lead) env_store(a.range + ((seg * 4 + D) * 3 + ax) * 4, rq[ax]);
    }
}

// squared norm of order D from b: guarded quad of the SQUARES in sq and the guard in Gq
template <int M>
__device__ __forceinline__ EnvQuad env_norm2(const EnvelopeArgs& a, const double (&b)[3][M + 1], const double (&S)[3], int sub, double& Gq) {
    double q[2 * M + 1];
    env_square<M, false>(b, q);
    Gq = 32.0 * (double)(2 * M + 1) * ENV_EPS * fma(S[0], S[0], fma(S[1], S[1], S[2] * S[2]));
    return env_guarded(env_scan<2 * M>(q, sub, a.depth), Gq);
}

template <int R>
__global__ __launch_bounds__(64) void envelope_kernel(EnvelopeArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_lanes; g += stride) {
        // (the shuffles below stay inside a group, whose eight lanes are live together and walk the same segments)
        const int b = (int)(g / LPT);
        const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        const bool lead = sub == 0;
        EnvPeak pk[5];
        int cert = 0x1555, viol = 0;   // (bits 2k of the seven tests)
        for (int i = 0; i < M; ++i) {
            const size_t seg = (size_t)s0 + i;
            if (!solved) {
                if (lead) {
                    if (a.range)
                        for (int k = 0; k < 48; ++k) a.range[seg * 48 + k] = 0.0;
                    if (a.norm)
                        for (int k = 0; k < 20; ++k) a.norm[seg * 20 + k] = 0.0;
                    if (a.seg_verdict) a.seg_verdict[seg] = 0;
                }
                continue;
            }
            const double T = a.times[seg];
            double c[3][NC];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int k = 0; k < NC; ++k) c[ax][k] = a.coeff[(size_t)3 * NC * s0 + (size_t)ax * axs + (size_t)i * NC + k];
            int bits = 0;
            EnvQuad nq[5];   // reported: |v|, |a|, |j|, thrust, w
            double S[3], G[3], Gq;
            EnvQuad rq[3];
            {   // position: ranges and the box
                double bb[3][NC];
                env_axes<NC, 0>(a, c, T, sub, seg, lead, bb, S, rq, G);
                if (a.box_lo) {
                    bool cb = true, vb = false;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double lo = a.box_lo[seg * 3 + ax], hi = a.box_hi[seg * 3 + ax];
                        cb = cb && lo <= rq[ax].olo && rq[ax].ohi <= hi;
                        vb = vb || rq[ax].ilo + G[ax] < lo || rq[ax].ihi - G[ax] > hi;
                    }
                    bits |= ((cb ? 1 : 0) | (vb ? 2 : 0)) << 12;
                }
            }
            {   // velocity
                double bb[3][NC - 1];
                env_axes<NC, 1>(a, c, T, sub, seg, lead, bb, S, rq, G);
                const EnvQuad sq = env_norm2<NC - 2>(a, bb, S, sub, Gq);
                bits |= env_bits<true>(0, sq, Gq, a.v2);
                nq[0] = env_rooted(sq);
            }
            {   // acceleration, thrust, tilt
                double bb[3][NC - 2];
                env_axes<NC, 2>(a, c, T, sub, seg, lead, bb, S, rq, G);
                EnvQuad sq = env_norm2<NC - 3>(a, bb, S, sub, Gq);
                bits |= env_bits<true>(1, sq, Gq, a.a2);
                nq[1] = env_rooted(sq);
                // z = a + g e_z: the shift of every z coefficient; S_z after the shift (a_0 = b_0 is the only monomial that moves)
                S[2] = S[2] - fabs(bb[2][0]) + fabs(bb[2][0] + ENV_GRAVITY);
#pragma unroll
                for (int k = 0; k < NC - 2; ++k) bb[2][k] += ENV_GRAVITY;
                double qt[2 * (NC - 3) + 1], qz[2 * (NC - 3) + 1];
                env_square<NC - 3, false>(bb, qt);
                env_square<NC - 3, true>(bb, qz);
                Gq = 32.0 * (double)(2 * (NC - 3) + 1) * ENV_EPS * fma(S[0], S[0], fma(S[1], S[1], S[2] * S[2]));
                sq = env_guarded(env_scan<2 * (NC - 3)>(qt, sub, a.depth), Gq);
                bits |= env_bits<false>(3, sq, Gq, a.fmin2) | env_bits<true>(4, sq, Gq, a.fmax2);
                nq[3] = env_rooted(sq);
#pragma unroll
                for (int k = 0; k <= 2 * (NC - 3); ++k) qz[k] = fma(-a.cos2, qt[k], qz[k]);
                nq[4] = env_guarded(env_scan<2 * (NC - 3)>(qz, sub, a.depth), Gq);
                if (a.tilt_on) {
                    const bool ct = nq[4].olo >= 0.0 && rq[2].olo > -ENV_GRAVITY;
                    const bool vt = nq[4].ilo + Gq < 0.0 || rq[2].ilo + G[2] < -ENV_GRAVITY;
                    bits |= ((ct ? 1 : 0) | (vt ? 2 : 0)) << 10;
                }
            }
            {   // jerk
                double bb[3][NC - 3];
                env_axes<NC, 3>(a, c, T, sub, seg, lead, bb, S, rq, G);
                const EnvQuad sq = env_norm2<NC - 4>(a, bb, S, sub, Gq);
                bits |= env_bits<true>(2, sq, Gq, a.j2);
                nq[2] = env_rooted(sq);
            }
            cert &= bits;
            viol |= bits;
#pragma unroll
            for (int k = 0; k < 5; ++k) pk[k].add(nq[k]);
            if (lead) {
                if (a.norm)
#pragma unroll
                    for (int k = 0; k < 5; ++k) env_store(a.norm + (seg * 5 + k) * 4, nq[k]);
                if (a.seg_verdict) a.seg_verdict[seg] = bits;
            }
        }
        if (lead) {
            if (a.peak)
#pragma unroll
                for (int k = 0; k < 5; ++k) env_store(a.peak + ((size_t)b * 5 + k) * 4, solved ? pk[k].get() : EnvQuad{0.0, 0.0, 0.0, 0.0});
            if (a.verdict) a.verdict[b] = solved ? ((cert & 0x1555) | (viol & 0x2aaa)) : 0;
        }
    }
}

}  // namespace uavqp
