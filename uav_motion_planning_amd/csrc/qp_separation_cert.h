// qp_separation_cert.h -- certified continuous-time separation between the vehicles of a swarm (uavqp_separation_certificate_device,
// include/uavqp.h): for every vehicle a LOWER bound of its separation from every partner that holds for EVERY t of a clock window, an
// UPPER bound taken at a reported instant and partner, and a three-valued verdict against d_req.  The swarm penalty and its optimiser
// SAMPLE the shared clock (min_sep); two vehicles that close d_safe between two samples pass them.  This bounds.
//
// The certified curve.  The clock knots of vehicle b are the DOUBLES K_0 = start_b, K_{m+1} = fl(K_m + T_m).  q_b(t) is segment 0 at local
// time 0 for t <= K_0 (the vehicle waits), segment m at local time t - K_m (real arithmetic) for t in [K_m, K_{m+1}], the last segment at
// T_{M-1} for t >= K_M (it has arrived).  Pieces are closed: at a knot both values belong to the curve (the leaf on either side of the
// knot sees its own; at the last instant of the window the curve is the piece the last leaf lies in).  This is the swarm penalty's curve
// without the 1e-4 s of overhang poly_past_segment allows.  s_ij(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) of q_i(t) - q_j(t).
//
// Leaves.  h = dt / 2^depth, tau_w = fl(clock_start + w h) (one rounding: the nearest double), w = 0..NL, NL = n_cells 2^depth; leaf l is
// [tau_l, tau_{l+1}].  With depth = 0 the tau_w are the penalty's sample instants.  n = 2r - 1.
//
// Entries (tests/separation_cert_reference.py restates all of this in numpy).  Per (vehicle, leaf), every segment m whose closed piece
// meets the leaf (K_m <= tau_{l+1} and K_{m+1} >= tau_l; not the last one at K_M = tau_l: that leaf has arrived) is restricted to the
// leaf: env_bernstein on the segment (qp_envelope.h), then two general-ratio de Casteljau splits, with the leaf's ends in local time clamped to the piece, la = max(tau_l - K_m, 0), lb = min(tau_{l+1}
// - K_m, T_m):  the first at lambda_1 = lb / T_m keeps the left half, the second at lambda_2 = la / lb keeps the right half, both ratios
// clamped to [0, 1] (a NaN ratio, 0 / 0, counts as 0).  A hold is the same with fixed ratios: waiting (tau_{l+1} <= K_0) segment 0 at
// lambda_1 = lambda_2 = 0, arrived (tau_l >= K_M) the last segment at lambda_1 = lambda_2 = 1: a constant polynomial.
//   single   the leaf lies in ONE piece -- waiting, arrived, or K_m <= tau_l and tau_{l+1} <= K_{m+1} on the doubles: the entry is the
//            3 x (n + 1) coefficients of that piece.
//   box      otherwise (the leaf straddles a knot, the departure, the arrival, or several): the entry is the per-axis [lo, hi] over the
//            coefficients of every restricted piece (the held points are the end coefficients of the first and of the last segment, which
//            the clamps put into their pieces), the position at the leaf's left end (coefficient 0 of the first piece) and at its right
//            end (coefficient n of the last).
// Guard per axis, G_x = (64 (n + 1) + 2 n kappa) 2^-53 S_x, the largest over the pieces of the entry; S_x = sum_k |c_k T^k| of the segment
// (env_bernstein), kappa = max(|K_m|, |K_{m+1}|) / T_m.  Derivation, in units of 2^-53 S_x: env_bernstein leaves its coefficients within
// 16 (n + 1) (qp_envelope.h).  A split is n levels of fl(fl(1 - lambda) a) + lambda b with |a|, |b| <= S: two roundings and the rounded
// weight, 3 n per split, 6 n for two.  The ratios: tau and K are doubles by definition, so la, lb carry one rounding each and the two
// quotients one more, together under 8 in the parameter u = t_local / T_m; a coefficient of the restricted piece is a blossom value of the
// segment, which moves by at most |dp/du| <= sum_k k |a_k| <= n S per unit of u: 8 n.  Sum 16 (n + 1) + 14 n < 30 (n + 1): 64 (n + 1) leaves
// room.  The last term: K_{m+1} is the ROUNDED sum, so a t of the piece may have t - K_m > T_m by up to 2^-53 |K_m + T_m|, that is u beyond
// 1 by delta <= 2^-53 kappa (1 + 2^-52), where the curve leaves the hull of the clamped piece by at most n S (1 + delta)^(n-1) delta:
// 2 n kappa covers it while delta < 1e-3 (a duration not absurdly small against the clock time; T_m <= 0 makes the guard non-finite).
// A non-finite guard (non-finite coefficients or duration of a piece the window meets) makes the bounds of the vehicle AND of its
// partners NaN, their `where` {-1, 0, -1, 0} and their words 0.
//
// Pair (i, j) on leaf l, Gs_x = G_ix + G_jx:
//   both single   lo_x = min_k (b_ik - b_jk), hi_x = max_k: both are Bernstein in the same parameter over the same leaf, so their difference
//                 is Bernstein too and correlated motion cancels
//   otherwise     lo_x = lo_ix - hi_jx, hi_x = hi_ix - lo_jx, the box of a single entry being the min / max of its coefficients
//   lo_x -= Gs_x, hi_x += Gs_x;  g_x = max(0, lo_x, -hi_x);  L = sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R,
//   R = 16 2^-53 (m_x + m_y + m_z), m_x = max(|lo_x|, |hi_x|): the differences and the widening lose 2 2^-53 m_x per axis, the squares, their
//   sum, the root and 1 / downwash (a rounded reciprocal) under 6 2^-53 of the norm, which is at most m_x + m_y + m_z.
//   Witness at the leaf's left end (and, for the last leaf, at its right end), p the entries' end positions, d = p_i - p_j:
//   U = sqrt(d_x^2 + d_y^2 + (d_z / downwash)^2) + sqrt(3) max_x Gs_x + 16 2^-53 (|d_x| + |d_y| + |d_z|)
//   (each end position is within G of the true one per axis).
// fl(a - b) = -fl(b - a), so L and U of (i, j) are the bits of (j, i).
// Per vehicle:  lower = max(0, min over partners and leaves of L), upper = min over partners and witnesses of U; a tie goes to the smaller
// partner, then to the smaller index.  Every min is exact: the same bytes for any grid, run to run, alone or inside a batch.
//
// Work: the lane scheme of qp_swarm.h.  One workgroup of SEP_BLOCK lanes per swarm of A vehicles (grid-stride over the swarms), the leaves
// in rising tiles of TL = SEP_ENTRIES / A.  Per tile, three phases over LDS:
//   1. locate + restrict: one lane per (vehicle, leaf) walks the vehicle's knots and leaves the entry in LDS.  Nothing after this phase
//      touches times or coefficients.
//   2. pairs: one lane per (vehicle i, leaf) holds its entry in registers and runs over the partners' entries in LDS (lanes of a wave share
//      few leaves: a partner's coefficient is a broadcast read); leaves (L, partner) and (U, partner, end) in LDS.
//   3. fold: lane i owns vehicle i, folds its leaves of the tile into registers that live across tiles, and stores once after the last;
//      lane 0 forms the swarm's word.
// Both splits are written out with constant indices (env_split's way): nothing is indexed at run time, no scratch.
// LDS per workgroup: (3 x 2r + 3) doubles + 1 int per entry, 2 doubles + 2 ints of results per entry, 2 x SEP_BLOCK ints: 63488 bytes at
// r = 4, 51200 at r = 3 (static, under 64 KiB); two workgroups per CU, which is what the launch caps its grid at (uavqp_separation_cert.h).
// No atomics, no workspace, no memset: every output element is written exactly once.
// A swarm of more than SWARM_MAX vehicles (the _host entry refuses it) is not evaluated: NaN bounds, zero words, nothing in LDS.
//
// Out of scope: splitting a straddling leaf at the pair's merged knots (without it a straddling leaf falls back to boxes), a degree-2n
// squared-distance polynomial per pair, adaptive subdivision, non-cooperative obstacles, and wiring the verdict into uavqp_swarm_optimize_*.
// Registers and what bounds the kernel: DESIGN.md section 5.27.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_envelope.h"
#include "qp_swarm.h"

namespace uavqp {

constexpr int SEP_BLOCK = SWARM_MAX;      // one lane per vehicle in phase 3
constexpr int SEP_ENTRIES = 256;          // (vehicle, leaf) entries of one tile: two leaves of the largest swarm
constexpr double SEP_SQRT3 = 1.7320508075688772;

struct SeparationCertArgs {
    int n_traj, uniform, n_groups;
    const int32_t* seg_offsets;
    const int32_t* group_offsets;   // null: one swarm, the whole batch
    const double* times;
    const double* coeff;
    const int32_t* status;          // null: every trajectory counts as solved
    const double* start;            // null: all zero
    double* lower;                  // [n_traj] or null
    double* upper;                  // [n_traj] or null
    int32_t* where;                 // [n_traj][4] or null
    int32_t* verdict;               // [n_traj] or null
    int32_t* group_verdict;         // [n_groups] or null
    int n_leaves;                   // NL = n_cells 2^depth
    double clock_start, h;          // h = dt / 2^depth
    double inv_dw;                  // 1 / downwash
    double d_req;
};

enum : int { SEP_SINGLE = 0, SEP_BOX = 1 };

// One general-ratio de Casteljau split in place: the left half [0, lam] (position j ends as level j, element 0) ...
template <int M>
__device__ __forceinline__ void sep_split_left(double (&w)[M + 1], double lam) {
    const double om = 1.0 - lam;
#pragma unroll
    for (int k = 1; k <= M; ++k)
#pragma unroll
        for (int j = M; j >= k; --j) w[j] = fma(lam, w[j], om * w[j - 1]);
}
// ... or the right half [lam, 1] (position j ends as level M - j, element j)
template <int M>
__device__ __forceinline__ void sep_split_right(double (&w)[M + 1], double lam) {
    const double om = 1.0 - lam;
#pragma unroll
    for (int k = 1; k <= M; ++k)
#pragma unroll
        for (int j = 0; j <= M - k; ++j) w[j] = fma(lam, w[j + 1], om * w[j]);
}

__device__ __forceinline__ double sep_ratio(double x) { return fmin(fmax(x, 0.0), 1.0); }   // (fmax(NaN, 0) = 0)

// what phase 1 gathers over the pieces of one entry
template <int NC>
struct SepEntry {
    double p[3][NC];                 // the piece restricted last
    double lo[3], hi[3], G[3];       // over every piece so far
    double left[3];                  // coefficient 0 of the first piece
    int pieces = 0;

    // segment m (c: its coefficients of axis 0, axs: doubles from one axis to the next) restricted to [lam2 lam1, lam1] of its [0, 1]
    __device__ __forceinline__ void add(const double* c, size_t axs, double T, double kappa, double lam1, double lam2) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            double cc[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) cc[k] = c[(size_t)ax * axs + k];
            const double S = env_bernstein<NC, 0>(cc, T, p[ax]);
            const double g = (64.0 * (double)NC + 2.0 * (double)(NC - 1) * kappa) * ENV_EPS * S;
            sep_split_left<NC - 1>(p[ax], lam1);
            sep_split_right<NC - 1>(p[ax], lam2);
            double l = p[ax][0], u = p[ax][0];
#pragma unroll
            for (int k = 1; k < NC; ++k) {
                l = fmin(l, p[ax][k]);
                u = fmax(u, p[ax][k]);
            }
            if (pieces == 0) {
                lo[ax] = l; hi[ax] = u; G[ax] = g;
                left[ax] = p[ax][0];
            } else {
                lo[ax] = fmin(lo[ax], l);
                hi[ax] = fmax(hi[ax], u);
                G[ax] = g > G[ax] || g != g ? g : G[ax];   // (a NaN stays)
            }
        }
        ++pieces;
    }
};

// (v, p, w) <- the smaller of it and (ov, op, ow): by value, a tie by partner, then by index
__device__ __forceinline__ void sep_take(double& v, int& p, int& w, double ov, int op, int ow) {
    if (ov < v || (ov == v && (op < p || (op == p && ow < w)))) {
        v = ov; p = op; w = ow;
    }
}

template <int R>
__global__ __launch_bounds__(SEP_BLOCK) void separation_cert_kernel(SeparationCertArgs a) {
    constexpr int NC = 2 * R, E = SEP_ENTRIES;
    __shared__ double sh_c[3 * NC][E];   // single: the coefficients [axis][k]; box: [axis][0..3] = lo, hi, left end, right end
    __shared__ double sh_G[3][E];
    __shared__ double sh_L[E], sh_U[E];
    __shared__ int sh_kind[E], sh_pl[E], sh_pu[E];   // sh_pu: partner * 2 + (0 left end, 1 right end), -1 none
    __shared__ int sh_live[SEP_BLOCK], sh_word[SEP_BLOCK];
    const int tid = threadIdx.x;
    const int NL = a.n_leaves;

    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int b0 = a.group_offsets ? a.group_offsets[g] : 0;
        const int A_all = (a.group_offsets ? a.group_offsets[g + 1] : a.n_traj) - b0;
        if (A_all > SWARM_MAX) {   // an oversize swarm is not evaluated
            for (int i = tid; i < A_all; i += SEP_BLOCK) {
                const int b = b0 + i;
                if (a.lower) a.lower[b] = NAN;
                if (a.upper) a.upper[b] = NAN;
                if (a.where) {
                    a.where[(size_t)b * 4] = -1; a.where[(size_t)b * 4 + 1] = 0;
                    a.where[(size_t)b * 4 + 2] = -1; a.where[(size_t)b * 4 + 3] = 0;
                }
                if (a.verdict) a.verdict[b] = 0;
            }
            if (tid == 0 && a.group_verdict) a.group_verdict[g] = 0;
            continue;
        }
        const int A = A_all > 0 ? A_all : 0;

        // lane i owns vehicle i for the whole swarm
        const bool mine = tid < A;
        const int b = b0 + (mine ? tid : 0);
        const PolySpan sp = mine ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const bool live = mine && sp.M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        bool moving = false;   // still under way at the end of the window
        if (live) {
            double K = a.start ? a.start[b] : 0.0;
            for (int m = 0; m < sp.M; ++m) K += a.times[sp.s0 + m];
            moving = K > fma((double)NL, a.h, a.clock_start);
        }
        __syncthreads();   // (the previous swarm's lane 0 has read sh_word)
        if (mine) sh_live[tid] = live ? 1 : 0;

        double Lm = INFINITY, Um = INFINITY;
        int Lp = -1, Ll = 0, Up = -1, Uw = 0;
        bool bad = false;

        const int TL = A > 0 ? E / A : E;   // leaves per tile (A <= SWARM_MAX <= E: at least one)
        for (int l_lo = 0; l_lo < NL; l_lo += TL) {
            const int l_n = NL - l_lo < TL ? NL - l_lo : TL;
            const int n_ent = l_n * A;
            __syncthreads();   // sh_live is set; the previous tile has been consumed

            // ---- phase 1: each (vehicle, leaf) located and restricted once
            for (int e = tid; e < n_ent; e += SEP_BLOCK) {
                const int i = e % A, leaf = l_lo + e / A;
                if (!sh_live[i]) continue;
                const int bi = b0 + i;
                const auto [si, Mi] = poly_span(a.uniform, a.seg_offsets, bi);
                const double* T = a.times + si;
                const double* c = a.coeff + (size_t)3 * NC * si;
                const size_t axs = (size_t)NC * Mi;
                const double ta = fma((double)leaf, a.h, a.clock_start), tb = fma((double)(leaf + 1), a.h, a.clock_start);
                double K = a.start ? a.start[bi] : 0.0;
                SepEntry<NC> en;
                bool single = false;
                if (tb <= K) {   // waiting throughout
                    en.add(c, axs, T[0], fmax(fabs(K), fabs(K + T[0])) / T[0], 0.0, 0.0);
                    single = true;
                } else {
                    double Tm = 0.0, Kp = K;
                    for (int m = 0; m < Mi && K <= tb; ++m) {
                        Tm = T[m];
                        const double Kn = K + Tm;
                        if (Kn > ta || (Kn == ta && m < Mi - 1)) {   // (K_M = tau_l: arrived, below)
                            single = K <= ta && tb <= Kn;
                            if (single) en.pieces = 0;   // the leaf lies in this piece: a piece that only touched its left end is dropped
                            const double la = fmax(ta - K, 0.0), lb = fmin(tb - K, Tm);
                            en.add(c + (size_t)m * NC, axs, Tm, fmax(fabs(K), fabs(Kn)) / Tm, sep_ratio(lb / Tm), sep_ratio(la / lb));
                            if (single) break;
                        }
                        Kp = K;
                        K = Kn;
                    }
                    if (en.pieces == 0) {   // arrived throughout (the walk went through every segment: Kp = K_{M-1}, K = K_M <= ta)
                        en.add(c + (size_t)(Mi - 1) * NC, axs, Tm, fmax(fabs(Kp), fabs(K)) / Tm, 1.0, 1.0);
                        single = true;
                    }
                }
                sh_kind[e] = single ? SEP_SINGLE : SEP_BOX;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    sh_G[ax][e] = en.G[ax];
                    if (single) {
#pragma unroll
                        for (int k = 0; k < NC; ++k) sh_c[ax * NC + k][e] = en.p[ax][k];
                    } else {
                        sh_c[ax * NC][e] = en.lo[ax];
                        sh_c[ax * NC + 1][e] = en.hi[ax];
                        sh_c[ax * NC + 2][e] = en.left[ax];
                        sh_c[ax * NC + 3][e] = en.p[ax][NC - 1];
                    }
                }
            }
            __syncthreads();

            // ---- phase 2: pairs, from LDS alone
            for (int e = tid; e < n_ent; e += SEP_BLOCK) {
                const int i = e % A, row = e - i, leaf = l_lo + e / A;
                double Lv = INFINITY, Uv = INFINITY;
                int pl = -1, pu = -1;
                bool nan = false;
                if (sh_live[i]) {
                    const bool single_i = sh_kind[e] == SEP_SINGLE;
                    double ci[3][NC], Gi[3], lo_i[3], hi_i[3], left_i[3], right_i[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        Gi[ax] = sh_G[ax][e];
                        // (a box entry has four doubles per axis: the rest of its slots is never read)
#pragma unroll
                        for (int k = 0; k < NC; ++k) ci[ax][k] = single_i || k < 4 ? sh_c[ax * NC + k][e] : 0.0;
                        double l = ci[ax][0], u = ci[ax][0];
#pragma unroll
                        for (int k = 1; k < NC; ++k) {
                            l = fmin(l, ci[ax][k]);
                            u = fmax(u, ci[ax][k]);
                        }
                        lo_i[ax] = single_i ? l : ci[ax][0];
                        hi_i[ax] = single_i ? u : ci[ax][1];
                        left_i[ax] = single_i ? ci[ax][0] : ci[ax][2];
                        right_i[ax] = single_i ? ci[ax][NC - 1] : ci[ax][3];
                    }
                    for (int j = 0; j < A; ++j) {
                        if (j == i || !sh_live[j]) continue;
                        const int ej = row + j;
                        const bool single_j = sh_kind[ej] == SEP_SINGLE;
                        double gn[3], mag = 0.0, dl[3], dr[3], Gmax = 0.0;
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const double Gs = Gi[ax] + sh_G[ax][ej];
                            Gmax = Gs > Gmax || Gs != Gs ? Gs : Gmax;
                            double lo, hi;
                            if (single_i && single_j) {
                                lo = hi = ci[ax][0] - sh_c[ax * NC][ej];
#pragma unroll
                                for (int k = 1; k < NC; ++k) {
                                    const double d = ci[ax][k] - sh_c[ax * NC + k][ej];
                                    lo = fmin(lo, d);
                                    hi = fmax(hi, d);
                                }
                                dl[ax] = left_i[ax] - sh_c[ax * NC][ej];
                                dr[ax] = right_i[ax] - sh_c[ax * NC + NC - 1][ej];
                            } else {
                                double lo_j = sh_c[ax * NC][ej], hi_j = lo_j;
                                if (single_j) {
#pragma unroll
                                    for (int k = 1; k < NC; ++k) {
                                        const double v = sh_c[ax * NC + k][ej];
                                        lo_j = fmin(lo_j, v);
                                        hi_j = fmax(hi_j, v);
                                    }
                                } else {
                                    hi_j = sh_c[ax * NC + 1][ej];
                                }
                                lo = lo_i[ax] - hi_j;
                                hi = hi_i[ax] - lo_j;
                                dl[ax] = left_i[ax] - sh_c[ax * NC + (single_j ? 0 : 2)][ej];
                                dr[ax] = right_i[ax] - sh_c[ax * NC + (single_j ? NC - 1 : 3)][ej];
                            }
                            lo -= Gs;
                            hi += Gs;
                            gn[ax] = fmax(0.0, fmax(lo, -hi));
                            mag += fmax(fabs(lo), fabs(hi));
                        }
                        if (!(Gmax < INFINITY)) {   // (a NaN too)
                            nan = true;
                            continue;
                        }
                        const double gz = gn[2] * a.inv_dw;
                        const double Lj = sqrt(fma(gn[0], gn[0], fma(gn[1], gn[1], gz * gz))) - 16.0 * ENV_EPS * mag;
                        if (Lj < Lv) {
                            Lv = Lj;
                            pl = j;
                        }
                        const double pad = SEP_SQRT3 * Gmax;
                        const double zl = dl[2] * a.inv_dw;
                        const double Ul = sqrt(fma(dl[0], dl[0], fma(dl[1], dl[1], zl * zl))) + pad +
                                          16.0 * ENV_EPS * (fabs(dl[0]) + fabs(dl[1]) + fabs(dl[2]));
                        if (Ul < Uv) {
                            Uv = Ul;
                            pu = j * 2;
                        }
                        if (leaf == NL - 1) {
                            const double zr = dr[2] * a.inv_dw;
                            const double Ur = sqrt(fma(dr[0], dr[0], fma(dr[1], dr[1], zr * zr))) + pad +
                                              16.0 * ENV_EPS * (fabs(dr[0]) + fabs(dr[1]) + fabs(dr[2]));
                            if (Ur < Uv) {
                                Uv = Ur;
                                pu = j * 2 + 1;
                            }
                        }
                    }
                }
                sh_L[e] = nan ? NAN : Lv;
                sh_U[e] = Uv;
                sh_pl[e] = pl;
                sh_pu[e] = pu;
            }
            __syncthreads();

            // ---- phase 3: lane i folds vehicle i's leaves of the tile, in rising order
            if (live) {
                for (int k = 0; k < l_n; ++k) {
                    const int e = k * A + tid;
                    const double Lv = sh_L[e];
                    bad = bad || Lv != Lv;
                    const int pl = sh_pl[e], pu = sh_pu[e];
                    if (pl >= 0) sep_take(Lm, Lp, Ll, Lv, pl, l_lo + k);
                    if (pu >= 0) sep_take(Um, Up, Uw, sh_U[e], pu >> 1, l_lo + k + (pu & 1));
                }
            }
        }

        // ---- the per-vehicle outputs and the swarm's word
        if (mine) {
            int word = 0;
            double lower = INFINITY, upper = INFINITY;
            if (live) {
                lower = bad ? NAN : (Lp >= 0 ? fmax(0.0, Lm) : INFINITY);
                upper = bad ? NAN : Um;
                if (bad) Lp = Up = -1;
                word = bad ? 0
                           : (lower >= a.d_req ? UAVQP_SEPARATION_CERTIFIED : 0) | (upper < a.d_req ? UAVQP_SEPARATION_VIOLATED : 0) |
                                 (moving ? UAVQP_SEPARATION_MOVING : 0);
            }
            if (a.lower) a.lower[b] = lower;
            if (a.upper) a.upper[b] = upper;
            if (a.where) {
                a.where[(size_t)b * 4] = Lp >= 0 ? b0 + Lp : -1;
                a.where[(size_t)b * 4 + 1] = Lp >= 0 ? Ll : 0;
                a.where[(size_t)b * 4 + 2] = Up >= 0 ? b0 + Up : -1;
                a.where[(size_t)b * 4 + 3] = Up >= 0 ? Uw : 0;
            }
            if (a.verdict) a.verdict[b] = word;
            sh_word[tid] = live ? word : -1;
        }
        __syncthreads();
        if (tid == 0 && a.group_verdict) {
            int cert = UAVQP_SEPARATION_CERTIFIED, other = 0, n = 0;
            for (int i = 0; i < A; ++i) {
                const int w = sh_word[i];
                if (w < 0) continue;   // takes no part
                cert &= w;
                other |= w;
                ++n;
            }
            a.group_verdict[g] = n ? (cert | (other & (UAVQP_SEPARATION_VIOLATED | UAVQP_SEPARATION_MOVING))) : 0;
        }
    }
}

}  // namespace uavqp
