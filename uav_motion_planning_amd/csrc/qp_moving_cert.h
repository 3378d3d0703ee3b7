// qp_moving_cert.h -- certified continuous-time gap between solved trajectories and MOVING obstacle tracks (uavqp_moving_certificate_device,
// include/uavqp.h): for every segment a LOWER bound of its gap to every obstacle of the trajectory's set that holds for EVERY t of the
// segment's flight, an UPPER bound taken at a reported instant and obstacle, and a three-valued verdict against d_req.  The moving-obstacle
// penalty and its optimiser SAMPLE (d_min_gap); a vehicle and a track that close at 10 m/s move 1.25 m against each other between two of
// the default eight samples of a 1 s segment.  This bounds.
//
// The certified curves.  Trajectory b departs at S = traj_start[b]; its knot clock is the DOUBLES K_0 = S, K_{m+1} = fl(K_m + T_m) (the
// penalty's and the separation certificate's).  At local time s of segment m it is at q_m(s) and the clock shows K_m + s (real arithmetic).
// Obstacle o is the curve of the separation certificate (qp_separation_cert.h) on that clock, with its own knots K^o_0 = start_o,
// K^o_{m+1} = fl(K^o_m + T^o_m): segment 0 at local time 0 for t <= K^o_0 (it waits), segment m at local time t - K^o_m for t in
// [K^o_m, K^o_{m+1}], the last segment at its end for t >= K^o_M (it has arrived).  Pieces are closed: at a knot both values belong to the
// curve.  This is the penalty's obstacle WITHOUT the 1e-4 s of overhang its sampling rule (poly_past_segment) allows.
//     gap_o(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) - radius_o     of q(t) - o(t)
//
// Leaves (tests/moving_cert_reference.py restates all of this in numpy).  n = 2r - 1.  Leaf l = 0..2^depth - 1 of segment m is the local
// time [l, l + 1] T_m / 2^depth; its clock ends are ta = fma(l 2^-depth, T_m, K_m), tb = fma((l + 1) 2^-depth, T_m, K_m), one rounding
// each.  The trajectory over the leaf: the D = 0 Bernstein coefficients of env_bernstein and depth levels of env_split (qp_envelope.h),
// guard G_x = 16 (n + 1) 2^-53 S_x -- the leaf of the clearance certificate.  The obstacle over [ta, tb]: the entry of the separation
// certificate (SepEntry::add, sep_split_left / right, sep_ratio of qp_separation_cert.h, the same walk over the knots): SINGLE when the
// leaf lies in one piece (waiting, arrived, or K^o_m <= ta and tb <= K^o_{m+1}), otherwise BOX over the pieces the leaf meets.  A SINGLE
// entry is Bernstein in the same parameter u in [0, 1] as the leaf's own coefficients, so correlated motion cancels in the difference.
//
// Guard of the obstacle's entry, per axis: G^o_x = (64 (n + 1) + 4 n kappa_o) 2^-53 S_x, the largest over the pieces of the entry, with
// kappa_o = max(|K^o_m|, |K^o_{m+1}|, |ta|, |tb|) / T^o_m; a held obstacle (waiting, arrived) has the separation rule, 2 n kappa with
// kappa = max(|K^o_m|, |K^o_{m+1}|) / T^o_m.  Derivation, in units of 2^-53 S_x.  qp_separation_cert.h accounts for the conversion, the two
// splits and the rounded ratios with under 30 (n + 1) of its 64 (n + 1), and for the part of a piece beyond u = 1 that the ROUNDED knot
// K^o_{m+1} admits with 2 n kappa, kappa <= kappa_o.  New here: ta and tb are rounded, so the instant the kernel pairs with the parameter
// u of the leaf, ta + u (tb - ta), differs from the real one, K_m + (l + u) T_m / 2^depth, by at most delta = 2^-53 max(|ta|, |tb|).  In
// the obstacle's own parameter that is a shift of both ends of the restriction by at most delta / T^o_m <= 2^-53 kappa_o; a coefficient of
// the restricted piece is a blossom value of the segment, which moves by at most n S_x (1 + 2^-53 kappa_o)^(n-1) per unit of either end:
// under 2 n kappa_o while 2^-53 kappa_o < 1e-3.  2 n kappa + 2 n kappa_o <= 4 n kappa_o.  A hold is constant: no shift.
// A rounded end can also put the REAL end on the other side of an obstacle knot than the rounded one (a track may JUMP at a knot).  So
// the walk does not trust an inexact end: mc_clock says whether ta (tb) is exact -- it is for dyadic durations and departures: a
// formation --, an inexact one is taken as the interval [t - 2^-52 |t|, t + 2^-52 |t|], which holds the real end.  Which pieces the
// leaf meets, and whether it lies in ONE, is decided on [ta_lo, tb_hi]; the ratios are still those of [ta, tb], clamped: a piece met
// through the margin alone comes in as its end POINT (the real curve is within delta of it: the shift term above), and the entry is a
// BOX.  Where an obstacle knot lies in the interval of the left (right) end and the leaf is not in one piece, it is open which piece
// the witness instant belongs to: that obstacle gives NO upper bound at that witness (fewer candidates: `upper` stays an upper bound).
// A non-finite guard, or a duration that is not > 0, of the segment or of an obstacle piece one of its leaves meets makes the segment's
// bounds NaN, its `where` {-1, 0, -1, 0} and its word 0.  A NaN duration of the trajectory makes the knot clock NaN: no obstacle can be
// located on it, the walk below ends in its last branch with a zero duration, and every later segment is NaN as well.
//
// Pair (leaf, o), Gs_x = G_x + G^o_x, w the leaf's coefficients:
//   single   lo_x = min_k (w_k - b^o_k), hi_x = max_k
//   box      lo_x = min_k w_k - hi^o_x, hi_x = max_k w_k - lo^o_x
//   lo_x -= Gs_x, hi_x += Gs_x;  g_x = max(0, lo_x, -hi_x);  R = 16 2^-53 sum_x max(|lo_x|, |hi_x|)  (qp_separation_cert.h derives it)
//   L = max(0, sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R) - radius_o
//   witness at the leaf's left end (l), and for the last leaf also at its right end (l + 1): d = the difference of the end coefficients,
//   U = sqrt(d_x^2 + d_y^2 + (d_z / downwash)^2) + sqrt(3) max_x Gs_x + 16 2^-53 (|d_x| + |d_y| + |d_z|) - radius_o
// Per segment: lower = min over obstacles and leaves of L (negative inside a radius), upper = min over obstacles and witnesses of U; a tie
// goes to the smaller obstacle, then the smaller leaf / witness.  Every min is exact: the same bytes for any grid.
//
// Lanes.  The scheme of qp_envelope.h / qp_clearance_cert.h: eight lanes per trajectory walk its segments together (and with them the knot
// clock, every lane the same additions); on a segment lane j takes the dyadic piece named by the top three bits of the leaf index and
// loops over the leaves below it; at depth < 3 lanes repeat a leaf.  Per leaf the lane runs over the obstacles of the set in index order,
// walks the obstacle's knots, restricts it and bounds the pair: the leaf's 3 x 2r coefficients and ONE obstacle entry live in registers,
// every split has constant indices.  The eight lanes' (value, obstacle, index) triples are folded with shuffles by the exact
// lexicographic minimum.  Obstacle data comes through the ordinary load path: the lanes of a group, and all groups that avoid the same
// set, read the same few lines.  One launch, no LDS, no scratch, no workspace, no atomics; every output element is written exactly once.
//
// Out of scope: adaptive subdivision, splitting a leaf at an obstacle's knots (a straddling leaf falls back to a box), a per-obstacle
// cull, the time before departure and after arrival, wiring the verdict into uavqp_moving_optimize_*.
// Registers and what bounds the kernel: DESIGN.md section 5.29.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_envelope.h"
#include "qp_separation_cert.h"

namespace uavqp {

struct MovingCertArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;        // null: every trajectory counts as solved
    // the obstacle batch and who avoids what (uavqp_moving_obstacles)
    int n_obs, o_uniform, n_sets;
    const int32_t* o_seg_offsets;
    const double* o_times;
    const double* o_coeff;
    const double* o_start;        // null: all zero
    const double* o_radius;       // null: all zero
    const int32_t* set_offsets;   // null: one set, the whole obstacle batch
    const int32_t* traj_set;      // null: every trajectory avoids set 0
    const double* traj_start;     // null: all zero
    double* gap;                  // [sum M][2] or null
    int32_t* where;               // [sum M][4] or null
    double* peak;                 // [n_traj][2] or null
    int32_t* seg_verdict;         // [sum M] or null
    int32_t* verdict;             // [n_traj] or null
    int depth;
    double inv_dw;                // 1 / downwash
    double d_req;
};

__device__ __forceinline__ void mc_store_where(int32_t* w, int lp, int ll, int up, int uw) {
    w[0] = lp; w[1] = ll; w[2] = up; w[3] = uw;
}

// fma(x, T, K), and whether that double IS x T + K: a two-product and a two-sum (the intrinsics keep the compiler from contracting them)
// leave the rounding error of the exact sum in sl + pl.  A NaN counts as inexact.
__device__ __forceinline__ double mc_clock(double x, double T, double K, bool& exact) {
    const double t = fma(x, T, K);
    const double ph = __dmul_rn(x, T), pl = fma(x, T, -ph);
    const double s = __dadd_rn(K, ph), bb = __dsub_rn(s, K);
    const double sl = __dadd_rn(__dsub_rn(K, __dsub_rn(s, bb)), __dsub_rn(ph, bb));
    exact = __dadd_rn(sl, pl) == 0.0 && t == s;
    return t;
}

template <int R>
__global__ __launch_bounds__(64) void moving_cert_kernel(MovingCertArgs a) {
    constexpr int NC = 2 * R, M1 = NC - 1, LPT = TOPT_LPT;
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int top = a.depth < 3 ? a.depth : 3, rest = a.depth - top;
    const int piece = sub >> (3 - top);
    const int last = (1 << a.depth) - 1;
    const double inv_leaves = 1.0 / (double)(1 << a.depth);   // (a power of two: l * inv_leaves is exact)
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_lanes; g += stride) {
        // (the shuffles below stay inside a group, whose eight lanes are live together and walk the same segments)
        const int b = (int)(g / LPT);
        const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        const bool lead = sub == 0;
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
        double K = (act && a.traj_start) ? a.traj_start[b] : 0.0;   // the knot clock at the head of segment i
        double pk_lo = INFINITY, pk_hi = INFINITY;
        bool pk_bad = false;
        int cert = UAVQP_MOVING_CERT_CERTIFIED, viol = 0;
        for (int i = 0; i < M; ++i) {
            const size_t seg = (size_t)s0 + i;
            if (!act) {   // not solved: no word; solved without an obstacle: certified
                if (lead) {
                    if (a.gap) a.gap[seg * 2] = a.gap[seg * 2 + 1] = INFINITY;
                    if (a.where) mc_store_where(a.where + seg * 4, -1, 0, -1, 0);
                    if (a.seg_verdict) a.seg_verdict[seg] = solved ? UAVQP_MOVING_CERT_CERTIFIED : 0;
                }
                continue;
            }
            const double T = a.times[seg];
            double p[3][NC], G[3];
            bool bad = !(T > 0.0);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double c[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) c[k] = a.coeff[(size_t)3 * NC * s0 + (size_t)ax * axs + (size_t)i * NC + k];
                G[ax] = 16.0 * (double)NC * ENV_EPS * env_bernstein<NC, 0>(c, T, p[ax]);
            }
            for (int s = top - 1; s >= 0; --s) {
                const bool right = ((piece >> s) & 1) != 0;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) env_split<M1>(p[ax], right);
            }
            double Lm = INFINITY, Um = INFINITY;
            int Lp = -1, Ll = 0, Up = -1, Uw = 0;
            for (int l = 0; l < (1 << rest); ++l) {
                double w[3][NC], lo_i[3], hi_i[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int k = 0; k < NC; ++k) w[ax][k] = p[ax][k];
                for (int s = rest - 1; s >= 0; --s) {
                    const bool right = ((l >> s) & 1) != 0;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) env_split<M1>(w[ax], right);
                }
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    lo_i[ax] = hi_i[ax] = w[ax][0];
#pragma unroll
                    for (int k = 1; k < NC; ++k) {
                        lo_i[ax] = fmin(lo_i[ax], w[ax][k]);
                        hi_i[ax] = fmax(hi_i[ax], w[ax][k]);
                    }
                }
                const int leaf = (piece << rest) | l;
                bool ea, eb;
                const double ta = mc_clock((double)leaf * inv_leaves, T, K, ea), tb = mc_clock((double)(leaf + 1) * inv_leaves, T, K, eb);
                const double tmag = fmax(fabs(ta), fabs(tb));
                // where the REAL ends of the leaf can lie: a rounded end is off by at most half an ulp, under 2^-53 |t|
                const double ma = ea ? 0.0 : 2.0 * ENV_EPS * fabs(ta), mb = eb ? 0.0 : 2.0 * ENV_EPS * fabs(tb);
                const double ta_lo = ta - ma, ta_hi = ta + ma, tb_lo = tb - mb, tb_hi = tb + mb;
                for (int o = o0; o < o1; ++o) {
                    const auto [os0, Mo] = poly_span(a.o_uniform, a.o_seg_offsets, o);
                    if (Mo < 1) continue;   // (a track without a segment is nowhere)
                    const double* To = a.o_times + os0;
                    const double* c = a.o_coeff + (size_t)3 * NC * os0;
                    const size_t oaxs = (size_t)NC * Mo;
                    // ---- locate + restrict: the walk of separation_cert_kernel's phase 1 on the leaf [ta, tb]
                    double Ko = a.o_start ? a.o_start[o] : 0.0;
                    SepEntry<NC> en;
                    bool single = false;
                    bool amb_l = false, amb_r = false;   // a knot lies where the real left / right end can: which piece the witness is in is open
                    if (tb_hi <= Ko) {   // waiting throughout
                        const double T0 = To[0];
                        bad = bad || !(T0 > 0.0);
                        en.add(c, oaxs, T0, fmax(fabs(Ko), fabs(Ko + T0)) / T0, 0.0, 0.0);
                        single = true;
                    } else {
                        double Tm = 0.0, Kp = Ko;
                        for (int m = 0; m < Mo && Ko <= tb_hi; ++m) {
                            Tm = To[m];
                            const double Kn = Ko + Tm;
                            amb_l = amb_l || (!ea && ((Ko >= ta_lo && Ko <= ta_hi) || (Kn >= ta_lo && Kn <= ta_hi)));
                            amb_r = amb_r || (!eb && ((Ko >= tb_lo && Ko <= tb_hi) || (Kn >= tb_lo && Kn <= tb_hi)));
                            if (Kn > ta_lo || (Kn == ta_lo && m < Mo - 1)) {   // (K_M = ta: arrived, below)
                                single = Ko <= ta_lo && tb_hi <= Kn;
                                if (single) en.pieces = 0;   // the leaf lies in this piece: one that only touched its left end is dropped
                                const double la = fmax(ta - Ko, 0.0), lb = fmin(tb - Ko, Tm);
                                bad = bad || !(Tm > 0.0);
                                // (twice kappa_o: SepEntry::add takes 2 n of what it is given, the header asks for 4 n kappa_o)
                                en.add(c + (size_t)m * NC, oaxs, Tm, 2.0 * (fmax(fmax(fabs(Ko), fabs(Kn)), tmag) / Tm), sep_ratio(lb / Tm),
                                       sep_ratio(la / lb));
                                if (single) break;
                            }
                            Kp = Ko;
                            Ko = Kn;
                        }
                        if (en.pieces == 0) {   // arrived throughout (the walk went through every segment: Kp = K_{M-1}, Ko = K_M <= ta)
                            bad = bad || !(Tm > 0.0);
                            en.add(c + (size_t)(Mo - 1) * NC, oaxs, Tm, fmax(fabs(Kp), fabs(Ko)) / Tm, 1.0, 1.0);
                            single = true;
                        }
                        if (single) amb_l = amb_r = false;   // the whole real leaf lies in the one closed piece: its ends are values of the curve
                    }
                    // ---- the pair
                    double gn[3], mag = 0.0, dl[3], dr[3], Gmax = 0.0;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double Gs = G[ax] + en.G[ax];
                        Gmax = Gs > Gmax || Gs != Gs ? Gs : Gmax;   // (a NaN stays)
                        double lo, hi;
                        if (single) {
                            lo = hi = w[ax][0] - en.p[ax][0];
#pragma unroll
                            for (int k = 1; k < NC; ++k) {
                                const double d = w[ax][k] - en.p[ax][k];
                                lo = fmin(lo, d);
                                hi = fmax(hi, d);
                            }
                        } else {
                            lo = lo_i[ax] - en.hi[ax];
                            hi = hi_i[ax] - en.lo[ax];
                        }
                        dl[ax] = w[ax][0] - en.left[ax];
                        dr[ax] = w[ax][M1] - en.p[ax][M1];
                        lo -= Gs;
                        hi += Gs;
                        gn[ax] = fmax(0.0, fmax(lo, -hi));
                        mag += fmax(fabs(lo), fabs(hi));
                    }
                    if (!(Gmax < INFINITY)) {   // (a NaN too)
                        bad = true;
                        continue;
                    }
                    const double rad = a.o_radius ? a.o_radius[o] : 0.0;
                    const double gz = gn[2] * a.inv_dw;
                    const double Lo = fmax(0.0, sqrt(fma(gn[0], gn[0], fma(gn[1], gn[1], gz * gz))) - 16.0 * ENV_EPS * mag) - rad;
                    sep_take(Lm, Lp, Ll, Lo, o, leaf);
                    const double pad = SEP_SQRT3 * Gmax;
                    const double zl = dl[2] * a.inv_dw;
                    const double Ul = sqrt(fma(dl[0], dl[0], fma(dl[1], dl[1], zl * zl))) + pad +
                                      16.0 * ENV_EPS * (fabs(dl[0]) + fabs(dl[1]) + fabs(dl[2])) - rad;
                    if (!amb_l) sep_take(Um, Up, Uw, Ul, o, leaf);
                    if (leaf == last && !amb_r) {
                        const double zr = dr[2] * a.inv_dw;
                        const double Ur = sqrt(fma(dr[0], dr[0], fma(dr[1], dr[1], zr * zr))) + pad +
                                          16.0 * ENV_EPS * (fabs(dr[0]) + fabs(dr[1]) + fabs(dr[2])) - rad;
                        sep_take(Um, Up, Uw, Ur, o, leaf + 1);
                    }
                }
            }
            K += T;
            // the group's exact lexicographic minima (a lane without a candidate holds (INFINITY, -1, 0) and never wins over one with)
#pragma unroll
            for (int d = 1; d < LPT; d <<= 1) {
                const double ov = __shfl_xor(Lm, d, 64), ou = __shfl_xor(Um, d, 64);
                const int olp = __shfl_xor(Lp, d, 64), oll = __shfl_xor(Ll, d, 64), oup = __shfl_xor(Up, d, 64), ouw = __shfl_xor(Uw, d, 64);
                if (olp >= 0 && Lp < 0) { Lm = ov; Lp = olp; Ll = oll; }
                else if (olp >= 0) sep_take(Lm, Lp, Ll, ov, olp, oll);
                if (oup >= 0 && Up < 0) { Um = ou; Up = oup; Uw = ouw; }
                else if (oup >= 0) sep_take(Um, Up, Uw, ou, oup, ouw);
            }
            bad = topt_group_max(bad ? 1.0 : 0.0) != 0.0;
            const double lower = bad ? NAN : (Lp >= 0 ? Lm : INFINITY), upper = bad ? NAN : (Up >= 0 ? Um : INFINITY);
            const int bits = bad ? 0 : (lower >= a.d_req ? UAVQP_MOVING_CERT_CERTIFIED : 0) | (upper < a.d_req ? UAVQP_MOVING_CERT_VIOLATED : 0);
            cert &= bits;
            viol |= bits;
            pk_bad = pk_bad || bad;
            pk_lo = fmin(pk_lo, lower);
            pk_hi = fmin(pk_hi, upper);
            if (lead) {
                if (a.gap) {
                    a.gap[seg * 2] = lower;
                    a.gap[seg * 2 + 1] = upper;
                }
                if (a.where) mc_store_where(a.where + seg * 4, bad ? -1 : Lp, bad || Lp < 0 ? 0 : Ll, bad ? -1 : Up, bad || Up < 0 ? 0 : Uw);
                if (a.seg_verdict) a.seg_verdict[seg] = bits;
            }
        }
        if (lead) {
            if (a.peak) {
                a.peak[(size_t)b * 2] = pk_bad ? NAN : pk_lo;
                a.peak[(size_t)b * 2 + 1] = pk_bad ? NAN : pk_hi;
            }
            if (a.verdict)
                a.verdict[b] = (!solved || pk_bad) ? 0 : ((cert & UAVQP_MOVING_CERT_CERTIFIED) | (viol & UAVQP_MOVING_CERT_VIOLATED));
        }
    }
}

}  // namespace uavqp
