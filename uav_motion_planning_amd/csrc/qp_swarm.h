// qp_swarm.h -- the separation penalty between the vehicles of a swarm on a shared clock, with its gradients in the coefficients, the
// durations and the departure times (uavqp_swarm_penalty_device, include/uavqp.h: the definition, the formulas and the rules are there).
//
// Work.  One workgroup of SWARM_BLOCK = SWARM_MAX lanes takes one swarm of A vehicles (grid-stride over the swarms) and walks the N + 1
// clock samples in tiles of TS = SWARM_ENTRIES / A samples, from the LAST sample to the first.  Per tile, three phases over LDS:
//   1. locate + evaluate: one lane per (vehicle, sample) applies the segment rule of qp_poly.h once, caps it at the two holds, and leaves
//      position, velocity, segment, local time and hold state in LDS.  Nothing after this phase touches times or coefficients.
//   2. pairs: one lane per (vehicle i, sample k) runs over its partners j = 0..A-1 in LDS (lanes of a wave share k, so a partner's
//      position is one broadcast read) and leaves the force G_ik, phi_ik = sum_{j > i} x^3 and min_j rho2 in LDS.
//   3. accumulate: lane i owns vehicle i.  It consumes its samples in falling k with the 3 x 2r partial sums of the CURRENT segment, W of
//      that segment and the running sum of W over the later segments in registers.  Falling k visits the segments in falling order, so
//      when the vehicle leaves segment l, sum_{m > l} W_m is complete: the lane stores grad_coeff and grad_times of l once and moves
//      on (segments without a contributing sample in between get their zeros then).  The state lives in registers ACROSS tiles: that is
//      why the lane owns the vehicle, not a (vehicle, segment) pair -- a pair's samples may straddle tiles, a vehicle's segment only
//      ever falls.  Samples whose force is zero (most of them) cost one LDS read.
// After the last tile the lane stores what is left, grad_start and min_sep; lane 0 adds the vehicles' phi_i in index order.
// Order of the additions: j within a sample, k within a vehicle, i within the swarm -- indices within the swarm alone, none of them a
// function of TS, the grid or the swarm's place in the batch: the same bytes run to run, alone or inside a batch.
// A vehicle that is not solved (or has M < 1) is skipped by every pair loop and stores zeros / INFINITY.  A swarm of more than SWARM_MAX
// vehicles (the _host entry refuses it; offsets on the device are trusted) is not evaluated: Phi = NaN, zeros elsewhere, nothing in LDS.
//
// LDS.  12 doubles + 1 int per entry, SWARM_ENTRIES = 256 entries, SWARM_MAX doubles for phi_i and SWARM_MAX ints: 27136 bytes per
// workgroup, TS = 2 at A = 128, 32 at A = 8.  Phase 2 reads [field][k * A + j], the same j in every lane: one address per sample row
// (a broadcast); phase 3 reads [field][k * A + i], consecutive lanes consecutive doubles.
// Resources (gfx950, `make resource-usage`): swarm_penalty_kernel<3> 138 VGPRs, <4> 133 VGPRs, 106 SGPRs, no scratch, LDS 27136 bytes
// per workgroup, occupancy 3 waves per SIMD by the registers; the LDS admits 5 workgroups of 2 waves per CU, which is what the launch
// caps its grid at (uavqp_swarm.h).
// Measured and not kept (docs/measurement_log.md): a tile sized by the host so that a swarm of the batch's mean size takes ONE tile, with
// every duration read up front in phase 1 -- 65.3 us against 58.6 us per launch on 512 swarms x 8 vehicles x 65 samples.  The time is
// not in the number of tiles but in the few lanes a small swarm gives phases 1 and 3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_poly.h"

namespace uavqp {

constexpr int SWARM_MAX = UAVQP_SWARM_MAX_VEHICLES;   // largest swarm; one lane per vehicle in phase 3
constexpr int SWARM_BLOCK = SWARM_MAX;
constexpr int SWARM_ENTRIES = 256;                    // (vehicle, sample) entries of one tile: two samples of the largest swarm

struct SwarmArgs {
    int n_traj, uniform, n_groups;
    const int32_t* seg_offsets;
    const int32_t* group_offsets;   // null: one swarm, the whole batch
    const double* times;
    const double* coeff;
    const int32_t* status;          // null: every trajectory counts as solved
    const double* start;            // null: all zero
    double* penalty;                // [n_groups] or null
    double* grad_coeff;             // layout of coeff, or null
    double* grad_times;             // [sum M] or null
    double* grad_start;             // [n_traj] or null
    double* min_sep;                // [n_traj] or null
    int N;                          // n_samples: N + 1 clock samples
    double clock_start, dt, d_safe;
    double inv_d2;                  // 1 / d_safe^2
    double inv_dw2;                 // 1 / downwash^2
    double weight;
    double force;                   // -6 weight / d_safe^2
};

enum : int { SWARM_MOVING = 0, SWARM_WAITING = 1, SWARM_ARRIVED = 2 };

// grad_coeff and grad_times of segment l of a vehicle (gc, W: the sums of the samples it owns; tail = sum_{m > l} W_m; P: the arrived samples)
// ACC (internal, the swarm optimiser of uavqp_swarm_opt.h): ADD to what another penalty has left in the two arrays.  Every element has this
// one owning lane, so the sum is race-free and its order fixed.  `any`: a sample has added to gc -- most segments of a flight see no
// partner, and adding their zeros would be a read and a write of 3 x 2r doubles for nothing (x + 0 is x: the bytes are the same).
template <int NC, bool ACC>
__device__ __forceinline__ void swarm_store_segment(const SwarmArgs& a, size_t base, size_t axs, int s0, int l, int M, const double (&gc)[3][NC],
                                                    double tail, double P, bool any) {
    if (a.grad_coeff && (!ACC || any)) {
        double* at = a.grad_coeff + base + (size_t)l * NC;
        double old[3][NC];
        if (ACC)   // (all loads before the first store: the compiler cannot know that the two do not overlap)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int n = 0; n < NC; ++n) old[ax][n] = at[(size_t)ax * axs + n];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
            for (int n = 0; n < NC; ++n) at[(size_t)ax * axs + n] = ACC ? old[ax][n] + a.dt * gc[ax][n] : a.dt * gc[ax][n];
    }
    if (a.grad_times) {
        const double gt = l == M - 1 ? fma(a.dt, P, 0.0 - a.dt * tail) : 0.0 - a.dt * tail;   // (0 - x: never -0.0)
        if (!ACC) a.grad_times[s0 + l] = gt;
        else if (gt != 0.0) a.grad_times[s0 + l] += gt;
    }
}

template <int R, bool ACC = false>
__global__ __launch_bounds__(SWARM_BLOCK) void swarm_penalty_kernel(SwarmArgs a) {
    constexpr int NC = 2 * R, E = SWARM_ENTRIES;
    __shared__ double sh_q[3][E], sh_v[3][E], sh_G[3][E], sh_t[E], sh_phi[E], sh_rho[E];
    __shared__ int sh_seg[E];            // segment * 4 + hold state
    __shared__ double sh_sum[SWARM_MAX]; // phi_i
    __shared__ int sh_live[SWARM_MAX];
    const int tid = threadIdx.x;

    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int b0 = a.group_offsets ? a.group_offsets[g] : 0;
        const int A_all = (a.group_offsets ? a.group_offsets[g + 1] : a.n_traj) - b0;
        const bool fits = A_all <= SWARM_MAX;
        const int A = fits ? A_all : 0;   // an oversize swarm is not evaluated

        if (!fits) {
            // zeros for every vehicle of the oversize swarm, NaN for its penalty
            for (int i = tid; i < A_all; i += SWARM_BLOCK) {
                const int b = b0 + i;
                const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
                const size_t n_c = (size_t)3 * NC * (M > 0 ? M : 0), base = (size_t)3 * NC * s0;
                if (!ACC && a.grad_coeff)   // (ACC: adding zero leaves what is there)
                    for (size_t n = 0; n < n_c; ++n) a.grad_coeff[base + n] = 0.0;
                if (!ACC && a.grad_times)
                    for (int l = 0; l < M; ++l) a.grad_times[s0 + l] = 0.0;
                if (a.grad_start) a.grad_start[b] = 0.0;
                if (a.min_sep) a.min_sep[b] = INFINITY;
            }
            if (tid == 0 && a.penalty) a.penalty[g] = NAN;
            continue;
        }

        // lane i owns vehicle i for the whole swarm
        const bool mine = tid < A;
        const int b = b0 + (mine ? tid : 0);
        PolySpan sp = mine ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const int s0 = sp.s0, M = sp.M;
        const bool live = mine && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        const size_t axs = (size_t)NC * (M > 0 ? M : 0), base = (size_t)3 * NC * s0;
        __syncthreads();   // (the previous swarm's lane 0 has read sh_sum)
        if (mine) sh_live[tid] = live ? 1 : 0;

        double gc[3][NC];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
            for (int n = 0; n < NC; ++n) gc[ax][n] = 0.0;
        int cur = M - 1;                       // the segment whose sums the registers hold
        double W = 0.0, tail = 0.0, P = 0.0;   // W of cur, sum of W over the segments behind it, the arrived samples
        bool any = false;                      // a sample has added to gc of cur
        double phi_i = 0.0, rho_i = INFINITY;

        const int TS = A > 0 ? E / A : E;      // samples per tile (A <= SWARM_MAX <= E: at least one)
        for (int k_hi = a.N; k_hi >= 0; k_hi -= TS) {
            const int k_lo = k_hi - TS + 1 > 0 ? k_hi - TS + 1 : 0;
            const int n_ent = (k_hi - k_lo + 1) * A;
            __syncthreads();   // sh_live is set; the previous tile has been consumed

            // ---- phase 1: each (vehicle, sample) located and evaluated once
            for (int e = tid; e < n_ent; e += SWARM_BLOCK) {
                const int i = e % A, k = k_lo + e / A;
                if (!sh_live[i]) continue;
                const int bi = b0 + i;
                const auto [si, Mi] = poly_span(a.uniform, a.seg_offsets, bi);
                const double* T = a.times + si;
                const double u = fma((double)k, a.dt, a.clock_start) - (a.start ? a.start[bi] : 0.0);
                int idx = 0, state = SWARM_WAITING;
                double t = 0.0;
                if (!(u < 0.0)) {
                    const PolySeg ps = poly_segment(T, Mi, u);
                    const double T_last = T[Mi - 1];
                    const bool arrived = ps.past || (ps.idx == Mi - 1 && ps.t >= T_last);
                    idx = arrived ? Mi - 1 : ps.idx;
                    t = arrived ? T_last : ps.t;
                    state = arrived ? SWARM_ARRIVED : SWARM_MOVING;
                }
                const double* c = a.coeff + (size_t)3 * NC * si + (size_t)idx * NC;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double* ca = c + (size_t)ax * NC * Mi;
                    sh_q[ax][e] = poly_deriv<NC, 0>(ca, t);
                    sh_v[ax][e] = poly_deriv<NC, 1>(ca, t);
                }
                sh_t[e] = t;
                sh_seg[e] = idx * 4 + state;
            }
            __syncthreads();

            // ---- phase 2: pairs, from LDS alone
            for (int e = tid; e < n_ent; e += SWARM_BLOCK) {
                const int i = e % A, row = e - i;
                double G0 = 0.0, G1 = 0.0, G2 = 0.0, phi = 0.0, rho = INFINITY;
                if (sh_live[i]) {
                    const double qx = sh_q[0][e], qy = sh_q[1][e], qz = sh_q[2][e];
                    for (int j = 0; j < A; ++j) {
                        if (j == i || !sh_live[j]) continue;
                        const double dx = qx - sh_q[0][row + j], dy = qy - sh_q[1][row + j], dz = qz - sh_q[2][row + j];
                        const double rho2 = fma(dx, dx, fma(dy, dy, dz * dz * a.inv_dw2)) * a.inv_d2;
                        rho = fmin(rho, rho2);
                        const double x = fmax(0.0, 1.0 - rho2);
                        if (x > 0.0) {
                            const double f = a.force * (x * x);
                            G0 = fma(f, dx, G0);
                            G1 = fma(f, dy, G1);
                            G2 = fma(f * a.inv_dw2, dz, G2);
                            if (j > i) phi = fma(x, x * x, phi);
                        }
                    }
                }
                sh_G[0][e] = G0; sh_G[1][e] = G1; sh_G[2][e] = G2;
                sh_phi[e] = phi;
                sh_rho[e] = rho;
            }
            __syncthreads();

            // ---- phase 3: lane i consumes vehicle i's samples of the tile, last first
            if (live) {
                for (int k = k_hi; k >= k_lo; --k) {
                    const int e = (k - k_lo) * A + tid;
                    const double om = (k == 0 || k == a.N) ? 0.5 : 1.0;
                    phi_i = fma(om, sh_phi[e], phi_i);
                    rho_i = fmin(rho_i, sh_rho[e]);
                    const double G[3] = {om * sh_G[0][e], om * sh_G[1][e], om * sh_G[2][e]};
                    if (G[0] == 0.0 && G[1] == 0.0 && G[2] == 0.0) continue;
                    const int code = sh_seg[e], seg = code >> 2, state = code & 3;
                    while (cur > seg) {   // the vehicle has left segment cur (going back in time): its sums are complete
                        swarm_store_segment<NC, ACC>(a, base, axs, s0, cur, M, gc, tail, P, any);
                        tail += W;
                        W = 0.0;
                        any = false;
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                            for (int n = 0; n < NC; ++n) gc[ax][n] = 0.0;
                        --cur;
                    }
                    const double t = sh_t[e];
                    const double Gv = fma(G[0], sh_v[0][e], fma(G[1], sh_v[1][e], G[2] * sh_v[2][e]));
                    if (state == SWARM_MOVING) W += Gv;
                    if (state == SWARM_ARRIVED) P += Gv;
                    any = true;
                    double p = 1.0;
#pragma unroll
                    for (int n = 0; n < NC; ++n) {
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) gc[ax][n] = fma(G[ax], p, gc[ax][n]);
                        p *= t;
                    }
                }
            }
        }

        // ---- what the registers still hold, the segments before it, and the per-vehicle outputs
        if (mine) {
            if (!live) W = 0.0;
            while (cur >= 0) {
                swarm_store_segment<NC, ACC>(a, base, axs, s0, cur, M, gc, tail, P, any);
                tail += W;
                W = 0.0;
                any = false;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                    for (int n = 0; n < NC; ++n) gc[ax][n] = 0.0;
                --cur;
            }
            if (a.grad_start) a.grad_start[b] = 0.0 - a.dt * tail;
            if (a.min_sep) a.min_sep[b] = a.d_safe * sqrt(rho_i);
            sh_sum[tid] = phi_i;
        }
        __syncthreads();
        if (tid == 0 && a.penalty) {
            double s = 0.0;
            for (int i = 0; i < A; ++i) s += sh_sum[i];
            a.penalty[g] = a.dt * a.weight * s;
        }
    }
}

}  // namespace uavqp
