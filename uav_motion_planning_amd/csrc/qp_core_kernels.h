// qp_core_kernels.h -- BatchArgs and the kernels that need no solver header of their own: the window sort of the ragged dealing and the
// one-lane generic solve (any segment count).  The kernels that sample a solved trajectory are in qp_samplers.h.
// (Moved out of uavqp.hip in round 6 so that every kernel family can be compiled as its own translation unit: csrc/Makefile.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/uavqp.h"
#include "qp_device.h"

namespace uavqp {

struct BatchArgs {
    int n_traj;
    int uniform;       // > 0: uniform segment count
    int max_segments;  // ragged upper bound
    const int32_t* seg_offsets;
    const double* waypoints;
    const double* times;
    const double* bc;
    double* coeff;
    int32_t* status;
    double* ws;     // forward-sweep workspace (generic kernel)
    const int32_t* perm;  // ragged dealing (generic kernel, LSORT): lane slot -> trajectory
    const int4* perm4;    // the same with the trajectory's first segment and segment count packed in: {b, s0, M, 0} (pair kernel: one
                          // load instead of three dependent ones at the top of the wave)
    int fused_sort;       // pair kernel, LSORT (round 6): no window_sort_kernel launch -- every wave sorts its window's 512 segment counts itself (qp_generic2.h)
    double* dummy;  // 1 KiB sink for the predicated-off stores of the specialised kernel
#ifdef UAVQP_PHASE_TIMING
    long long* stamps;  // debug: s_memtime stamps of wave 0 (tools/ubench only)
#endif
};

// ---------------------------------------------------------------------------------------------------
// Generic kernel: any segment count (ragged batches), r = 3 or 4.
// Forward block elimination keeps E_k = S_k^-1 A01(k) and h_k = S_k^-1 z_k per interior knot in a
// HBM workspace  ws[wave][k-1][f][lane]  (every access a coalesced 512-byte row of the wave),
// the backward sweep re-reads them and emits segment coefficients as it goes.
//
// NAX = 3: one lane per trajectory carries all three axes (the factorisation is shared).
// NAX = 1: one lane per (trajectory, axis), 21 trajectories per wave: the 3 lanes of a trajectory repeat the (cheap)
//          matrix elimination, each carries one right-hand side and emits one axis.  Three times the waves and a
//          third of the per-lane state -- for batches that do not fill the machine with one lane per trajectory.
//          E_k is stored once per trajectory (by the x lane, in its own slot) and read by all three lanes from that
//          slot: same wave, program order, so the hand-off needs no fence.
// ---------------------------------------------------------------------------------------------------
// LSORT (ragged batches): every window of 16 x IPW consecutive trajectories (IPW = trajectories per wave: 64 or 21) is
// dealt to 16 consecutive single-wave workgroups by descending segment count -- workgroup q of the group takes ranks
// [IPW q, IPW (q + 1)) -- so that the lanes of one wave run sweeps of nearly equal length while the window stays
// contiguous in memory (a GLOBAL sort by M was measured at 157 -> 244 us on config 4: it destroys the locality the
// strided per-lane accesses live on).  The dealing is a permutation `perm` of the batch, written ONCE per window by
// window_sort_kernel (one workgroup per window, LDS counting sort); the solve kernel only reads it.  The order inside a
// bin is whatever the LDS atomics of that one sort give: it decides WHICH lane solves a trajectory, never the result, and
// since every trajectory index is written to exactly one slot of perm, none can be solved twice or dropped.
template <int WIN>
__global__ __launch_bounds__(256) void window_sort_kernel(const int32_t* __restrict__ seg_offsets, int n_traj, int32_t* __restrict__ perm,
                                                          int4* __restrict__ perm4) {
    constexpr int KPT = (WIN + 255) / 256;  // keys per thread
    __shared__ int s_cnt[256];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int base = blockIdx.x * WIN;
    int key[KPT], off0[KPT], cnt[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int w = j * 256 + tid, t = base + w;
        int Mt = -1;
        off0[j] = 0;
        cnt[j] = 0;
        if (w < WIN && t < n_traj) {
            off0[j] = seg_offsets[t];
            cnt[j] = seg_offsets[t + 1] - off0[j];
            Mt = cnt[j] < 0 ? 0 : (cnt[j] > 255 ? 255 : cnt[j]);
        }
        key[j] = Mt;
    }
    s_cnt[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (key[j] >= 0) atomicAdd(&s_cnt[255 - key[j]], 1);  // bin 0 = longest
    __syncthreads();
    // exclusive prefix over the 256 bins: wave scan + the totals of the waves in front
    const int c = s_cnt[tid];
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int run = incl - c;
    for (int q = 0; q < wv; ++q) run += s_wave[q];
    s_cnt[tid] = run;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (key[j] >= 0) {
            const int pos = atomicAdd(&s_cnt[255 - key[j]], 1);
            perm[base + pos] = base + j * 256 + tid;
            if (perm4) perm4[base + pos] = make_int4(base + j * 256 + tid, off0[j], cnt[j], 0);
        }
}

template <int R, bool LSORT, int NAX>
__global__ __launch_bounds__(64) void solve_generic_kernel(BatchArgs a) {
    constexpr int ND = R - 1, NC = 2 * R, F = ND * ND + NAX * ND;
    constexpr int LPI = 3 / NAX;              // lanes per trajectory
    constexpr int IPW = 64 / LPI;             // trajectories per wave (64 or 21)
    const int lane = threadIdx.x;
    const int ax0 = NAX == 1 ? lane % 3 : 0;
    const int item = lane / LPI;
    const bool lane_used = item < IPW;   // NAX = 1: lane 63 idles
    // workspace [wave][interior knot][field][lane]: a wave's record of one knot is F consecutive 512-byte rows
    const int kmax = a.max_segments > 1 ? a.max_segments - 1 : 1;
    // (no __restrict__: for the x lane ws and wsE are the same address)
    double* ws = a.ws + (size_t)blockIdx.x * kmax * F * 64 + lane;
    const double* wsE = ws - ax0;  // the x lane's slot holds E for the whole trajectory
    constexpr size_t wstride = 64;
    const int n_items = gridDim.x * IPW;  // LSORT: the host rounds the grid to a multiple of 16 (whole windows per round)
    const int n_round = (a.n_traj + n_items - 1) / n_items;
    for (int round = 0; round < n_round; ++round) {
        int b = lane_used ? round * n_items + blockIdx.x * IPW + item : a.n_traj;
        if constexpr (LSORT) {
            if (b < a.n_traj) b = a.perm[b];  // dealt by segment count inside the window (window_sort_kernel)
        }
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
        double* __restrict__ out = a.coeff + (size_t)3 * NC * s0;

        bool ok = (M >= 1) && (a.uniform > 0 || M <= a.max_segments);
        if (ok)
            for (int i = 0; i < M; ++i) ok = ok && (T[i] > 0.0) && (T[i] < INFINITY);
        if (!ok) {
            if (a.status && ax0 == 0) a.status[b] = UAVQP_INVALID_INPUT;
            continue;
        }

        double y0[ND][NAX], yM[ND][NAX];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                y0[d][ax] = bc[d * 3 + ax0 + ax];
                yM[d][ax] = bc[(ND + d) * 3 + ax0 + ax];
            }

        // ---------------- forward elimination over interior knots k = 1..M-1 ----------------
        SegBlocks<R> sa;
        sa.build(T[0]);
        double pb[NAX], dpa[NAX];
#pragma unroll
        for (int ax = 0; ax < NAX; ++ax) {
            pb[ax] = wp[3 + ax0 + ax];
            dpa[ax] = pb[ax] - wp[ax0 + ax];
        }
        double Eprev[ND][ND], hprev[ND][NAX];
        // software prefetch: the loads of step k+1 are issued before the arithmetic of step k (one lane per
        // trajectory has nothing else to hide an HBM round trip per knot behind)
        double Tn = M > 1 ? T[1] : 1.0, pn[NAX];
#pragma unroll
        for (int ax = 0; ax < NAX; ++ax) pn[ax] = M > 1 ? wp[6 + ax0 + ax] : 0.0;
        for (int k = 1; k < M; ++k) {
            const double Tk_ = Tn;
            double pcur[NAX];
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) pcur[ax] = pn[ax];
            if (k + 1 < M) {
                Tn = T[k + 1];
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) pn[ax] = wp[3 * (k + 2) + ax0 + ax];
            }
            SegBlocks<R> sb;
            sb.build(Tk_);
            double dpb[NAX];
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                const double pc = pcur[ax];
                dpb[ax] = pc - pb[ax];
                pb[ax] = pc;
            }
            double S[ND][ND], z[ND][NAX];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
#pragma unroll
                for (int j = 0; j < ND; ++j) S[i][j] = sa.A11[i][j] + sb.A00(i, j);
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) z[i][ax] = sb.gv(i) * dpb[ax] - sa.gw[i] * dpa[ax];
            }
            if (k == 1) {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int j = 0; j < ND; ++j)
#pragma unroll
                        for (int ax = 0; ax < NAX; ++ax) z[i][ax] -= sa.A01[j][i] * y0[j][ax];
            } else {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int j = 0; j < ND; ++j) {
#pragma unroll
                        for (int c = 0; c < ND; ++c) S[i][c] -= sa.A01[j][i] * Eprev[j][c];
#pragma unroll
                        for (int ax = 0; ax < NAX; ++ax) z[i][ax] -= sa.A01[j][i] * hprev[j][ax];
                    }
            }
            if (k == M - 1) {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int j = 0; j < ND; ++j)
#pragma unroll
                        for (int ax = 0; ax < NAX; ++ax) z[i][ax] -= sb.A01[i][j] * yM[j][ax];
            }
            SmallLDL<ND> ldl;
            ldl.factor(S);
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                double col[ND];
#pragma unroll
                for (int i = 0; i < ND; ++i) col[i] = z[i][ax];
                ldl.solve(col);
#pragma unroll
                for (int i = 0; i < ND; ++i) hprev[i][ax] = col[i];
            }
#pragma unroll
            for (int c = 0; c < ND; ++c) {
                double col[ND];
#pragma unroll
                for (int i = 0; i < ND; ++i) col[i] = sb.A01[i][c];
                ldl.solve(col);
#pragma unroll
                for (int i = 0; i < ND; ++i) Eprev[i][c] = col[i];
            }
            double* w = ws + (size_t)(k - 1) * F * wstride;
            if (ax0 == 0) {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int c = 0; c < ND; ++c) w[(size_t)(i * ND + c) * wstride] = Eprev[i][c];
            }
#pragma unroll
            for (int i = 0; i < ND; ++i)
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) w[(size_t)(ND * ND + i * NAX + ax) * wstride] = hprev[i][ax];
            sa = sb;
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) dpa[ax] = dpb[ax];
        }

        // ---------------- backward substitution + coefficient emission ----------------
        double ynext[ND][NAX], pend[NAX];
        bool finite = true;
#pragma unroll
        for (int ax = 0; ax < NAX; ++ax) {
            pend[ax] = wp[3 * M + ax0 + ax];
#pragma unroll
            for (int d = 0; d < ND; ++d) ynext[d][ax] = yM[d][ax];
        }
        // software prefetch of the sweep state of knot k-1 (and of T, waypoint) while knot k is processed
        double wn[F], Tkn = T[M - 1], pkn[NAX];
#pragma unroll
        for (int ax = 0; ax < NAX; ++ax) pkn[ax] = wp[3 * (M - 1) + ax0 + ax];
        auto load_rec = [&](int knot, double (&dst)[F]) {  // interior knot `knot` = 1..M-1
            const size_t off = (size_t)(knot - 1) * F * wstride;
#pragma unroll
            for (int f = 0; f < ND * ND; ++f) dst[f] = wsE[off + (size_t)f * wstride];
#pragma unroll
            for (int f = ND * ND; f < F; ++f) dst[f] = ws[off + (size_t)f * wstride];
        };
        if (M >= 2) load_rec(M - 1, wn);
        for (int k = M - 1; k >= 0; --k) {
            double wc[F];
#pragma unroll
            for (int f = 0; f < F; ++f) wc[f] = wn[f];
            const double Tk = Tkn;
            double pkc[NAX];
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) pkc[ax] = pkn[ax];
            if (k >= 1) {
                Tkn = T[k - 1];
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) pkn[ax] = wp[3 * (k - 1) + ax0 + ax];
                if (k >= 2) load_rec(k - 1, wn);
            }
            double y[ND][NAX];
            if (k == 0) {
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int ax = 0; ax < NAX; ++ax) y[d][ax] = y0[d][ax];
            } else {
#pragma unroll
                for (int i = 0; i < ND; ++i)
#pragma unroll
                    for (int ax = 0; ax < NAX; ++ax) y[i][ax] = wc[ND * ND + i * NAX + ax];
                if (k < M - 1) {
#pragma unroll
                    for (int i = 0; i < ND; ++i)
#pragma unroll
                        for (int c = 0; c < ND; ++c) {
                            const double e = wc[i * ND + c];
#pragma unroll
                            for (int ax = 0; ax < NAX; ++ax) y[i][ax] -= e * ynext[c][ax];
                        }
                }
            }
            const double itk = 1.0 / Tk;
#pragma unroll
            for (int ax = 0; ax < NAX; ++ax) {
                const double pk = pkc[ax];
                double ys[ND], ye[ND], c[NC];
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    ys[d] = y[d][ax];
                    ye[d] = ynext[d][ax];
                }
                segment_coeffs<R>(pk, ys, pend[ax], ye, Tk, itk, c);
                double* o = out + ((size_t)(ax0 + ax) * M + k) * NC;
#pragma unroll
                for (int j = 0; j < NC; ++j) o[j] = c[j];
                finite = finite && (fabs(c[NC - 1]) < INFINITY) && (fabs(c[R]) < INFINITY);
                pend[ax] = pk;
            }
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int ax = 0; ax < NAX; ++ax) ynext[d][ax] = y[d][ax];
        }
        if constexpr (NAX == 1) {  // AND over the three lanes of the trajectory (they took the same branches)
            const int f0 = finite ? 1 : 0, l0 = lane - ax0;
            finite = (__shfl(f0, l0, 64) & __shfl(f0, l0 + 1, 64) & __shfl(f0, l0 + 2, 64)) != 0;
        }
        if (a.status && ax0 == 0) a.status[b] = finite ? UAVQP_SOLVED : UAVQP_NON_FINITE;
    }
}

}  // namespace uavqp
