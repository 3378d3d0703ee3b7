// uavqp_pipeline.h -- BASELINE config 5 as ONE C-ABI call (included at the end of uavqp.hip): host-side sequencing of the entry
// points of include/uavqp.h plus the few small kernels the sequencing needs (counters for the loop control, box repair).
//
//   plain solve -> corridor boxes from the obstacle cloud (robot ellipsoid of KinoAstar::isCollisionFree, kino_astar.cpp:721-758,
//   attitude of that solve) -> at most max_rounds x (corridor-constrained solve, working set carried from round to round + time
//   re-allocation) -> SE(3) collision check of the result against a uniform grid over the cloud -> REPAIR: the boxes only bound the
//   knots and carry the attitude of the first solve, so the check of the final polynomials is the arbiter: the boxes of every
//   trajectory it flags are halved towards the searcher's waypoints (last round: collapsed onto them = the reference's equality
//   problem) and the batch is re-solved, at most repair_rounds times -- or, through uavqp_corridor_pipeline_rows_*, its between-knot hits
//   become position rows of the general-rows solve on a sub-batch (the knot boxes stay; see the rows repair kernels below).
//
// The reference has no such loop (constant 1.0 s per segment, test_minimum_jerk.cpp:65-71; every row an equality,
// minimum_control.cpp:98-125): nothing to mirror, parity is per inner solve (SURVEY.md section 8-a').
// Loop control is data dependent (did any duration change? does anything still collide?).  Per outer round the host needs ONE number:
// the compaction kernel writes it, tagged with the round's sequence number, into a word of pinned host-coherent memory that the host
// polls -- no copy command, no event, no stream stop between rounds.  What the check finds goes into a 64-byte counter block that is
// copied to the pinned page with the call's one stream synchronisation; everything else stays in device buffers.
#pragma once

namespace uavqp {

struct PipeCounters {
    unsigned int changed;        // trajectories whose durations the last re-allocation stretched
    unsigned int hit;            // trajectories the check flags
    unsigned int hit_blocked;    // ... of those: with an interior waypoint the cloud leaves no room around (degenerate box)
    unsigned int hit_repairable; // ... the rest (what a repair round works on)
    unsigned int unsolved;       // trajectories whose status is not UAVQP_SOLVED
    unsigned int gathered;       // rows repair: trajectories that received a row this round (the sub-batch), its segments, its longest
    unsigned int gathered_segments;
    unsigned int gathered_max_m;
    unsigned long long tmax_bits;  // max over trajectories of the total duration (bits of a non-negative double: ordered like integers)
    unsigned int gathered_slot1; // rows repair: some trajectory of the sub-batch uses row slot 1 (else it is packed one row per segment)
    unsigned int rows_kept;      // rows repair: rows in place at the end of the call
    unsigned long long pad2_[2];
};
static_assert(sizeof(PipeCounters) == 64, "counter block is one 64-byte record");

__global__ void pipe_zero_kernel(PipeCounters* c) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *c = PipeCounters{};
}

// head of a pipeline call: the stretch record starts at 1 (optional), the counter block at zero (nothing touches it before the check)
__global__ __launch_bounds__(256) void pipe_begin_kernel(double* __restrict__ scale, int n, PipeCounters* c) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (scale && i < n) scale[i] = 1.0;
    if (i == 0) *c = PipeCounters{};
}

// changed[b] > 0 / status[b] != SOLVED counts (either pointer may be null)
__global__ __launch_bounds__(256) void pipe_count_kernel(const int32_t* __restrict__ changed, const int32_t* __restrict__ status, int n, PipeCounters* c) {
    int nc = 0, nu = 0;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < n; b += gridDim.x * 256) {
        if (changed && changed[b] > 0) ++nc;
        if (status && status[b] != UAVQP_SOLVED) ++nu;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nc += __shfl_xor(nc, d, 64);
        nu += __shfl_xor(nu, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nc) atomicAdd(&c->changed, (unsigned)nc);
        if (nu) atomicAdd(&c->unsolved, (unsigned)nu);
    }
}

// What the check needs per trajectory, in one launch, eight lanes per trajectory (sub-lane j takes segments j, j + 8, ...; three
// xor-shuffles combine): the total duration -> max over the batch (all trajectories are sampled on ONE grid: dt = max total /
// (samples - 1), which the check kernel reads from the counter block -- the host does not wait for it), first_hit = "none", and on the
// first pass roomy[b] (null afterwards: a repair has shrunk the boxes since).  Was: three kernels, a copy and a stream synchronisation.
__global__ __launch_bounds__(256) void pipe_check_prep_kernel(int n, int uniform, const int32_t* __restrict__ seg_offsets, const double* __restrict__ times,
                                                              const double* __restrict__ lo, const double* __restrict__ hi, uint8_t* __restrict__ roomy,
                                                              int32_t* __restrict__ first_hit, int n_samples, PipeCounters* c) {
    constexpr int LPT = 8;
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)n * LPT, stride = (long long)gridDim.x * 256;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;
    double mx = 0.0;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        int s0 = 0, M = 0;
        if (live) {
            if (uniform > 0) { M = uniform; s0 = b * M; } else { s0 = seg_offsets[b]; M = seg_offsets[b + 1] - s0; }
        }
        // (the partial sums of the eight sub-lanes are added in a fixed tree: the same bits on every run; dt only places the samples)
        double t = 0.0;
        for (int i = sub; i < M; i += LPT) t += times[s0 + i];
        int ok = 1;
        if (roomy) {
            const size_t row0 = (size_t)s0 + b;
            for (int i = sub; i < M; i += LPT) {
                if (i == 0) continue;            // interior waypoint rows only
                const double* l = lo + 3 * (row0 + i);
                const double* h = hi + 3 * (row0 + i);
                const double w = fmin(fmin(h[0] - l[0], h[1] - l[1]), h[2] - l[2]);
                ok &= (w > 0.0) ? 1 : 0;
            }
        }
#pragma unroll
        for (int d = 1; d < LPT; d <<= 1) {
            t += __shfl_xor(t, d, 64);
            ok &= __shfl_xor(ok, d, 64);
        }
        if (live && sub == 0) {
            if (roomy) roomy[b] = (uint8_t)ok;
            first_hit[b] = n_samples;
            if (t > mx && t < INFINITY) mx = t;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
    // one atomic per workgroup (2048 waves on one address cost more than the rest of the kernel)
    __shared__ double s_mx[4];
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        mx = fmax(fmax(s_mx[0], s_mx[1]), fmax(s_mx[2], s_mx[3]));
        if (mx > 0.0) atomicMax(&c->tmax_bits, (unsigned long long)__double_as_longlong(mx));
    }
}

// flag[b] = trajectory b collides (first_hit < n_samples) AND is roomy; counts for the host -- with the number of trajectories whose
// status is not UAVQP_SOLVED (status may be null): when no repair follows, this block is the call's summary
__global__ __launch_bounds__(256) void pipe_hits_kernel(int n, const int32_t* __restrict__ first_hit, int n_samples, const uint8_t* __restrict__ roomy,
                                                        uint8_t* __restrict__ flag, const int32_t* __restrict__ status, PipeCounters* c) {
    int nh = 0, nb = 0, nr = 0, nu = 0;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < n; b += gridDim.x * 256) {
        const bool hit = first_hit[b] < n_samples;
        const bool rm = roomy[b] != 0;
        flag[b] = (hit && rm) ? 1 : 0;
        nh += hit;
        nb += hit && !rm;
        nr += hit && rm;
        if (status && status[b] != UAVQP_SOLVED) ++nu;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nh += __shfl_xor(nh, d, 64);
        nb += __shfl_xor(nb, d, 64);
        nr += __shfl_xor(nr, d, 64);
        nu += __shfl_xor(nu, d, 64);
    }
    __shared__ int s_n[4][4];
    if ((threadIdx.x & 63) == 0) {
        int* q = s_n[threadIdx.x >> 6];
        q[0] = nh; q[1] = nb; q[2] = nr; q[3] = nu;
    }
    __syncthreads();
    if (threadIdx.x < 4) {      // one atomic per counter and workgroup
        const int k = threadIdx.x, v = s_n[0][k] + s_n[1][k] + s_n[2][k] + s_n[3][k];
        unsigned int* dst = k == 0 ? &c->hit : k == 1 ? &c->hit_blocked : k == 2 ? &c->hit_repairable : &c->unsolved;
        if (v) atomicAdd(dst, (unsigned)v);
    }
}

// boxes of the flagged trajectories move towards their waypoints: lo <- w - shrink (w - lo), hi <- w + shrink (hi - w)
// (shrink = 0.5 halves them, 0 collapses them onto the waypoint: the reference's equality row).  One wave per trajectory.
__global__ __launch_bounds__(64) void pipe_shrink_kernel(int n, int uniform, const int32_t* __restrict__ seg_offsets, const double* __restrict__ wp,
                                                         double* __restrict__ lo, double* __restrict__ hi, const uint8_t* __restrict__ flag, double shrink) {
    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        if (!flag[b]) continue;
        int s0, M;
        if (uniform > 0) { M = uniform; s0 = b * M; } else { s0 = seg_offsets[b]; M = seg_offsets[b + 1] - s0; }
        const size_t e0 = 3 * ((size_t)s0 + b);
        for (int i = threadIdx.x; i < 3 * (M + 1); i += 64) {
            const double w = wp[e0 + i];
            lo[e0 + i] = w - shrink * (w - lo[e0 + i]);
            hi[e0 + i] = w + shrink * (hi[e0 + i] - w);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Rows repair (uavqp_corridor_pipeline_rows_device): a between-knot hit becomes a position row p_i(tau T_i) in [a - h, a + h] around an
// anchor a pushed out of the cloud, solved by the general-rows solve on a compact sub-batch of the trajectories that got one.
// ---------------------------------------------------------------------------------------------------
constexpr double REPAIR_PUSH_TARGET = 2.0;   // G: the anchor is pushed until its clearance reaches G (docs/measurement_log.md)
constexpr int REPAIR_PUSH_STEPS = 4;         // at most this many pushes per row

struct RepairRowsArgs {
    int n_traj, uniform, n_samples, n_obs;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    double t0, dt;
    const unsigned long long* tmax_bits;   // optional (pipeline): dt = (double with these bits) / (n_samples - 1), as the check forms it
    const uint8_t* flags;                  // [n_traj][n_samples] per-sample verdicts of the check
    const int32_t* first_hit;              // optional: a trajectory with first_hit >= n_samples is skipped without a scan
    const double* obs;
    double robot_r, robot_h, h_max;
    double* row_tau;                       // [segments][2] IN / OUT
    int32_t* row_deriv;                    // [segments][2] IN / OUT
    double* row_lo;                        // [segments][2][3] IN / OUT
    double* row_hi;
    int32_t* new_rows;                     // [n_traj] OUT: rows this call placed
    uint8_t* placed;                       // optional [segments] OUT (bits set, the caller zeroes it): bit j = slot j placed by this call
    int solvable_only;                     // pipeline: no rows for trajectories the rows solve cannot take (M < 2 or M > 63)
};

// clearance g(a) = min over ALL points of |E^-1 (o - a)| (the metric of the check kernels, frame f = b1, b2, b3) and its arg-min (lowest
// index on a tie), across the wave; every lane returns the same pair
__device__ __forceinline__ double repair_clearance(const RepairRowsArgs& a, const double* p, const double* f, double ir, double ih, int& arg) {
    double m = INFINITY;
    int im = 0x7fffffff;
    for (int o = threadIdx.x; o < a.n_obs; o += 64) {
        const double* q = a.obs + (size_t)o * 3;
        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
        const double e1 = (f[0] * dx + f[1] * dy + f[2] * dz) * ir;
        const double e2 = (f[3] * dx + f[4] * dy + f[5] * dz) * ir;
        const double e3 = (f[6] * dx + f[7] * dy + f[8] * dz) * ih;
        const double v = e1 * e1 + e2 * e2 + e3 * e3;
        if (v < m) { m = v; im = o; }       // (o ascends per lane: the first of equal values stays)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(m, d, 64);
        const int oi = __shfl_xor(im, d, 64);
        if (om < m || (om == m && oi < im)) { m = om; im = oi; }
    }
    arg = im;
    return sqrt(m);
}

// One wave per trajectory.  Lane i finds the first colliding run of samples in segment i (M > 64: in passes of 64 segments) and the
// frame at its middle sample; the wave then treats those segments one after the other: the clearance is a min over the whole cloud.
template <int R>
__global__ __launch_bounds__(64) void repair_rows_kernel(RepairRowsArgs a) {
    constexpr int NC = 2 * R;
    const int lane = threadIdx.x;
    const double dt = a.tmax_bits ? __longlong_as_double((long long)*a.tmax_bits) / (double)(a.n_samples - 1) : a.dt;
    const double ir = 1.0 / a.robot_r, ih = 1.0 / a.robot_h;
    for (int b = blockIdx.x; b < a.n_traj; b += gridDim.x) {
        const auto [s0, M] = poly_span(a.uniform, a.seg_offsets, b);
        const bool skip = M < 1 || a.n_samples < 1 || (a.solvable_only && (M < 2 || M > 63)) || (a.first_hit && a.first_hit[b] >= a.n_samples);
        int count = 0;
        if (!skip) {
            const double* T = a.times + s0;
            const uint8_t* fl = a.flags + (size_t)b * a.n_samples;
            for (int i0 = 0; i0 < M; i0 += 64) {
                const int i = i0 + lane;
                int first = -1, last = -1;
                if (i < M) {
                    for (int s = 0; s < a.n_samples; ++s) {
                        const int idx = poly_segment(T, M, a.t0 + s * dt).idx;   // (the rule of the check kernels)
                        if (idx < i) continue;
                        if (idx > i) break;
                        const bool f = fl[s] != 0;
                        if (first < 0) {
                            if (f) first = last = s;
                        } else if (f) {
                            last = s;
                        } else {
                            break;               // the first run is over
                        }
                    }
                }
                const bool want = first >= 0;
                double tau = 0.0, p[3] = {0.0, 0.0, 0.0}, fr[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (want) {
                    const double t = poly_segment(T, M, a.t0 + ((first + last) >> 1) * dt).t;
                    tau = fmin(fmax(t / T[i], 1.0 / 32.0), 31.0 / 32.0);
                    double acc[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double* ca = a.coeff + (size_t)3 * NC * s0 + ((size_t)ax * M + i) * NC;
                        p[ax] = poly_deriv<NC, 0>(ca, t);
                        acc[ax] = poly_deriv<NC, 2>(ca, t);
                    }
                    poly_body_frame(acc, fr, fr + 3, fr + 6);   // (as in the check kernels)
                }
                unsigned long long todo = __ballot(want);
                while (todo) {
                    const int j = __builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    double q[3], f[9];
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[c] = __shfl(p[c], j, 64);
#pragma unroll
                    for (int c = 0; c < 9; ++c) f[c] = __shfl(fr[c], j, 64);
                    // push-out: radially away from the nearest point (in the metric) until the clearance reaches G
                    int arg = 0;
                    double g = repair_clearance(a, q, f, ir, ih, arg);
                    for (int k = 0; k < REPAIR_PUSH_STEPS && g < REPAIR_PUSH_TARGET && g > 0.0; ++k) {
                        const double* o = a.obs + (size_t)arg * 3;
                        const double sc = REPAIR_PUSH_TARGET / g;
#pragma unroll
                        for (int c = 0; c < 3; ++c) q[c] = o[c] + (q[c] - o[c]) * sc;
                        g = repair_clearance(a, q, f, ir, ih, arg);
                    }
                    if (lane == j && g > 1.0) {
                        const size_t sg = (size_t)s0 + i;
                        int slot = -1;
                        if (a.row_deriv[2 * sg] < 0) slot = 0;
                        else if (a.row_deriv[2 * sg + 1] < 0 && fabs(tau - a.row_tau[2 * sg]) > 1.0 / 32.0) slot = 1;
                        if (slot >= 0) {
                            const size_t rw = 2 * sg + slot;
                            a.row_tau[rw] = tau;
                            a.row_deriv[rw] = 0;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                // |E^-1 e_c|^2 = Q_cc: the half-widths of uavqp_corridor_from_cloud_device around the anchor
                                const double qcc = (f[c] * f[c] + f[3 + c] * f[3 + c]) * ir * ir + f[6 + c] * f[6 + c] * ih * ih;
                                double h = (g - 1.0) / (3.0 * sqrt(qcc));
                                h = h < a.h_max ? h : a.h_max;
                                a.row_lo[3 * rw + c] = q[c] - h;
                                a.row_hi[3 * rw + c] = q[c] + h;
                            }
                            if (a.placed) a.placed[sg] |= (uint8_t)(1u << slot);
                            ++count;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d, 64);
        if (lane == 0) a.new_rows[b] = count;
    }
}

// every row slot unused (deriv -1, zero tau and bounds)
__global__ __launch_bounds__(256) void pipe_rows_clear_kernel(long long n_slots, double* __restrict__ tau, int32_t* __restrict__ deriv,
                                                             double* __restrict__ lo, double* __restrict__ hi) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n_slots; k += (long long)gridDim.x * 256) {
        tau[k] = 0.0;
        deriv[k] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[3 * k + c] = 0.0; hi[3 * k + c] = 0.0; }
    }
}

// The trajectories with new_rows > 0, in index order: list[k], the exclusive prefix of their segment counts (the sub-batch's CSR offsets,
// sub_off[count] = its segments) -> the counter block (gathered, gathered_segments, gathered_max_m, gathered_slot1).  One workgroup.
__global__ __launch_bounds__(1024) void pipe_rows_compact_kernel(int n, int uniform, const int32_t* __restrict__ seg_offsets,
                                                                 const int32_t* __restrict__ new_rows, const int32_t* __restrict__ deriv,
                                                                 int32_t* __restrict__ list, int32_t* __restrict__ sub_off, PipeCounters* c) {
    __shared__ int s_cnt[1024], s_seg[1024];
    int base_cnt = 0, base_seg = 0, mmax = 0, slot1 = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int b = c0 + (int)threadIdx.x;
        int sel = 0, M = 0;
        if (b < n && new_rows[b] > 0) {
            int s0;
            if (uniform > 0) { M = uniform; s0 = b * M; } else { s0 = seg_offsets[b]; M = seg_offsets[b + 1] - s0; }
            sel = 1;
            mmax = M > mmax ? M : mmax;
            for (int i = 0; i < M; ++i) slot1 |= deriv[2 * ((size_t)s0 + i) + 1] >= 0;
        }
        s_cnt[threadIdx.x] = sel;
        s_seg[threadIdx.x] = sel ? M : 0;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {       // inclusive scans
            const int vc = threadIdx.x >= (unsigned)d ? s_cnt[threadIdx.x - d] : 0;
            const int vs = threadIdx.x >= (unsigned)d ? s_seg[threadIdx.x - d] : 0;
            __syncthreads();
            s_cnt[threadIdx.x] += vc;
            s_seg[threadIdx.x] += vs;
            __syncthreads();
        }
        if (sel) {
            const int k = base_cnt + s_cnt[threadIdx.x] - 1;
            list[k] = b;
            sub_off[k] = base_seg + s_seg[threadIdx.x] - M;
        }
        base_cnt += s_cnt[1023];
        base_seg += s_seg[1023];
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int om = __shfl_xor(mmax, d, 64);
        mmax = om > mmax ? om : mmax;
        slot1 |= __shfl_xor(slot1, d, 64);
    }
    if (threadIdx.x == 0) sub_off[base_cnt] = base_seg;
    if ((threadIdx.x & 63) == 0) {
        if (mmax) atomicMax(&c->gathered_max_m, (unsigned)mmax);
        if (slot1) atomicOr(&c->gathered_slot1, 1u);
    }
    if (threadIdx.x == 0) {
        c->gathered = (unsigned)base_cnt;
        c->gathered_segments = (unsigned)base_seg;
    }
}

// sub-batch k <- trajectory list[k]: waypoints, knot boxes, durations, boundary conditions, its rows (K = 1: slot 0 only).  One wave each.
__global__ __launch_bounds__(64) void pipe_rows_gather_kernel(int G, int uniform, const int32_t* __restrict__ seg_offsets, int r, int K,
                                                              const int32_t* __restrict__ list, const int32_t* __restrict__ sub_off,
                                                              const double* __restrict__ wp, const double* __restrict__ lo, const double* __restrict__ hi,
                                                              const double* __restrict__ times, const double* __restrict__ bc,
                                                              const double* __restrict__ tau, const int32_t* __restrict__ deriv,
                                                              const double* __restrict__ rlo, const double* __restrict__ rhi,
                                                              double* __restrict__ g_wp, double* __restrict__ g_lo, double* __restrict__ g_hi,
                                                              double* __restrict__ g_times, double* __restrict__ g_bc, double* __restrict__ g_tau,
                                                              int32_t* __restrict__ g_deriv, double* __restrict__ g_rlo, double* __restrict__ g_rhi) {
    for (int k = blockIdx.x; k < G; k += gridDim.x) {
        const int b = list[k], d0 = sub_off[k];
        int s0, M;
        if (uniform > 0) { M = uniform; s0 = b * M; } else { s0 = seg_offsets[b]; M = seg_offsets[b + 1] - s0; }
        const size_t e0 = 3 * ((size_t)s0 + b), f0 = 3 * ((size_t)d0 + k);
        for (int i = threadIdx.x; i < 3 * (M + 1); i += 64) {
            g_wp[f0 + i] = wp[e0 + i];
            g_lo[f0 + i] = lo[e0 + i];
            g_hi[f0 + i] = hi[e0 + i];
        }
        for (int i = threadIdx.x; i < M; i += 64) g_times[(size_t)d0 + i] = times[(size_t)s0 + i];
        const int nbc = 2 * (r - 1) * 3;
        for (int i = threadIdx.x; i < nbc; i += 64) g_bc[(size_t)k * nbc + i] = bc[(size_t)b * nbc + i];
        for (int q = threadIdx.x; q < M * K; q += 64) {
            const int i = q / K, j = q - i * K;
            const size_t src = 2 * ((size_t)s0 + i) + j, dst = (size_t)K * ((size_t)d0 + i) + j;
            g_tau[dst] = tau[src];
            g_deriv[dst] = deriv[src];
#pragma unroll
            for (int c = 0; c < 3; ++c) { g_rlo[3 * dst + c] = rlo[3 * src + c]; g_rhi[3 * dst + c] = rhi[3 * src + c]; }
        }
    }
}

// sub-batch k -> trajectory list[k] when its solve(s) ended UAVQP_SOLVED (st2 may be null: no second solve): coefficients, durations, status.
// Otherwise the rows this round placed are withdrawn; coefficients, durations and status stay what they were.
__global__ __launch_bounds__(64) void pipe_rows_scatter_kernel(int G, int uniform, const int32_t* __restrict__ seg_offsets, int r,
                                                               const int32_t* __restrict__ list, const int32_t* __restrict__ sub_off,
                                                               const int32_t* __restrict__ st1, const int32_t* __restrict__ st2,
                                                               const double* __restrict__ g_coeff, const double* __restrict__ g_times,
                                                               double* __restrict__ coeff, double* __restrict__ times, int32_t* __restrict__ status,
                                                               const uint8_t* __restrict__ placed, double* __restrict__ tau, int32_t* __restrict__ deriv,
                                                               double* __restrict__ rlo, double* __restrict__ rhi) {
    for (int k = blockIdx.x; k < G; k += gridDim.x) {
        const int b = list[k], d0 = sub_off[k];
        int s0, M;
        if (uniform > 0) { M = uniform; s0 = b * M; } else { s0 = seg_offsets[b]; M = seg_offsets[b + 1] - s0; }
        const bool ok = st1[k] == UAVQP_SOLVED && (!st2 || st2[k] == UAVQP_SOLVED);
        if (ok) {
            const int nc = 3 * 2 * r;
            for (int i = threadIdx.x; i < nc * M; i += 64) coeff[(size_t)nc * s0 + i] = g_coeff[(size_t)nc * d0 + i];
            for (int i = threadIdx.x; i < M; i += 64) times[(size_t)s0 + i] = g_times[(size_t)d0 + i];
            if (threadIdx.x == 0) status[b] = UAVQP_SOLVED;
        } else {
            for (int q = threadIdx.x; q < 2 * M; q += 64) {
                const size_t sg = (size_t)s0 + q / 2;
                if (placed[sg] & (1u << (q & 1))) {
                    const size_t rw = 2 * sg + (q & 1);
                    tau[rw] = 0.0;
                    deriv[rw] = -1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { rlo[3 * rw + c] = 0.0; rhi[3 * rw + c] = 0.0; }
                }
            }
        }
    }
}

// rows in place (deriv >= 0) -> rows_kept
__global__ __launch_bounds__(256) void pipe_rows_count_kernel(long long n_slots, const int32_t* __restrict__ deriv, PipeCounters* c) {
    int nk = 0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n_slots; k += (long long)gridDim.x * 256) nk += deriv[k] >= 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nk += __shfl_xor(nk, d, 64);
    if ((threadIdx.x & 63) == 0 && nk) atomicAdd(&c->rows_kept, (unsigned)nk);
}

}  // namespace uavqp

// the pinned page the pipeline's counters are read through: counter block [0] + the ring of per-round words [at 256 bytes];
// host-coherent: the device writes a round's word while the stream runs on
static int ensure_h_pipe(uavqp_ctx* ctx) {
    if (ctx->h_pipe) return UAVQP_OK;
    UAVQP_HIP(hipHostMalloc(&ctx->h_pipe, 1024, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(ctx->h_pipe, 0, 1024);
    return dev_grow(ctx->stream, ctx->pipe, 256);   // (as ever: a ctx's first call asks for the counter block alone, then for the layout below)
}

extern "C" void uavqp_default_pipeline_params(uavqp_pipeline_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_pipeline_params);
    p->robot_r = 0.4;        // test_kino_astar_searching.launch:56
    p->robot_h = 0.1;        // :57
    p->h_max = 0.8;          // corridor half-widths h ~ U(0.3, 0.8) m
    p->v_max = 7.0;          // max_velocity, test_kino_astar_searching.launch:49
    p->a_max = 10.0;         // max_accelration, :50
    p->max_rounds = 5;       // BASELINE config 5: "an outer loop of <= 5 time re-allocations"
    p->samples_per_seg = 16;
    p->max_stretch = 2.0;
    p->check_samples = 100;
    p->repair_rounds = 2;
    p->check_robot_r = 0.0;  // <= 0: the ellipsoid the boxes were built with
    p->check_robot_h = 0.0;
}

// rows from the hits of a check (include/uavqp.h uavqp_repair_rows_from_hits_device); the pipeline's form takes dt from the counter block,
// skips trajectories the check found free (first_hit) and those the rows solve cannot take, and records the slots it fills
static int repair_rows_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                            const double* d_coeff, int n_samples, double t0, double dt, const unsigned long long* d_tmax_bits,
                            const uint8_t* d_flags, const int32_t* d_first_hit, const double* d_obstacles, int n_obs, double robot_r,
                            double robot_h, double h_max, double* d_row_tau, int32_t* d_row_deriv, double* d_row_lo, double* d_row_hi,
                            int32_t* d_new_rows, uint8_t* d_placed, int solvable_only) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || n_samples < 0 || n_obs < 0 || !(robot_r > 0.0) || !(robot_h > 0.0) ||
        !(h_max >= 0.0))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || !d_new_rows || (n_samples > 0 && !d_flags) || (n_obs > 0 && !d_obstacles) || !d_row_tau || !d_row_deriv ||
        !d_row_lo || !d_row_hi || (uniform_segments == 0 && !d_seg_offsets))
        return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::RepairRowsArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_samples = n_samples; a.n_obs = n_obs;
    a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.t0 = t0; a.dt = dt; a.tmax_bits = d_tmax_bits;
    a.flags = d_flags; a.first_hit = d_first_hit; a.obs = d_obstacles; a.robot_r = robot_r; a.robot_h = robot_h; a.h_max = h_max;
    a.row_tau = d_row_tau; a.row_deriv = d_row_deriv; a.row_lo = d_row_lo; a.row_hi = d_row_hi; a.new_rows = d_new_rows;
    a.placed = d_placed; a.solvable_only = solvable_only;
    const int grid = n_traj < ctx->num_cus * 32 ? n_traj : ctx->num_cus * 32;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::repair_rows_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::repair_rows_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_repair_rows_from_hits_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                  const double* d_waypoints, const double* d_times, const double* d_coeff, int n_samples,
                                                  double t0, double dt, const uint8_t* d_flags, const double* d_obstacles, int n_obs,
                                                  double robot_r, double robot_h, double h_max, double* d_row_tau, int32_t* d_row_deriv,
                                                  double* d_row_lo, double* d_row_hi, int32_t* d_new_rows) {
    if (n_traj > 0 && !d_waypoints) return UAVQP_ERR_INVALID_ARG;
    return repair_rows_impl(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, n_samples, t0, dt, nullptr, d_flags, nullptr,
                            d_obstacles, n_obs, robot_r, robot_h, h_max, d_row_tau, d_row_deriv, d_row_lo, d_row_hi, d_new_rows, nullptr, 0);
}

// The box path (d_row_deriv == NULL) and the rows path (all four row arrays given) share this body; the box path runs exactly the
// launches it ran before the rows path existed.
static int corridor_pipeline_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                  const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                  const double* d_obstacles, int n_obs, const uavqp_grid* grid,
                                  const uavqp_pipeline_params* params, double* d_coeff_out, int32_t* d_status_out,
                                  double* d_corr_lo, double* d_corr_hi, int32_t* d_first_hit, double* d_row_tau, int32_t* d_row_deriv,
                                  double* d_row_lo, double* d_row_hi, uavqp_pipeline_result* result) {
    const bool rows_mode = d_row_deriv != nullptr;
    if (rows_mode && (!d_row_tau || !d_row_lo || !d_row_hi)) return UAVQP_ERR_INVALID_ARG;
    if (!ctx || !params || params->struct_size != (int32_t)sizeof(uavqp_pipeline_params) || (r != 3 && r != 4) || n_traj < 0 ||
        uniform_segments < 0 || n_obs < 0 || total_segments < 0)
        return UAVQP_ERR_INVALID_ARG;
    const uavqp_pipeline_params P = *params;
    if (!(P.robot_r > 0.0) || !(P.robot_h > 0.0) || !(P.h_max >= 0.0) || !(P.v_max > 0.0) || !(P.a_max > 0.0) || P.max_rounds < 1 ||
        P.samples_per_seg < 1 || !(P.max_stretch > 1.0) || P.check_samples < 0 || P.check_samples == 1 || P.repair_rounds < 0)
        return UAVQP_ERR_INVALID_ARG;
    if (result) *result = uavqp_pipeline_result{};
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out || !d_status_out || !d_corr_lo || !d_corr_hi || (n_obs > 0 && !d_obstacles) ||
        (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) ||
        (uniform_segments > 0 && (long long)uniform_segments * n_traj != total_segments))
        return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int n = n_traj, uni = uniform_segments, mx = uni > 0 ? uni : max_segments;
    // every workspace below is sized from the caller's total_segments: it is checked against the last CSR offset on the device
    // before anything that depends on it is launched.  The word travels through the host-coherent page (await_word below) while the
    // kernels that only look at seg_offsets[0..n] -- the dealing order, the counter reset -- already run.
    int rc = ensure_h_pipe(ctx);
    if (rc != UAVQP_OK) return rc;
    volatile unsigned long long* const h_words = (volatile unsigned long long*)((char*)ctx->h_pipe + 256);   // [0..3] round counts, [4] this check
    unsigned long long* d_words = nullptr;
    UAVQP_HIP(hipHostGetDevicePointer((void**)&d_words, (void*)h_words, 0));
    auto await_word = [&](int slot, unsigned int want, unsigned int* value) -> int {
        return await_host_word(s, h_words + slot, want, value, "uavqp_corridor_pipeline_device");
    };
    unsigned int probe_seq = 0u;
    if (uni == 0) hipLaunchKernelGGL(uavqp::host_word_kernel, dim3(1), dim3(1), 0, s, (const int32_t*)(d_seg_offsets + n_traj), (volatile unsigned long long*)(d_words + 4), probe_seq = ++ctx->pipe_seq);
    const int n_rows = total_segments + n_traj;
    const bool checking = P.check_samples > 0;

    const bool deal_by_length = uni == 0 && n >= 64 && ctx->settings.ragged_window_sort;
    // G of the dual prelude across the rounds (the re-allocation multiplies all durations of a trajectory by one factor: G only rescales)
    const bool g_across = ctx->settings.corridor_initial_guess == 2 && mx - 1 <= 24 && mx >= 2;
    const int cblocks = (n + uavqp::COMPACT_BLOCK - 1) / uavqp::COMPACT_BLOCK;           // workgroups of a compaction (more than one: two launches)
    if (cblocks > 1024) { g_last_error = "uavqp_corridor_pipeline_device: more than 16 777 216 trajectories in one call"; return UAVQP_ERR_INVALID_ARG; }
    const size_t nt_ = (size_t)n, ts_ = (size_t)total_segments, b_i32n = sizeof(int32_t) * nt_, b_wp = sizeof(double) * 3 * (ts_ + nt_);
    Carve c;
    const int i_cnt = c.add(256), i_it = c.add(b_i32n), i_ch = c.add(b_i32n), i_fh = c.add(b_i32n), i_as = c.add(sizeof(uint64_t) * 6 * nt_);
    const int i_rm = c.add(nt_), i_fl = c.add(nt_);
    const LengthOrder i_or = length_order_slots(c, n, deal_by_length);      // dealing order of the corridor solves
    // compacted dealing order of the next re-solve (two lists: round k compacts round k - 1's into the other one), then their two counts
    // (words 0 and 32 of one slot) and the per-workgroup counts of a large compaction
    const int i_cp[2] = {c.add(b_i32n), c.add(b_i32n)}, i_na = c.add(256), i_cblk = c.add(sizeof(int) * (size_t)cblocks);
    const int i_sc = c.add(sizeof(double) * nt_, g_across), i_gc = c.add(sizeof(double) * nt_ * uavqp::corridor_gcache_stride, g_across);
    // rows repair: per-sample flags of the check, new rows per trajectory, slots placed this round, the sub-batch (list, CSR offsets,
    // inputs, rows, outputs) -- sized for the whole batch
    const bool rm = rows_mode;
    const int i_sflags = c.add(nt_ * (size_t)(checking ? P.check_samples : 0), rm), i_newrows = c.add(b_i32n, rm), i_placed = c.add(ts_, rm);
    const int i_glist = c.add(sizeof(int32_t) * (nt_ + 1), rm), i_goff = c.add(sizeof(int32_t) * (nt_ + 1), rm);
    const int i_gwp = c.add(b_wp, rm), i_glo = c.add(b_wp, rm), i_ghi = c.add(b_wp, rm), i_gT = c.add(sizeof(double) * ts_, rm);
    const int i_gbc = c.add(sizeof(double) * nt_ * 2 * (r - 1) * 3, rm), i_gtau = c.add(sizeof(double) * 2 * ts_, rm), i_gdrv = c.add(sizeof(int32_t) * 2 * ts_, rm);
    const int i_grlo = c.add(sizeof(double) * 6 * ts_, rm), i_grhi = c.add(sizeof(double) * 6 * ts_, rm), i_gco = c.add(sizeof(double) * 3 * 2 * r * ts_, rm);
    const int i_gst1 = c.add(b_i32n, rm), i_gst2 = c.add(b_i32n, rm), i_git = c.add(b_i32n, rm), i_gch = c.add(b_i32n, rm);
    rc = carve_on(ctx->stream, ctx->pipe, c);
    if (rc != UAVQP_OK) return rc;
    uavqp::PipeCounters* d_cnt = c.at<uavqp::PipeCounters>(i_cnt);
    int32_t* d_iters = c.at<int32_t>(i_it);
    int32_t* d_changed = c.at<int32_t>(i_ch);
    int32_t* d_fh = d_first_hit ? d_first_hit : c.at<int32_t>(i_fh);
    uint64_t* d_active = c.at<uint64_t>(i_as);
    int32_t* const d_cp2[2] = {c.at<int32_t>(i_cp[0]), c.at<int32_t>(i_cp[1])};
    int* const d_na2[2] = {c.at<int>(i_na), c.at<int>(i_na) + 32};
    int* const d_cblk = c.at<int>(i_cblk);
    int cur_list = 0;                                                                  // the list the next re-solve takes
    double* d_scale = c.at<double>(i_sc);     // factor by which every trajectory was stretched since its G was stored
    double* d_gcache = c.at<double>(i_gc);
    int solves_done = 0;
    uint8_t* d_roomy = c.at<uint8_t>(i_rm);
    uint8_t* d_flag = c.at<uint8_t>(i_fl);
    uavqp::PipeCounters* h_cnt = (uavqp::PipeCounters*)ctx->h_pipe;
    uint8_t *d_sflags = c.at<uint8_t>(i_sflags), *d_placed = c.at<uint8_t>(i_placed);
    int32_t *d_newrows = c.at<int32_t>(i_newrows), *d_glist = c.at<int32_t>(i_glist), *d_goff = c.at<int32_t>(i_goff);
    double *d_gwp = c.at<double>(i_gwp), *d_glo = c.at<double>(i_glo), *d_ghi = c.at<double>(i_ghi), *d_gT = c.at<double>(i_gT), *d_gbc = c.at<double>(i_gbc);
    double *d_gtau = c.at<double>(i_gtau), *d_grlo = c.at<double>(i_grlo), *d_grhi = c.at<double>(i_grhi), *d_gco = c.at<double>(i_gco);
    int32_t *d_gdrv = c.at<int32_t>(i_gdrv), *d_gst1 = c.at<int32_t>(i_gst1), *d_gst2 = c.at<int32_t>(i_gst2), *d_git = c.at<int32_t>(i_git), *d_gch = c.at<int32_t>(i_gch);
    int cgrid = (n + 255) / 256;
    if (cgrid > ctx->num_cus * 8) cgrid = ctx->num_cus * 8;

    auto read_counters = [&]() -> int {   // device counter block -> pinned page, then the one synchronisation of this round
        UAVQP_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(uavqp::PipeCounters), hipMemcpyDeviceToHost, s));
        UAVQP_HIP(hipStreamSynchronize(s));
        return UAVQP_OK;
    };
    // (warm = 2: d_coeff_out still holds the previous round's polynomials -- their knot positions are the re-solve's starting point)
    // every corridor solve of the call deals the same trajectories: their order by segment count is made once
    const int32_t* d_order = nullptr;
    if (deal_by_length) {
        rc = make_length_order(ctx, d_seg_offsets, n, c, i_or, &d_order);
        if (rc != UAVQP_OK) return rc;
    }
    // Re-solves take only the trajectories whose problem changed since their last solve -- durations stretched by the re-allocation
    // (d_changed) or boxes shrunk by a repair (d_flag): the others would reproduce their coefficients bit for bit.  With the default
    // cold start (uavqp_settings.corridor_initial_guess = 2: the working set of the position-space dual method, verified by one block
    // solve) a re-solve is a cold solve; with the other settings it is warm-started from the previous round as before.
    const bool cold_rounds = ctx->settings.corridor_initial_guess == 2 && (uni > 0 ? uni : mx) - 1 <= 32;
    auto corridor_solve = [&](int warm, const int32_t* only_i32 = nullptr, const unsigned char* only_u8 = nullptr, bool precompacted = false) {
        const int32_t* d_cp = d_cp2[cur_list];
        const int* d_na = d_na2[cur_list];
        // first solve: every trajectory takes part, its G is stored; later solves load it and rescale by the stretch since then
        const int gmode = (g_across && cold_rounds) ? (solves_done == 0 ? 1 : 2) : 0;
        ++solves_done;
        return corridor_warm_impl(ctx, r, n, uni, mx, d_seg_offsets, d_waypoints, d_times, d_bc, d_corr_lo, d_corr_hi, d_coeff_out,
                                  d_status_out, d_iters, d_active, cold_rounds ? 0 : warm, total_segments, d_order, only_i32, only_u8,
                                  d_gcache, d_scale, gmode, precompacted ? d_cp : nullptr, precompacted ? d_na : nullptr);
    };
    auto reallocate = [&]() -> int {      // + count of the trajectories it stretched
        int rc_ = time_reallocate_impl(ctx, r, n, uni, d_seg_offsets, d_times, d_coeff_out, P.v_max, P.a_max, P.samples_per_seg,
                                       P.max_stretch, d_changed, d_scale);
        if (rc_ != UAVQP_OK) return rc_;
        hipLaunchKernelGGL(uavqp::pipe_zero_kernel, dim3(1), dim3(64), 0, s, d_cnt);
        hipLaunchKernelGGL(uavqp::pipe_count_kernel, dim3(cgrid), dim3(256), 0, s, (const int32_t*)d_changed, (const int32_t*)nullptr, n, d_cnt);
        return read_counters();
    };

    hipLaunchKernelGGL(uavqp::pipe_begin_kernel, dim3(d_scale ? (n + 255) / 256 : 1), dim3(256), 0, s, d_scale, n, d_cnt);
    if (rows_mode && total_segments > 0) {
        long long rgrid = (2LL * total_segments + 255) / 256;
        if (rgrid > (long long)ctx->num_cus * 8) rgrid = (long long)ctx->num_cus * 8;
        hipLaunchKernelGGL(uavqp::pipe_rows_clear_kernel, dim3((unsigned)rgrid), dim3(256), 0, s, 2LL * total_segments, d_row_tau, d_row_deriv,
                           d_row_lo, d_row_hi);
    }
    if (uni == 0) {
        unsigned int last_offset = 0u;
        rc = await_word(4, probe_seq, &last_offset);
        if (rc != UAVQP_OK) return rc;
        if ((int32_t)last_offset != total_segments) {
            g_last_error = "uavqp_corridor_pipeline_device: total_segments does not match seg_offsets[n_traj]";
            (void)hipStreamSynchronize(s);
            return UAVQP_ERR_INVALID_ARG;
        }
    }
    // 1. the reference's equality problem, 2. boxes from the cloud with the attitude of that solve
    rc = uavqp_solve_batch_device(ctx, r, n, uni, mx, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out, d_status_out);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_corridor_from_cloud_device(ctx, r, n, uni, d_seg_offsets, n_rows, d_waypoints, d_times, d_coeff_out, d_obstacles, n_obs,
                                          P.robot_r, P.robot_h, P.h_max, d_corr_lo, d_corr_hi, nullptr);
    if (rc != UAVQP_OK) return rc;
    // 3. outer loop.  The host only needs a round's count to know whether ANOTHER round is due, so it does not stop the stream for it:
    // the count of round k arrives in its own word of the host-coherent page (below), and round 1 -- later rounds while the last examined
    // one still stretched many trajectories (> n / 64) -- is enqueued before the previous count is looked at: if that one then reports
    // zero, the extra round re-solves nobody and stretches nobody (same bytes everywhere), at the price of a few empty launches.  Was
    // (round 3): copy + stream synchronisation + 25-30 us of idle device per round.
    int rounds = 0, still = 0;
    bool cap_solve_enqueued = false;
    {
        // A round's count reaches the host through a word of pinned, host-coherent memory that the compaction kernel writes itself, tagged
        // with the round's sequence number: the host polls the word (was: a 4-byte copy + an event per round -- a copy kernel and ~6 us of
        // idle device behind the event packet, per round).
        unsigned long long* const d_ring = d_words;
        unsigned int seq_of[4] = {0u, 0u, 0u, 0u};
        auto enqueue_round = [&](int rnd) -> int {
            int rc_ = corridor_solve(rnd > 0 ? 2 : 0, rnd > 0 ? (const int32_t*)d_changed : nullptr, nullptr, rnd > 0);
            if (rc_ != UAVQP_OK) return rc_;
            // rounds after the first look only at the trajectories that round re-solved (the list of the previous compaction): the others
            // have the coefficients and durations the previous re-allocation already accepted (their flag in d_changed is 0 and stays 0)
            const int32_t* d_prev = rnd > 0 ? d_cp2[cur_list] : nullptr;
            const int* d_nprev = rnd > 0 ? d_na2[cur_list] : nullptr;
            rc_ = time_reallocate_impl(ctx, r, n, uni, d_seg_offsets, d_times, d_coeff_out, P.v_max, P.a_max, P.samples_per_seg,
                                       P.max_stretch, d_changed, d_scale, d_prev, d_nprev);
            if (rc_ != UAVQP_OK) return rc_;
            // the dealing order of the trajectories it stretched, for the re-solve of the next round -- and their number, which is the
            // round's counter (was: a zeroing kernel, a counting kernel, and the compaction at the head of the next solve)
            const int nxt = rnd > 0 ? cur_list ^ 1 : cur_list;
            seq_of[rnd & 3] = ++ctx->pipe_seq;
            if (cblocks == 1)
                hipLaunchKernelGGL(uavqp::compact_order_kernel, dim3(1), dim3(1024), 0, s, rnd > 0 ? d_prev : d_order, n, (const int32_t*)d_changed,
                                   (const unsigned char*)nullptr, d_cp2[nxt], d_na2[nxt], (const unsigned int*)nullptr, d_nprev,
                                   (volatile unsigned long long*)&d_ring[rnd & 3], seq_of[rnd & 3]);
            else
                for (int phase = 0; phase < 2; ++phase)
                    hipLaunchKernelGGL(uavqp::compact_order_blocks_kernel, dim3(cblocks), dim3(1024), 0, s, rnd > 0 ? d_prev : d_order, n,
                                       (const int32_t*)d_changed, (const unsigned char*)nullptr, d_cp2[nxt], d_na2[nxt], d_nprev, d_cblk, phase,
                                       (volatile unsigned long long*)&d_ring[rnd & 3], seq_of[rnd & 3]);
            cur_list = nxt;
            if (rnd + 1 == P.max_rounds) {
                // the cap: the trajectories this last re-allocation stretched need one more solve so that their coefficients belong to
                // d_times -- enqueued behind the compaction without waiting for its count (an empty list solves nobody)
                rc_ = corridor_solve(2, (const int32_t*)d_changed, nullptr, true);
                if (rc_ != UAVQP_OK) return rc_;
                cap_solve_enqueued = true;
            }
            return UAVQP_OK;
        };
        int enq = 0, exam = 0;
        unsigned int last = 0;
        for (;;) {
            // (round 1 is enqueued unseen too: a batch that comes here for a re-allocation normally has something to stretch in round 0)
            while (enq < P.max_rounds && (enq <= exam || (enq == exam + 1 && (exam == 0 || (long long)last * 64 > (long long)n)))) {
                rc = enqueue_round(enq);
                if (rc != UAVQP_OK) return rc;
                ++enq;
            }
            if (exam >= enq) break;
            rc = await_word(exam & 3, seq_of[exam & 3], &last);
            if (rc != UAVQP_OK) return rc;
            ++exam;
            ++rounds;
            still = (int)last;
            if (still == 0 || exam >= P.max_rounds) break;   // the last solve already belongs to the final durations / cap reached
        }
        // (a speculative round may still be in flight: everything that follows is ordered behind it on the same stream)
    }
    if (still != 0 && !cap_solve_enqueued) {
        // cap reached with durations changed by the last re-allocation: one more solve so that the coefficients match d_times
        rc = corridor_solve(2, (const int32_t*)d_changed, nullptr, true);
        if (rc != UAVQP_OK) return rc;
    }
    // 4. check + repair
    int repairs = 0, before = -1, blocked = 0, after = 0, summary_unsolved = -1;
    // Rows repair round on the sub-batch of the G trajectories that received a row (list + CSR offsets made by the compaction): gather,
    // general-rows solve with their knot boxes and rows, one re-allocation of the sub-batch and a second solve if it stretched anything,
    // then write back what ended UAVQP_SOLVED -- the others keep coefficients, durations and status and lose this round's rows.
    auto rows_repair_round = [&](int G, int Gseg, int Gmax, int K) -> int {
        int ggrid = G < ctx->num_cus * 32 ? G : ctx->num_cus * 32;
        hipLaunchKernelGGL(uavqp::pipe_rows_gather_kernel, dim3(ggrid), dim3(64), 0, s, G, uni, d_seg_offsets, r, K, (const int32_t*)d_glist,
                           (const int32_t*)d_goff, d_waypoints, (const double*)d_corr_lo, (const double*)d_corr_hi, (const double*)d_times, d_bc,
                           (const double*)d_row_tau, (const int32_t*)d_row_deriv, (const double*)d_row_lo, (const double*)d_row_hi, d_gwp, d_glo,
                           d_ghi, d_gT, d_gbc, d_gtau, d_gdrv, d_grlo, d_grhi);
        int rc_ = rows_batch_impl(ctx, r, G, 0, Gmax, d_goff, d_gwp, d_gT, d_gbc, d_glo, d_ghi, K, d_gtau, d_gdrv, d_grlo, d_grhi, d_gco, d_gst1,
                                  d_git, nullptr, Gseg);
        if (rc_ != UAVQP_OK) return rc_;
        rc_ = time_reallocate_impl(ctx, r, G, 0, d_goff, d_gT, d_gco, P.v_max, P.a_max, P.samples_per_seg, P.max_stretch, d_gch, nullptr);
        if (rc_ != UAVQP_OK) return rc_;
        hipLaunchKernelGGL(uavqp::pipe_zero_kernel, dim3(1), dim3(64), 0, s, d_cnt);
        int g2 = (G + 255) / 256;
        if (g2 > ctx->num_cus * 8) g2 = ctx->num_cus * 8;
        hipLaunchKernelGGL(uavqp::pipe_count_kernel, dim3(g2), dim3(256), 0, s, (const int32_t*)d_gch, (const int32_t*)nullptr, G, d_cnt);
        rc_ = read_counters();
        if (rc_ != UAVQP_OK) return rc_;
        still = (int)h_cnt->changed;
        const bool again = still > 0;
        if (again) {   // rows are fractions of T_i: they stay attached to the stretched segments
            rc_ = rows_batch_impl(ctx, r, G, 0, Gmax, d_goff, d_gwp, d_gT, d_gbc, d_glo, d_ghi, K, d_gtau, d_gdrv, d_grlo, d_grhi, d_gco, d_gst2,
                                  d_git, nullptr, Gseg);
            if (rc_ != UAVQP_OK) return rc_;
        }
        hipLaunchKernelGGL(uavqp::pipe_rows_scatter_kernel, dim3(ggrid), dim3(64), 0, s, G, uni, d_seg_offsets, r, (const int32_t*)d_glist,
                           (const int32_t*)d_goff, (const int32_t*)d_gst1, again ? (const int32_t*)d_gst2 : (const int32_t*)nullptr,
                           (const double*)d_gco, (const double*)d_gT, d_coeff_out, d_times, d_status_out, (const uint8_t*)d_placed, d_row_tau,
                           d_row_deriv, d_row_lo, d_row_hi);
        UAVQP_HIP(hipGetLastError());
        return UAVQP_OK;
    };
    double check_dt = 0.0;
    uavqp_grid* own_grid = nullptr;
    if (checking) {
        const double chk_r = P.check_robot_r > 0.0 ? P.check_robot_r : P.robot_r, chk_h = P.check_robot_h > 0.0 ? P.check_robot_h : P.robot_h;
        if (!grid) {
            rc = uavqp_obstacle_grid_build_device(ctx, d_obstacles, n_obs, chk_r + 0.1, &own_grid);
            if (rc != UAVQP_OK) return rc;
            grid = own_grid;
        }
        int pgrid = (int)(((long long)n * 8 + 255) / 256);
        if (pgrid > ctx->num_cus * 2) pgrid = ctx->num_cus * 2;
        for (int pass = 0;; ++pass) {
            // (the counter block is zero: pipe_begin_kernel, nothing since -- after a repair the zeroing kernel below)
            if (pass > 0) hipLaunchKernelGGL(uavqp::pipe_zero_kernel, dim3(1), dim3(64), 0, s, d_cnt);
            hipLaunchKernelGGL(uavqp::pipe_check_prep_kernel, dim3(pgrid), dim3(256), 0, s, n, uni, d_seg_offsets, (const double*)d_times,
                               (const double*)d_corr_lo, (const double*)d_corr_hi, pass == 0 ? d_roomy : (uint8_t*)nullptr, d_fh, P.check_samples, d_cnt);
            rc = ellipsoid_check_grid_impl(ctx, r, n, uni, d_seg_offsets, d_times, d_coeff_out, P.check_samples, 0.0, 0.0, &d_cnt->tmax_bits, grid,
                                           chk_r, chk_h, d_fh, d_sflags);
            if (rc != UAVQP_OK) break;
            hipLaunchKernelGGL(uavqp::pipe_hits_kernel, dim3(cgrid), dim3(256), 0, s, n, (const int32_t*)d_fh, P.check_samples, (const uint8_t*)d_roomy, d_flag,
                               (const int32_t*)d_status_out, d_cnt);
            if (rows_mode && repairs < P.repair_rounds) {
                // rows from the hits (dt from the counter block, as the check formed it) and the sub-batch they make: its size arrives
                // with the check's counters
                if (total_segments > 0) UAVQP_HIP(hipMemsetAsync(d_placed, 0, (size_t)total_segments, s));
                rc = repair_rows_impl(ctx, r, n, uni, d_seg_offsets, d_times, d_coeff_out, P.check_samples, 0.0, 0.0, &d_cnt->tmax_bits, d_sflags,
                                      d_fh, d_obstacles, n_obs, chk_r, chk_h, P.h_max, d_row_tau, d_row_deriv, d_row_lo, d_row_hi, d_newrows, d_placed, 1);
                if (rc != UAVQP_OK) break;
                hipLaunchKernelGGL(uavqp::pipe_rows_compact_kernel, dim3(1), dim3(1024), 0, s, n, uni, d_seg_offsets, (const int32_t*)d_newrows,
                                   (const int32_t*)d_row_deriv, d_glist, d_goff, d_cnt);
            }
            rc = read_counters();
            if (rc != UAVQP_OK) break;
            double tmax;
            std::memcpy(&tmax, &h_cnt->tmax_bits, sizeof(double));
            check_dt = tmax / (double)(P.check_samples - 1);          // the quotient the check kernel formed from the same bits
            summary_unsolved = (int)h_cnt->unsolved;
            after = (int)h_cnt->hit;
            if (before < 0) {
                before = (int)h_cnt->hit;
                blocked = (int)h_cnt->hit_blocked;
            }
            if (rows_mode) {
                if (h_cnt->hit == 0 || repairs >= P.repair_rounds || h_cnt->gathered == 0) break;
                rc = rows_repair_round((int)h_cnt->gathered, (int)h_cnt->gathered_segments, (int)h_cnt->gathered_max_m, h_cnt->gathered_slot1 ? 2 : 1);
                if (rc != UAVQP_OK) break;
                summary_unsolved = -1;
                ++repairs;
                continue;
            }
            if (h_cnt->hit_repairable == 0 || repairs >= P.repair_rounds) break;
            // halve the boxes of the flagged trajectories towards their waypoints (last round: the waypoint equalities), re-solve
            // warm-started, re-allocate once (the durations only ever stretch) and solve again if that changed anything
            summary_unsolved = -1;                                     // statuses change below: the summary is counted again
            const double shrink = (repairs + 1 == P.repair_rounds) ? 0.0 : 0.5;
            hipLaunchKernelGGL(uavqp::pipe_shrink_kernel, dim3(n < ctx->num_cus * 32 ? n : ctx->num_cus * 32), dim3(64), 0, s, n, uni, d_seg_offsets,
                               d_waypoints, d_corr_lo, d_corr_hi, (const uint8_t*)d_flag, shrink);
            rc = corridor_solve(2, nullptr, (const unsigned char*)d_flag);
            if (rc != UAVQP_OK) break;
            rc = reallocate();
            if (rc != UAVQP_OK) break;
            still = (int)h_cnt->changed;
            if (still > 0) {
                rc = corridor_solve(2, (const int32_t*)d_changed);
                if (rc != UAVQP_OK) break;
            }
            ++repairs;
        }
        if (own_grid) (void)uavqp_obstacle_grid_destroy(ctx, own_grid);
        if (rc != UAVQP_OK) return rc;
    }
    // 5. summary (the last check pass counted the statuses along with its hits unless a repair re-solved something after it)
    if (summary_unsolved < 0) {
        hipLaunchKernelGGL(uavqp::pipe_zero_kernel, dim3(1), dim3(64), 0, s, d_cnt);
        hipLaunchKernelGGL(uavqp::pipe_count_kernel, dim3(cgrid), dim3(256), 0, s, (const int32_t*)nullptr, (const int32_t*)d_status_out, n, d_cnt);
        rc = read_counters();
        if (rc != UAVQP_OK) return rc;
        summary_unsolved = (int)h_cnt->unsolved;
    }
    int rows_kept = 0;
    if (rows_mode && total_segments > 0) {
        hipLaunchKernelGGL(uavqp::pipe_zero_kernel, dim3(1), dim3(64), 0, s, d_cnt);
        hipLaunchKernelGGL(uavqp::pipe_rows_count_kernel, dim3(cgrid), dim3(256), 0, s, 2LL * total_segments, (const int32_t*)d_row_deriv, d_cnt);
        rc = read_counters();
        if (rc != UAVQP_OK) return rc;
        rows_kept = (int)h_cnt->rows_kept;
    }
    UAVQP_HIP(hipGetLastError());
    if (result) {
        result->repair_rows = rows_kept;
        result->rounds = rounds;
        result->repairs = repairs;
        result->still_stretching = still;
        result->colliding_before_repair = before < 0 ? 0 : before;
        result->colliding_with_blocked_waypoints = blocked;
        result->colliding_after = after;
        result->unsolved = (int32_t)summary_unsolved;
        result->check_dt = check_dt;
    }
    return UAVQP_OK;
}

extern "C" int uavqp_corridor_pipeline_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                              const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                              const double* d_obstacles, int n_obs, const uavqp_grid* grid,
                                              const uavqp_pipeline_params* params, double* d_coeff_out, int32_t* d_status_out,
                                              double* d_corr_lo, double* d_corr_hi, int32_t* d_first_hit, uavqp_pipeline_result* result) {
    return corridor_pipeline_impl(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc,
                                  d_obstacles, n_obs, grid, params, d_coeff_out, d_status_out, d_corr_lo, d_corr_hi, d_first_hit, nullptr, nullptr,
                                  nullptr, nullptr, result);
}

extern "C" int uavqp_corridor_pipeline_rows_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                                   const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                                   const double* d_obstacles, int n_obs, const uavqp_grid* grid,
                                                   const uavqp_pipeline_params* params, double* d_coeff_out, int32_t* d_status_out,
                                                   double* d_corr_lo, double* d_corr_hi, int32_t* d_first_hit, double* d_row_tau,
                                                   int32_t* d_row_deriv, double* d_row_lo, double* d_row_hi, uavqp_pipeline_result* result) {
    if (n_traj > 0 && (!d_row_tau || !d_row_deriv || !d_row_lo || !d_row_hi)) return UAVQP_ERR_INVALID_ARG;
    return corridor_pipeline_impl(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc,
                                  d_obstacles, n_obs, grid, params, d_coeff_out, d_status_out, d_corr_lo, d_corr_hi, d_first_hit, d_row_tau,
                                  d_row_deriv, d_row_lo, d_row_hi, result);
}

static int corridor_pipeline_host_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                       const int32_t* seg_offsets, const double* waypoints, double* times, const double* bc,
                                       const double* obstacles, int n_obs, const uavqp_pipeline_params* params, double* coeff_out,
                                       int32_t* status_out, double* corr_lo, double* corr_hi, int32_t* first_hit, double* row_tau,
                                       int32_t* row_deriv, double* row_lo, double* row_hi, uavqp_pipeline_result* result) {
    const bool rows_mode = row_deriv != nullptr;
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || n_obs < 0) return UAVQP_ERR_INVALID_ARG;
    if (result) *result = uavqp_pipeline_result{};
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out || (n_obs > 0 && !obstacles) || (uniform_segments == 0 && !seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, b_wp = sizeof(double) * 3 * (tot + n);
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.in(waypoints, b_wp);
    const int i_lo = st.out(corr_lo, b_wp), i_hi = st.out(corr_hi, b_wp);   // (the boxes: scratch when the caller does not want them back)
    const int i_t = st.inout(times, sizeof(double) * tot);                  // stretched by the re-allocation
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_obs = st.in(n_obs > 0 ? obstacles : nullptr, sizeof(double) * 3 * (size_t)(n_obs > 0 ? n_obs : 1));
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_fh = st.out(params && params->check_samples > 0 ? first_hit : nullptr, sizeof(int32_t) * n);   // (written by the check only)
    const int i_rt = rows_mode ? st.out(row_tau, sizeof(double) * 2 * tot) : -1, i_rd = rows_mode ? st.out(row_deriv, sizeof(int32_t) * 2 * tot) : -1;
    const int i_rl = rows_mode ? st.out(row_lo, sizeof(double) * 6 * tot) : -1, i_rh = rows_mode ? st.out(row_hi, sizeof(double) * 6 * tot) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = corridor_pipeline_impl(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                                st.at<double>(i_t), st.at<double>(i_bc), st.at<double>(i_obs), n_obs, nullptr, params, st.at<double>(i_out),
                                st.at<int32_t>(i_st), st.at<double>(i_lo), st.at<double>(i_hi), st.at<int32_t>(i_fh), st.at<double>(i_rt),
                                st.at<int32_t>(i_rd), st.at<double>(i_rl), st.at<double>(i_rh), result);
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_corridor_pipeline_host");
}

extern "C" int uavqp_corridor_pipeline_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                            const int32_t* seg_offsets, const double* waypoints, double* times, const double* bc,
                                            const double* obstacles, int n_obs, const uavqp_pipeline_params* params, double* coeff_out,
                                            int32_t* status_out, double* corr_lo, double* corr_hi, int32_t* first_hit,
                                            uavqp_pipeline_result* result) {
    return corridor_pipeline_host_impl(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, obstacles, n_obs, params,
                                       coeff_out, status_out, corr_lo, corr_hi, first_hit, nullptr, nullptr, nullptr, nullptr, result);
}

extern "C" int uavqp_corridor_pipeline_rows_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                                 const int32_t* seg_offsets, const double* waypoints, double* times, const double* bc,
                                                 const double* obstacles, int n_obs, const uavqp_pipeline_params* params, double* coeff_out,
                                                 int32_t* status_out, double* corr_lo, double* corr_hi, int32_t* first_hit, double* row_tau,
                                                 int32_t* row_deriv, double* row_lo, double* row_hi, uavqp_pipeline_result* result) {
    if (n_traj > 0 && (!row_tau || !row_deriv || !row_lo || !row_hi)) return UAVQP_ERR_INVALID_ARG;
    return corridor_pipeline_host_impl(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, obstacles, n_obs, params,
                                       coeff_out, status_out, corr_lo, corr_hi, first_hit, row_tau, row_deriv, row_lo, row_hi, result);
}
