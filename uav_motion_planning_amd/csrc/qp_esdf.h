// qp_esdf.h -- occupancy grid -> signed Euclidean distance field, its trilinear query, and the clearance penalty of solved trajectories
// against it (uavqp_esdf_* / uavqp_clearance_penalty_*, include/uavqp.h).  Translation unit: k_esdf.hip.
//
// Grid.  [nx][ny][nz], z fastest (the reference's toAddress); a voxel index is below 2^30 and stays an int, the byte offsets are widened
// where a pointer is indexed.
// Rasterise.  One lane per (point, inflation offset); a hit stores the byte 1 (idempotent: no atomics, no order).
// Update.  Three separable passes over two int32 fields (squared voxel distance to the nearest occupied / nearest free voxel), in place:
//   z    a block stages up to ESDF_TILE voxels of whole, consecutive z lines as bytes in LDS; a lane owns output positions and walks
//        outwards from p until both an occupied and a free voxel were met: the 1-D squared distances of both fields from one tile.
//   y, x a block stages the slab (all q of the axis) x (a tile of neighbouring z) of one field in LDS -- global loads and stores run along
//        z -- and a lane takes  min_q f(q) + (p - q)^2  by walking outwards from p, stopping once (p - q)^2 reaches its best: exact, no
//        run-time indexed arrays in registers.  Lanes of a wave read consecutive LDS words at every step.
//   The x pass turns the sentinel into INT32_MAX and writes dist (float64) with the second field: a lane owns the same voxels in both
//   rounds, so it reads back the sq_pos it wrote itself.  "No such voxel" is ESDF_INF = 2^30 between the passes (every true value is
//   below 3 * 1023^2; 2^30 + 1023^2 does not overflow).
// Query.  One lane per point, eight gathers; the interpolation of the reference's getDistWithGradTrilinear.
// Penalty.  The structure of limit_penalty_kernel (qp_limits.h): eight lanes per trajectory, sub-lane j owns segments j, j + 8, ..., the
//   field query inlined per sample, the coefficient gradient kept in registers and stored once per segment, sums by the xor butterfly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/uavqp.h"
#include "qp_limits.h"

namespace uavqp {

constexpr int ESDF_INF = 1 << 30;
constexpr int ESDF_TILE = 8192;    // LDS entries of a block: 8 KB of bytes in the z pass, 32 KB of int32 in the y / x passes
constexpr int ESDF_BLOCK = 256;

struct EsdfView {
    int nx, ny, nz;
    double ox, oy, oz;       // origin
    double hx, hy, hz;       // origin + dims * resolution
    double res, inv_res, max_dist;
    const double* dist;
};

struct EsdfRasterArgs {
    int nx, ny, nz;
    double ox, oy, oz, res, inv_res;
    const double* pts;       // [n_pts][3]
    int n_pts, ixy, iz;
    uint8_t* occ;
};

struct EsdfArgs {
    int nx, ny, nz;
    const uint8_t* occ;
    int32_t* sq_pos;
    int32_t* sq_neg;
    double* dist;
    double res, max_dist;
};

struct EsdfQueryArgs {
    EsdfView map;
    int n_pts;
    const double* pts;       // [n_pts][3]
    double* dist;            // [n_pts] or null
    double* grad;            // [n_pts][3] or null
    uint8_t* inside;         // [n_pts] or null
};

struct ClearanceArgs {
    int n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;    // null: every trajectory counts as solved
    double* penalty;          // [n_traj] or null
    double* grad_coeff;       // layout of coeff, or null
    double* grad_times;       // [sum M] or null
    double* min_dist;         // [n_traj] or null
    int32_t* outside;         // [n_traj] or null
    int K, al16;
    double d_safe, inv_safe, weight;
    EsdfView map;
};

// distance and gradient at one point; false (dist = 0, grad = 0) outside the map.  A NaN coordinate is outside.
__device__ inline bool esdf_sample(const EsdfView& m, double px, double py, double pz, double& dist, double (&g)[3]) {
    dist = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    if (!(px >= m.ox + 1e-4 && px <= m.hx - 1e-4 && py >= m.oy + 1e-4 && py <= m.hy - 1e-4 && pz >= m.oz + 1e-4 && pz <= m.hz - 1e-4)) return false;
    const double half = 0.5 * m.res;
    const int ix = (int)floor((px - half - m.ox) * m.inv_res), iy = (int)floor((py - half - m.oy) * m.inv_res),
              iz = (int)floor((pz - half - m.oz) * m.inv_res);
    const double dx = (px - (((double)ix + 0.5) * m.res + m.ox)) * m.inv_res, dy = (py - (((double)iy + 0.5) * m.res + m.oy)) * m.inv_res,
                 dz = (pz - (((double)iz + 0.5) * m.res + m.oz)) * m.inv_res;
    const int x0 = min(max(ix, 0), m.nx - 1), x1 = min(max(ix + 1, 0), m.nx - 1);
    const int y0 = min(max(iy, 0), m.ny - 1), y1 = min(max(iy + 1, 0), m.ny - 1);
    const int z0 = min(max(iz, 0), m.nz - 1), z1 = min(max(iz + 1, 0), m.nz - 1);
    const double* __restrict__ D = m.dist;
    const int r00 = (x0 * m.ny + y0) * m.nz, r01 = (x0 * m.ny + y1) * m.nz, r10 = (x1 * m.ny + y0) * m.nz, r11 = (x1 * m.ny + y1) * m.nz;
    const double v000 = D[r00 + z0], v001 = D[r00 + z1], v010 = D[r01 + z0], v011 = D[r01 + z1];
    const double v100 = D[r10 + z0], v101 = D[r10 + z1], v110 = D[r11 + z0], v111 = D[r11 + z1];
    const double v00 = (1 - dx) * v000 + dx * v100, v01 = (1 - dx) * v001 + dx * v101;
    const double v10 = (1 - dx) * v010 + dx * v110, v11 = (1 - dx) * v011 + dx * v111;
    const double v0 = (1 - dy) * v00 + dy * v10, v1 = (1 - dy) * v01 + dy * v11;
    dist = (1 - dz) * v0 + dz * v1;
    g[2] = (v1 - v0) * m.inv_res;
    g[1] = ((1 - dz) * (v10 - v00) + dz * (v11 - v01)) * m.inv_res;
    double gx = (1 - dz) * (1 - dy) * (v100 - v000);
    gx += (1 - dz) * dy * (v110 - v010);
    gx += dz * (1 - dy) * (v101 - v001);
    gx += dz * dy * (v111 - v011);
    g[0] = gx * m.inv_res;
    return true;
}

// (defined in k_esdf.hip alone; the host translation unit launches them through these declarations and kernel_instances.h)
__global__ __launch_bounds__(ESDF_BLOCK) void esdf_raster_kernel(EsdfRasterArgs a);
__global__ __launch_bounds__(ESDF_BLOCK) void esdf_z_kernel(EsdfArgs a, int lines_per_block);
template <bool LAST>
__global__ __launch_bounds__(ESDF_BLOCK) void esdf_axis_kernel(EsdfArgs a, int n, int stride, int outer_stride, int zt, int n_ztiles);
__global__ __launch_bounds__(ESDF_BLOCK) void esdf_query_kernel(EsdfQueryArgs a);
template <int R>
__global__ __launch_bounds__(64) void clearance_penalty_kernel(ClearanceArgs a);

#if defined(UAVQP_KERNEL_TU) || defined(UAVQP_SINGLE_TU)

__global__ __launch_bounds__(ESDF_BLOCK) void esdf_raster_kernel(EsdfRasterArgs a) {
    const int wxy = 2 * a.ixy + 1, wz = 2 * a.iz + 1;
    const long long n_off = (long long)wxy * wxy * wz, total = n_off * a.n_pts;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += step) {
        const long long pt = g / n_off;
        long long o = g - pt * n_off;
        const int kz = (int)(o % wz) - a.iz;
        o /= wz;
        const int ky = (int)(o % wxy) - a.ixy, kx = (int)(o / wxy) - a.ixy;
        const double fx = floor((a.pts[3 * pt] + (double)kx * a.res - a.ox) * a.inv_res);
        const double fy = floor((a.pts[3 * pt + 1] + (double)ky * a.res - a.oy) * a.inv_res);
        const double fz = floor((a.pts[3 * pt + 2] + (double)kz * a.res - a.oz) * a.inv_res);
        // (compared as doubles: a far or non-finite point never reaches the cast)
        if (fx >= 0.0 && fx < (double)a.nx && fy >= 0.0 && fy < (double)a.ny && fz >= 0.0 && fz < (double)a.nz)
            a.occ[((int)fx * a.ny + (int)fy) * a.nz + (int)fz] = 1;
    }
}

__global__ __launch_bounds__(ESDF_BLOCK) void esdf_z_kernel(EsdfArgs a, int lines_per_block) {
    __shared__ uint8_t tile[ESDF_TILE];
    const int n_lines = a.nx * a.ny, nz = a.nz;
    const int l0 = blockIdx.x * lines_per_block;
    const int nl = min(lines_per_block, n_lines - l0);
    const int base = l0 * nz, cnt = nl * nz;          // cnt <= ESDF_TILE (the host picks lines_per_block so)
    for (int e = threadIdx.x; e < cnt; e += ESDF_BLOCK) tile[e] = a.occ[base + e] != 0 ? 1 : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += ESDF_BLOCK) {
        const int line = e / nz, p = e - line * nz, lo = line * nz;
        const int dmax = max(p, nz - 1 - p);
        int dp = ESDF_INF, dn = ESDF_INF;
        for (int d = 0; d <= dmax && (dp == ESDF_INF || dn == ESDF_INF); ++d) {
            bool occ = false, fre = false;
            if (p - d >= 0) { const bool u = tile[lo + p - d] != 0; occ |= u; fre |= !u; }
            if (p + d < nz) { const bool u = tile[lo + p + d] != 0; occ |= u; fre |= !u; }
            if (occ && dp == ESDF_INF) dp = d * d;
            if (fre && dn == ESDF_INF) dn = d * d;
        }
        a.sq_pos[base + e] = dp;
        a.sq_neg[base + e] = dn;
    }
}

template <bool LAST>
__global__ __launch_bounds__(ESDF_BLOCK) void esdf_axis_kernel(EsdfArgs a, int n, int stride, int outer_stride, int zt, int n_ztiles) {
    __shared__ int32_t tile[ESDF_TILE];
    const int o = blockIdx.x / n_ztiles, z0 = (blockIdx.x - o * n_ztiles) * zt;
    const int w = min(zt, a.nz - z0);
    const int base = o * outer_stride + z0, cnt = n * w;   // cnt <= ESDF_TILE (the host picks zt so)
#pragma unroll 1
    for (int field = 0; field < 2; ++field) {
        int32_t* F = field == 0 ? a.sq_pos : a.sq_neg;
        for (int e = threadIdx.x; e < cnt; e += ESDF_BLOCK) {
            const int q = e / w, z = e - q * w;
            tile[e] = F[base + q * stride + z];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += ESDF_BLOCK) {
            const int p = e / w, z = e - p * w;
            const int dmax = max(p, n - 1 - p);
            int best = tile[e];
            for (int d = 1; d <= dmax; ++d) {
                const int dd = d * d;
                if (dd >= best) break;
                if (p - d >= 0) best = min(best, tile[e - d * w] + dd);
                if (p + d < n) best = min(best, tile[e + d * w] + dd);
            }
            best = min(best, ESDF_INF);
            const int at = base + p * stride + z;
            if (!LAST) {
                F[at] = best;
            } else {
                const int32_t sq = best >= ESDF_INF ? INT32_MAX : best;
                F[at] = sq;
                if (field == 1) {
                    const double d_pos = fmin(a.res * sqrt((double)a.sq_pos[at]), a.max_dist);   // (round 0 of this same lane wrote it)
                    const double d_neg = fmin(a.res * sqrt((double)sq), a.max_dist);
                    a.dist[at] = d_neg == 0.0 ? d_pos : d_pos - d_neg + a.res;
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ESDF_BLOCK) void esdf_query_kernel(EsdfQueryArgs a) {
    const int step = gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_pts; i += step) {
        double d, g[3];
        const bool in = esdf_sample(a.map, a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2], d, g);
        if (a.dist) a.dist[i] = d;
        if (a.grad) { a.grad[3 * i] = g[0]; a.grad[3 * i + 1] = g[1]; a.grad[3 * i + 2] = g[2]; }
        if (a.inside) a.inside[i] = in ? 1 : 0;
    }
}

template <int R>
__global__ __launch_bounds__(64) void clearance_penalty_kernel(ClearanceArgs a) {
    constexpr int NC = 2 * R, LPT = TOPT_LPT;
    // (the loop of topt_for_each_group written out: through the lambda the compiler stops peeling the sample loop, which moves the last bits
    // of the penalty and of its time gradient -- docs/measurement_log.md)
    const int sub = threadIdx.x % LPT;
    const long long n_lanes = (long long)a.n_traj * LPT;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n_round = (n_lanes + stride - 1) / stride * stride;  // whole waves take part in the shuffles
    const double inv_K = 1.0 / (double)a.K;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_round; g += stride) {
        const bool live = g < n_lanes;
        const int b = live ? (int)(g / LPT) : 0;
        const auto [s0, M] = live ? poly_span(a.uniform, a.seg_offsets, b) : PolySpan{0, 0};
        const size_t axs = (size_t)NC * (M > 0 ? M : 0);
        const bool solved = live && M > 0 && (!a.status || a.status[b] == UAVQP_SOLVED);
        double Phi = 0.0, neg_min = -INFINITY;   // (the minimum as a maximum of negatives: topt_group_max)
        int n_out = 0;
        for (int i = sub; i < M; i += LPT) {
            const size_t at = (size_t)3 * NC * s0 + (size_t)i * NC;
            double gc[3][NC];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
#pragma unroll
                for (int k = 0; k < NC; ++k) gc[ax][k] = 0.0;
            double phi = 0.0, dT = 0.0, T = 0.0;
            if (solved) {
                T = a.times[s0 + i];
                double c[3][NC];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_load<NC>(a.coeff + at + (size_t)ax * axs, c[ax], a.al16 != 0);
                for (int s = 0; s <= a.K; ++s) {
                    const double tau = (double)s * inv_K, t = tau * T;
                    const double om = (s == 0 || s == a.K) ? 0.5 : 1.0;
                    double p[3], v[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        double pp = c[ax][NC - 1], pv = topt_falling(NC - 1, 1) * c[ax][NC - 1];
#pragma unroll
                        for (int k = NC - 2; k >= 0; --k) {
                            pp = fma(pp, t, c[ax][k]);
                            if (k >= 1) pv = fma(pv, t, topt_falling(k, 1) * c[ax][k]);
                        }
                        p[ax] = pp; v[ax] = pv;
                    }
                    double d, gd[3];
                    if (!esdf_sample(a.map, p[0], p[1], p[2], d, gd)) { ++n_out; continue; }
                    neg_min = fmax(neg_min, -d);
                    const double x = fmax(0.0, (a.d_safe - d) * a.inv_safe);
                    if (x > 0.0) {
                        phi = fma(om, a.weight * x * (x * x), phi);
                        const double e = -3.0 * a.weight * (x * x) * a.inv_safe;
                        dT = fma(om * tau, e * fma(gd[0], v[0], fma(gd[1], v[1], gd[2] * v[2])), dT);
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const double wg = om * e * gd[ax];
                            double pk = t;
                            gc[ax][0] += wg;
#pragma unroll
                            for (int k = 1; k < NC; ++k) {
                                gc[ax][k] = fma(wg, pk, gc[ax][k]);
                                pk *= t;
                            }
                        }
                    }
                }
            }
            const double h = T * inv_K;
            Phi = fma(h, phi, Phi);
            if (a.grad_times) a.grad_times[s0 + i] = fma(h, dT, phi * inv_K);
            if (a.grad_coeff)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) lim_store<NC>(a.grad_coeff + at + (size_t)ax * axs, gc[ax], h, a.al16 != 0);
        }
        Phi = topt_group_sum(Phi);
        neg_min = topt_group_max(neg_min);
#pragma unroll
        for (int dl = 1; dl < LPT; dl <<= 1) n_out += __shfl_xor(n_out, dl, 64);
        if (live && sub == 0) {
            if (a.penalty) a.penalty[b] = Phi;
            if (a.min_dist) a.min_dist[b] = neg_min == -INFINITY ? a.map.max_dist : -neg_min;
            if (a.outside) a.outside[b] = n_out;
        }
    }
}

#endif  // UAVQP_KERNEL_TU || UAVQP_SINGLE_TU

}  // namespace uavqp
