// uavqp_esdf.h -- host side of uavqp_esdf_* and uavqp_clearance_penalty_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_limits.h (whose argument checks and staging it follows).  Kernels: qp_esdf.h (translation unit k_esdf.hip).
// A map owns ONE device buffer, laid out through Carve at creation: occupancy bytes, the two int32 fields, the float64 distances.
// Nothing is allocated afterwards; rasterise, update, query and penalty are launches on the ctx stream with nothing read back.
#pragma once

struct uavqp_esdf {
    int device = 0;
    int dims[3] = {0, 0, 0};
    double origin[3] = {0, 0, 0};
    double res = 0, max_dist = 0;
    size_t n_vox = 0;
    DevBuf buf;
    uint8_t* occ = nullptr;
    int32_t* sq_pos = nullptr;
    int32_t* sq_neg = nullptr;
    double* dist = nullptr;
    bool updated = false;
};

static uavqp::EsdfView esdf_view(const uavqp_esdf* m) {
    uavqp::EsdfView v;
    v.nx = m->dims[0]; v.ny = m->dims[1]; v.nz = m->dims[2];
    v.ox = m->origin[0]; v.oy = m->origin[1]; v.oz = m->origin[2];
    v.hx = m->origin[0] + (double)m->dims[0] * m->res;
    v.hy = m->origin[1] + (double)m->dims[1] * m->res;
    v.hz = m->origin[2] + (double)m->dims[2] * m->res;
    v.res = m->res; v.inv_res = 1.0 / m->res; v.max_dist = m->max_dist;
    v.dist = m->dist;
    return v;
}

static bool esdf_usable(const uavqp_ctx* ctx, const uavqp_esdf* m) { return ctx && m && m->device == ctx->device; }

extern "C" int uavqp_esdf_create(uavqp_ctx* ctx, const int32_t dims[3], const double origin[3], double resolution, double max_dist,
                                 uavqp_esdf** out) {
    if (!ctx || !dims || !origin || !out) return UAVQP_ERR_INVALID_ARG;
    *out = nullptr;
    size_t n_vox = 1;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 1 || dims[k] > 1024 || !(origin[k] > -INFINITY && origin[k] < INFINITY)) return UAVQP_ERR_INVALID_ARG;
        n_vox *= (size_t)dims[k];
    }
    if (n_vox > ((size_t)1 << 30)) return UAVQP_ERR_INVALID_ARG;
    if (!(resolution > 0.0 && resolution < INFINITY) || !(max_dist > 0.0 && max_dist < INFINITY)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp_esdf* m = new (std::nothrow) uavqp_esdf();
    if (!m) return UAVQP_ERR_ALLOC;
    m->device = ctx->device;
    for (int k = 0; k < 3; ++k) { m->dims[k] = dims[k]; m->origin[k] = origin[k]; }
    m->res = resolution; m->max_dist = max_dist; m->n_vox = n_vox;
    Carve c;
    const int i_occ = c.add(n_vox), i_pos = c.add(sizeof(int32_t) * n_vox), i_neg = c.add(sizeof(int32_t) * n_vox),
              i_dist = c.add(sizeof(double) * n_vox);
    int rc = carve_on(ctx->stream, m->buf, c);
    if (rc == UAVQP_OK && hipMemsetAsync(c.at<uint8_t>(i_occ), 0, n_vox, ctx->stream) != hipSuccess) {
        g_last_error = "uavqp_esdf_create: clearing the occupancy grid failed";
        rc = UAVQP_ERR_HIP;
    }
    if (rc != UAVQP_OK) {
        dev_free(m->buf);
        delete m;
        return rc;
    }
    m->occ = c.at<uint8_t>(i_occ); m->sq_pos = c.at<int32_t>(i_pos); m->sq_neg = c.at<int32_t>(i_neg); m->dist = c.at<double>(i_dist);
    *out = m;
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_destroy(uavqp_ctx* ctx, uavqp_esdf* esdf) {
    if (!esdf) return UAVQP_OK;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    (void)hipSetDevice(esdf->device);
    dev_free(esdf->buf);
    delete esdf;
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_set_occupancy_device(uavqp_ctx* ctx, uavqp_esdf* esdf, const uint8_t* d_occ) {
    if (!esdf_usable(ctx, esdf) || !d_occ) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    UAVQP_HIP(hipMemcpyAsync(esdf->occ, d_occ, esdf->n_vox, hipMemcpyDeviceToDevice, ctx->stream));
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_rasterize_cloud_device(uavqp_ctx* ctx, uavqp_esdf* esdf, const double* d_obstacles, int n_obs, int inflate_xy,
                                                 int inflate_z, int clear_first) {
    if (!esdf_usable(ctx, esdf) || n_obs < 0 || (n_obs > 0 && !d_obstacles)) return UAVQP_ERR_INVALID_ARG;
    if (inflate_xy < 0 || inflate_z < 0 || inflate_xy > 1024 || inflate_z > 1024) return UAVQP_ERR_INVALID_ARG;
    // (the lanes are counted in a long long: offsets <= 2049^3 < 2^34, refused together with a cloud that would carry the product past 2^62)
    if ((2.0 * inflate_xy + 1) * (2.0 * inflate_xy + 1) * (2.0 * inflate_z + 1) * (double)n_obs > 4.0e18) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    if (clear_first) UAVQP_HIP(hipMemsetAsync(esdf->occ, 0, esdf->n_vox, ctx->stream));
    if (n_obs == 0) return UAVQP_OK;
    uavqp::EsdfRasterArgs a;
    a.nx = esdf->dims[0]; a.ny = esdf->dims[1]; a.nz = esdf->dims[2];
    a.ox = esdf->origin[0]; a.oy = esdf->origin[1]; a.oz = esdf->origin[2];
    a.res = esdf->res; a.inv_res = 1.0 / esdf->res;
    a.pts = d_obstacles; a.n_pts = n_obs; a.ixy = inflate_xy; a.iz = inflate_z; a.occ = esdf->occ;
    const long long w = 2LL * inflate_xy + 1, total = w * w * (2LL * inflate_z + 1) * n_obs;
    long long grid = (total + uavqp::ESDF_BLOCK - 1) / uavqp::ESDF_BLOCK;
    if (grid > (long long)ctx->num_cus * 32) grid = (long long)ctx->num_cus * 32;
    hipLaunchKernelGGL(uavqp::esdf_raster_kernel, dim3((unsigned)grid), dim3(uavqp::ESDF_BLOCK), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_update_device(uavqp_ctx* ctx, uavqp_esdf* esdf) {
    if (!esdf_usable(ctx, esdf)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int nx = esdf->dims[0], ny = esdf->dims[1], nz = esdf->dims[2];
    uavqp::EsdfArgs a;
    a.nx = nx; a.ny = ny; a.nz = nz;
    a.occ = esdf->occ; a.sq_pos = esdf->sq_pos; a.sq_neg = esdf->sq_neg; a.dist = esdf->dist;
    a.res = esdf->res; a.max_dist = esdf->max_dist;
    const dim3 block(uavqp::ESDF_BLOCK);
    // z: whole consecutive lines, as many as the tile holds
    const int lines = nx * ny, lpb = std::max(1, uavqp::ESDF_TILE / nz);
    hipLaunchKernelGGL(uavqp::esdf_z_kernel, dim3((unsigned)((lines + lpb - 1) / lpb)), block, 0, ctx->stream, a, lpb);
    // y: one block per (x, tile of z); x: one block per (y, tile of z).  The tile holds (length of the axis) x zt entries.
    const int zt_y = std::max(1, std::min(nz, uavqp::ESDF_TILE / ny)), nt_y = (nz + zt_y - 1) / zt_y;
    hipLaunchKernelGGL(uavqp::esdf_axis_kernel<false>, dim3((unsigned)(nx * nt_y)), block, 0, ctx->stream, a, ny, nz, ny * nz, zt_y, nt_y);
    const int zt_x = std::max(1, std::min(nz, uavqp::ESDF_TILE / nx)), nt_x = (nz + zt_x - 1) / zt_x;
    hipLaunchKernelGGL(uavqp::esdf_axis_kernel<true>, dim3((unsigned)(ny * nt_x)), block, 0, ctx->stream, a, nx, ny * nz, nz, zt_x, nt_x);
    UAVQP_HIP(hipGetLastError());
    esdf->updated = true;
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_read_device(uavqp_ctx* ctx, uavqp_esdf* esdf, uint8_t* d_occ, int32_t* d_sq_pos, int32_t* d_sq_neg, double* d_dist) {
    if (!esdf_usable(ctx, esdf)) return UAVQP_ERR_INVALID_ARG;
    if ((d_sq_pos || d_sq_neg || d_dist) && !esdf->updated) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = esdf->n_vox;
    if (d_occ) UAVQP_HIP(hipMemcpyAsync(d_occ, esdf->occ, n, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_sq_pos) UAVQP_HIP(hipMemcpyAsync(d_sq_pos, esdf->sq_pos, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_sq_neg) UAVQP_HIP(hipMemcpyAsync(d_sq_neg, esdf->sq_neg, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_dist) UAVQP_HIP(hipMemcpyAsync(d_dist, esdf->dist, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream));
    return UAVQP_OK;
}

// (arguments checked by the callers)
static int esdf_query_enqueue(uavqp_ctx* ctx, const uavqp_esdf* esdf, int n_pts, const double* d_pts, double* d_dist, double* d_grad,
                              uint8_t* d_inside) {
    uavqp::EsdfQueryArgs a;
    a.map = esdf_view(esdf);
    a.n_pts = n_pts; a.pts = d_pts; a.dist = d_dist; a.grad = d_grad; a.inside = d_inside;
    long long grid = ((long long)n_pts + uavqp::ESDF_BLOCK - 1) / uavqp::ESDF_BLOCK;
    if (grid > (long long)ctx->num_cus * 32) grid = (long long)ctx->num_cus * 32;
    hipLaunchKernelGGL(uavqp::esdf_query_kernel, dim3((unsigned)grid), dim3(uavqp::ESDF_BLOCK), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_esdf_query_device(uavqp_ctx* ctx, uavqp_esdf* esdf, int n_pts, const double* d_pts, double* d_dist, double* d_grad,
                                       uint8_t* d_inside) {
    if (!esdf_usable(ctx, esdf) || !esdf->updated || n_pts < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_pts == 0 || (!d_dist && !d_grad && !d_inside)) return UAVQP_OK;
    if (!d_pts) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return esdf_query_enqueue(ctx, esdf, n_pts, d_pts, d_dist, d_grad, d_inside);
}

extern "C" int uavqp_esdf_query_host(uavqp_ctx* ctx, uavqp_esdf* esdf, int n_pts, const double* pts, double* dist, double* grad,
                                     uint8_t* inside) {
    if (!esdf_usable(ctx, esdf) || !esdf->updated || n_pts < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_pts == 0 || (!dist && !grad && !inside)) return UAVQP_OK;
    if (!pts) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_pts;
    Stage st;
    const int i_p = st.in(pts, sizeof(double) * 3 * n);
    const int i_d = dist ? st.out(dist, sizeof(double) * n) : -1;
    const int i_g = grad ? st.out(grad, sizeof(double) * 3 * n) : -1;
    const int i_in = inside ? st.out(inside, n) : -1;
    int rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = esdf_query_enqueue(ctx, esdf, n_pts, st.at<double>(i_p), st.at<double>(i_d), st.at<double>(i_g), st.at<uint8_t>(i_in));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_esdf_query_host");
}

extern "C" void uavqp_default_clearance_params(uavqp_clearance_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_clearance_params);
    p->samples_per_seg = 8;   // as uavqp_default_limit_params
    p->d_safe = 0.5;
    p->weight = 1e3;
}

static bool clearance_params_valid(const uavqp_clearance_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_clearance_params)) return false;
    if (p->samples_per_seg < 1) return false;
    if (!(p->d_safe > 0.0 && p->d_safe < INFINITY) || !(p->weight >= 0.0 && p->weight < INFINITY)) return false;
    return true;
}

// (arguments checked by the callers)
static int clearance_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_esdf* esdf, const uavqp_clearance_params& P, double* d_penalty,
                                     double* d_grad_coeff, double* d_grad_times, double* d_min_dist, int32_t* d_outside) {
    uavqp::ClearanceArgs a;
    solved_fill(a, B);
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.min_dist = d_min_dist; a.outside = d_outside;
    a.K = P.samples_per_seg;
    a.al16 = coeff_al16(B.coeff, d_grad_coeff);
    a.d_safe = P.d_safe; a.inv_safe = 1.0 / P.d_safe; a.weight = P.weight;
    a.map = esdf_view(esdf);
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::clearance_penalty_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_clearance_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                              const double* d_times, const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                              const uavqp_clearance_params* params, double* d_penalty, double* d_grad_coeff,
                                              double* d_grad_times, double* d_min_dist, int32_t* d_outside) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return esdf_usable(ctx, esdf) && esdf->updated && clearance_params_valid(params); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_min_dist || d_outside, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return clearance_penalty_enqueue(ctx, B, esdf, *params, d_penalty, d_grad_coeff, d_grad_times, d_min_dist, d_outside);
}

extern "C" int uavqp_clearance_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                            const double* times, const double* coeff, const int32_t* status, const uavqp_esdf* esdf,
                                            const uavqp_clearance_params* params, double* penalty, double* grad_coeff, double* grad_times,
                                            double* min_dist, int32_t* outside) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return esdf_usable(ctx, esdf) && esdf->updated && clearance_params_valid(params); },
                               penalty || grad_coeff || grad_times || min_dist || outside, &run);
    if (!run) return rc;
    BatchShape sh;
    rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_p = penalty ? st.out(penalty, sizeof(double) * n) : -1;
    const int i_g = grad_coeff ? st.out(grad_coeff, sizeof(double) * 3 * 2 * r * tot) : -1;
    const int i_gt = grad_times ? st.out(grad_times, sizeof(double) * tot) : -1;
    const int i_md = min_dist ? st.out(min_dist, sizeof(double) * n) : -1;
    const int i_o = outside ? st.out(outside, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = clearance_penalty_enqueue(ctx, in.device(st), esdf, *params, st.at<double>(i_p), st.at<double>(i_g), st.at<double>(i_gt),
                                   st.at<double>(i_md), st.at<int32_t>(i_o));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_clearance_penalty_host");
}
