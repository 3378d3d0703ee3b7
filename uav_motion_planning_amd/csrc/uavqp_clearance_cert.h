// uavqp_clearance_cert.h -- host side of uavqp_clearance_certificate_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_esdf.h (the map); argument check and staging follow uavqp_envelope.h.  Kernel: qp_clearance_cert.h (translation unit k_clearance_cert.hip).
// One launch, nothing allocated, no workspace, nothing read back; the map stays a device object in both entries.
#pragma once

extern "C" void uavqp_default_clearance_cert_params(uavqp_clearance_cert_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_clearance_cert_params);
    p->depth = 4;      // as uavqp_default_envelope_params: 16 leaves
    p->d_req = 0.5;    // the d_safe of uavqp_default_clearance_params
}

static bool clearance_cert_params_valid(const uavqp_clearance_cert_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_clearance_cert_params)) return false;
    if (p->depth < 0 || p->depth > 8) return false;
    return p->d_req > 0.0 && p->d_req < INFINITY;
}

// the checks the two entries share; *skip: nothing to do (UAVQP_OK)
static int clearance_cert_args_check(const uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                     const double* times, const double* coeff, const uavqp_esdf* esdf,
                                     const uavqp_clearance_cert_params* params, bool any_output, bool* skip) {
    *skip = false;
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!esdf_usable(ctx, esdf) || !esdf->updated || !clearance_cert_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || !any_output) { *skip = true; return UAVQP_OK; }
    if (!times || !coeff || (uniform_segments == 0 && !seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    return UAVQP_OK;
}

// (arguments checked by the callers)
static int clearance_cert_enqueue(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                  const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf, const uavqp_clearance_cert_params& P,
                                  double* d_clear, int32_t* d_witness, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    uavqp::ClearanceCertArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.status = d_status;
    a.sq_pos = esdf->sq_pos;
    const uavqp::EsdfView v = esdf_view(esdf);   // (origin, top and 1 / res as every kernel on this map sees them)
    a.nx = v.nx; a.ny = v.ny; a.nz = v.nz;
    a.ox = v.ox; a.oy = v.oy; a.oz = v.oz; a.hx = v.hx; a.hy = v.hy; a.hz = v.hz;
    a.res = v.res; a.inv_res = v.inv_res;
    double big = 0.0;
    for (double x : {v.ox, v.oy, v.oz, v.hx, v.hy, v.hz}) big = std::max(big, std::fabs(x));
    a.mag = big + v.res * std::sqrt((double)v.nx * v.nx + (double)v.ny * v.ny + (double)v.nz * v.nz);
    a.d_req = P.d_req; a.depth = P.depth;
    a.clear = d_clear; a.witness = d_witness; a.peak = d_peak; a.seg_verdict = d_seg_verdict; a.verdict = d_verdict;
    int grid = topt_grid(ctx, n_traj);
    if (ctx->clearance_cert_blocks > 0) grid = std::min(grid, ctx->clearance_cert_blocks);   // (the rest is taken by the grid-stride loop)
    if (r == 3)
        hipLaunchKernelGGL(uavqp::clearance_cert_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::clearance_cert_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_clearance_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                  const double* d_times, const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                                  const uavqp_clearance_cert_params* params, double* d_clear, int32_t* d_witness, double* d_peak,
                                                  int32_t* d_seg_verdict, int32_t* d_verdict) {
    bool skip;
    const int rc = clearance_cert_args_check(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, esdf, params,
                                             d_clear || d_witness || d_peak || d_seg_verdict || d_verdict, &skip);
    if (rc != UAVQP_OK || skip) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return clearance_cert_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status, esdf, *params, d_clear, d_witness,
                                  d_peak, d_seg_verdict, d_verdict);
}

extern "C" int uavqp_clearance_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                                const double* times, const double* coeff, const int32_t* status, const uavqp_esdf* esdf,
                                                const uavqp_clearance_cert_params* params, double* clear, int32_t* witness, double* peak,
                                                int32_t* seg_verdict, int32_t* verdict) {
    bool skip;
    int rc = clearance_cert_args_check(ctx, r, n_traj, uniform_segments, seg_offsets, times, coeff, esdf, params,
                                       clear || witness || peak || seg_verdict || verdict, &skip);
    if (rc != UAVQP_OK || skip) return rc;
    BatchShape sh;
    rc = batch_shape(n_traj, uniform_segments, 0, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_c = st.in(coeff, sizeof(double) * 3 * 2 * r * tot);
    const int i_st = status ? st.in(status, sizeof(int32_t) * n) : -1;
    const int i_cl = clear ? st.out(clear, sizeof(double) * 2 * tot) : -1;
    const int i_w = witness ? st.out(witness, sizeof(int32_t) * tot) : -1;
    const int i_p = peak ? st.out(peak, sizeof(double) * 2 * n) : -1;
    const int i_sv = seg_verdict ? st.out(seg_verdict, sizeof(int32_t) * tot) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = clearance_cert_enqueue(ctx, r, n_traj, uniform_segments, st.at<int32_t>(i_off), st.at<double>(i_t), st.at<double>(i_c),
                                st.at<int32_t>(i_st), esdf, *params, st.at<double>(i_cl), st.at<int32_t>(i_w), st.at<double>(i_p),
                                st.at<int32_t>(i_sv), st.at<int32_t>(i_v));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_clearance_certificate_host");
}
