// uavqp_clearance_cert.h -- host side of uavqp_clearance_certificate_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_esdf.h (the map).  Kernel: qp_clearance_cert.h (translation unit k_clearance_cert.hip).
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

// (arguments checked by the callers)
static int clearance_cert_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_esdf* esdf, const uavqp_clearance_cert_params& P, double* d_clear,
                                  int32_t* d_witness, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    uavqp::ClearanceCertArgs a;
    solved_fill(a, B);
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
    int grid = topt_grid(ctx, B.n_traj);
    if (ctx->clearance_cert_blocks > 0) grid = std::min(grid, ctx->clearance_cert_blocks);   // (the rest is taken by the grid-stride loop)
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::clearance_cert_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_clearance_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                  const double* d_times, const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                                  const uavqp_clearance_cert_params* params, double* d_clear, int32_t* d_witness, double* d_peak,
                                                  int32_t* d_seg_verdict, int32_t* d_verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return esdf_usable(ctx, esdf) && esdf->updated && clearance_cert_params_valid(params); },
                                     d_clear || d_witness || d_peak || d_seg_verdict || d_verdict, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return clearance_cert_enqueue(ctx, B, esdf, *params, d_clear, d_witness, d_peak, d_seg_verdict, d_verdict);
}

extern "C" int uavqp_clearance_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                                const double* times, const double* coeff, const int32_t* status, const uavqp_esdf* esdf,
                                                const uavqp_clearance_cert_params* params, double* clear, int32_t* witness, double* peak,
                                                int32_t* seg_verdict, int32_t* verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return esdf_usable(ctx, esdf) && esdf->updated && clearance_cert_params_valid(params); },
                               clear || witness || peak || seg_verdict || verdict, &run);
    if (!run) return rc;
    BatchShape sh;
    rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_cl = clear ? st.out(clear, sizeof(double) * 2 * tot) : -1;
    const int i_w = witness ? st.out(witness, sizeof(int32_t) * tot) : -1;
    const int i_p = peak ? st.out(peak, sizeof(double) * 2 * n) : -1;
    const int i_sv = seg_verdict ? st.out(seg_verdict, sizeof(int32_t) * tot) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = clearance_cert_enqueue(ctx, in.device(st), esdf, *params, st.at<double>(i_cl), st.at<int32_t>(i_w), st.at<double>(i_p),
                                st.at<int32_t>(i_sv), st.at<int32_t>(i_v));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_clearance_certificate_host");
}
