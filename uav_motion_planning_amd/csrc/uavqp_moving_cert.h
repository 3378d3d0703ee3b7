// uavqp_moving_cert.h -- host side of uavqp_moving_certificate_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_moving.h, whose check of the obstacle struct (moving_obstacles_valid, moving_host_check) and staging of its arrays (MovingStage)
// it shares.  Kernel: qp_moving_cert.h (translation unit k_moving_cert.hip).  One launch, nothing allocated, nothing read back.
#pragma once

extern "C" void uavqp_default_moving_cert_params(uavqp_moving_cert_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_moving_cert_params);
    p->depth = 3;        // eight leaves per segment: the witnesses are the samples of uavqp_default_moving_params
    p->downwash = 1.0;
    p->d_req = 1.0;      // the d_safe of uavqp_default_moving_params
}

static bool moving_cert_params_valid(const uavqp_moving_cert_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_moving_cert_params)) return false;
    if (p->depth < 0 || p->depth > 6) return false;
    if (!(p->downwash >= 1.0 && p->downwash < INFINITY)) return false;
    if (!(p->d_req > 0.0 && p->d_req < INFINITY)) return false;
    return true;
}

// (arguments checked by the callers)
static int moving_cert_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_moving_obstacles& O, const uavqp_moving_cert_params& P,
                               double* d_gap, int32_t* d_where, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    uavqp::MovingCertArgs a;
    solved_fill(a, B);
    a.n_obs = O.n_obs; a.o_uniform = O.uniform_segments; a.n_sets = O.n_sets; a.o_seg_offsets = O.seg_offsets; a.o_times = O.times;
    a.o_coeff = O.coeff; a.o_start = O.start; a.o_radius = O.radius; a.set_offsets = O.set_offsets; a.traj_set = O.traj_set;
    a.traj_start = O.traj_start;
    a.gap = d_gap; a.where = d_where; a.peak = d_peak; a.seg_verdict = d_seg_verdict; a.verdict = d_verdict;
    a.depth = P.depth; a.inv_dw = 1.0 / P.downwash; a.d_req = P.d_req;
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::moving_cert_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_moving_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                               const double* d_times, const double* d_coeff, const int32_t* d_status,
                                               const uavqp_moving_obstacles* obstacles, const uavqp_moving_cert_params* params, double* d_gap,
                                               int32_t* d_where, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return moving_cert_params_valid(params) && moving_obstacles_valid(obstacles); },
                                     d_gap || d_where || d_peak || d_seg_verdict || d_verdict, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return moving_cert_enqueue(ctx, B, *obstacles, *params, d_gap, d_where, d_peak, d_seg_verdict, d_verdict);
}

extern "C" int uavqp_moving_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                             const double* times, const double* coeff, const int32_t* status,
                                             const uavqp_moving_obstacles* obstacles, const uavqp_moving_cert_params* params, double* gap,
                                             int32_t* where, double* peak, int32_t* seg_verdict, int32_t* verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return moving_cert_params_valid(params) && moving_obstacles_valid(obstacles); },
                               gap || where || peak || seg_verdict || verdict, &run);
    if (!run) return rc;
    BatchShape sh, osh;
    rc = solved_shape(B, &sh);
    if (rc == UAVQP_OK) rc = moving_host_check(*obstacles, n_traj, &osh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    MovingStage ms;
    ms.declare(st, *obstacles, r, n_traj, osh);
    const int i_g = gap ? st.out(gap, sizeof(double) * 2 * tot) : -1;
    const int i_w = where ? st.out(where, sizeof(int32_t) * 4 * tot) : -1;
    const int i_p = peak ? st.out(peak, sizeof(double) * 2 * n) : -1;
    const int i_sv = seg_verdict ? st.out(seg_verdict, sizeof(int32_t) * tot) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = moving_cert_enqueue(ctx, in.device(st), ms.device(st, *obstacles), *params, st.at<double>(i_g), st.at<int32_t>(i_w), st.at<double>(i_p),
                             st.at<int32_t>(i_sv), st.at<int32_t>(i_v));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_moving_certificate_host");
}
