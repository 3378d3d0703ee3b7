// uavqp_limits.h -- host side of uavqp_limit_penalty_device / _host and uavqp_time_optimize_limits_device / _host (include/uavqp.h):
// included by uavqp.hip behind uavqp_time_opt.h (whose sequencing the limit-aware optimiser shares) and uavqp_adjoint.h.
// Kernels: qp_limits.h (translation unit k_limits.hip).  The penalty is one launch, nothing allocated, nothing read back.
#pragma once

extern "C" void uavqp_default_limit_params(uavqp_limit_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_limit_params);
    p->samples_per_seg = 8;
    p->v_max = 7.0;       // the limits uavqp_default_pipeline_params carries
    p->a_max = 10.0;
    p->weight_v = 1e3;    // comparable with time_weight: the ratios inside the penalty are dimensionless
    p->weight_a = 1e3;
}

static bool limit_params_valid(const uavqp_limit_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_limit_params)) return false;
    if (p->samples_per_seg < 1) return false;
    if (!(p->v_max > 0.0 && p->v_max < INFINITY) || !(p->a_max > 0.0 && p->a_max < INFINITY)) return false;
    if (!(p->weight_v >= 0.0 && p->weight_v < INFINITY) || !(p->weight_a >= 0.0 && p->weight_a < INFINITY)) return false;
    return true;
}

// (arguments checked by the callers)
static int limit_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_limit_params& L, double* d_penalty, double* d_grad_coeff,
                                 double* d_grad_times, double* d_peak) {
    uavqp::LimitArgs a;
    solved_fill(a, B);
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.peak = d_peak;
    a.K = L.samples_per_seg;
    a.al16 = coeff_al16(B.coeff, d_grad_coeff);
    a.v_max = L.v_max; a.a_max = L.a_max; a.inv_v2 = 1.0 / (L.v_max * L.v_max); a.inv_a2 = 1.0 / (L.a_max * L.a_max);
    a.wv = L.weight_v; a.wa = L.weight_a;
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::limit_penalty_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_limit_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                          const double* d_times, const double* d_coeff, const int32_t* d_status,
                                          const uavqp_limit_params* params, double* d_penalty, double* d_grad_coeff, double* d_grad_times,
                                          double* d_peak) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return limit_params_valid(params); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_peak, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return limit_penalty_enqueue(ctx, B, *params, d_penalty, d_grad_coeff, d_grad_times, d_peak);
}

extern "C" int uavqp_limit_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                        const double* coeff, const int32_t* status, const uavqp_limit_params* params, double* penalty,
                                        double* grad_coeff, double* grad_times, double* peak) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return limit_params_valid(params); },
                               penalty || grad_coeff || grad_times || peak, &run);
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
    const int i_pk = peak ? st.out(peak, sizeof(double) * 2 * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = limit_penalty_enqueue(ctx, in.device(st), *params, st.at<double>(i_p), st.at<double>(i_g), st.at<double>(i_gt), st.at<double>(i_pk));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_limit_penalty_host");
}

extern "C" int uavqp_time_optimize_limits_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                                 const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                                 const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                                                 double* d_objective_out, int32_t* d_accepted_out, const uavqp_limit_params* limits,
                                                 double* d_peak_out) {
    if (!limit_params_valid(limits)) return UAVQP_ERR_INVALID_ARG;
    return time_optimize_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, params,
                             d_coeff_out, d_status_out, d_objective_out, d_accepted_out, limits, d_peak_out);
}

extern "C" int uavqp_time_optimize_limits_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                               const int32_t* seg_offsets, const double* waypoints, double* times, const double* bc,
                                               const uavqp_time_opt_params* params, double* coeff_out, int32_t* status_out,
                                               double* objective_out, int32_t* accepted_out, const uavqp_limit_params* limits, double* peak_out) {
    if (!limit_params_valid(limits)) return UAVQP_ERR_INVALID_ARG;
    return time_optimize_run_host(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, params, coeff_out, status_out,
                                  objective_out, accepted_out, limits, peak_out, "uavqp_time_optimize_limits_host");
}
