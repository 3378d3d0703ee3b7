// uavqp_attitude.h -- host side of uavqp_attitude_penalty_device / _host (include/uavqp.h): included by uavqp.hip behind uavqp_limits.h.
// Kernel: qp_attitude.h (translation unit k_attitude.hip).  The penalty is one launch, nothing allocated, nothing read back.
// uavqp_attitude_optimize_device (uavqp_spacetime_lbfgs.h) enqueues the accumulating variant through attitude_penalty_enqueue.
#pragma once

extern "C" void uavqp_default_attitude_params(uavqp_attitude_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_attitude_params);
    p->samples_per_seg = 8;     // as uavqp_default_limit_params
    p->gravity = 9.81;          // the constant of poly_body_frame (qp_poly.h)
    p->f_min = 3.0;             // a small racing-class multirotor: thrust between 0.3 and 2 times its weight,
    p->f_max = 20.0;
    p->tilt_max = 1.05;         // 60 degrees of tilt,
    p->rate_max = 2.1;          // 120 degrees per second of body rate
    p->weight_thrust = 1e3;     // comparable with the other penalties: the u inside the penalty are dimensionless
    p->weight_tilt = 1e3;
    p->weight_rate = 1e3;
}

static bool attitude_params_valid(const uavqp_attitude_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_attitude_params)) return false;
    if (p->samples_per_seg < 1) return false;
    if (!(p->gravity > 0.0 && p->gravity < INFINITY)) return false;
    if (!(p->f_min >= 0.0 && p->f_min < p->f_max && p->f_max < INFINITY)) return false;
    if (!(p->tilt_max > 0.0 && p->tilt_max < 1.5707963267948966)) return false;
    if (!(p->rate_max > 0.0 && p->rate_max < INFINITY)) return false;
    for (double w : {p->weight_thrust, p->weight_tilt, p->weight_rate})
        if (!(w >= 0.0 && w < INFINITY)) return false;
    return true;
}

static bool attitude_any_weight(const uavqp_attitude_params& A) { return A.weight_thrust > 0.0 || A.weight_tilt > 0.0 || A.weight_rate > 0.0; }

// (arguments checked by the callers)  accumulate (uavqp_attitude_optimize_device only, not in the C ABI): penalty, grad_coeff and grad_times
// are ADDED to what the arrays hold
static int attitude_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_attitude_params& A, double* d_penalty, double* d_grad_coeff,
                                    double* d_grad_times, double* d_peak, bool accumulate = false) {
    uavqp::AttitudeArgs a;
    solved_fill(a, B);
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.peak = d_peak;
    a.K = A.samples_per_seg;
    a.al16 = coeff_al16(B.coeff, d_grad_coeff);
    const double g2 = A.gravity * A.gravity, tn = std::tan(A.tilt_max);
    a.gravity = A.gravity; a.inv_g2 = 1.0 / g2;
    a.inv_fmax2 = 1.0 / (A.f_max * A.f_max);
    a.lo_one = A.f_min > 0.0 ? 1.0 : 0.0;
    a.inv_fmin2 = A.f_min > 0.0 ? 1.0 / (A.f_min * A.f_min) : 0.0;
    a.kappa = tn * tn;
    a.rate2 = A.rate_max * A.rate_max; a.inv_rg4 = 1.0 / (a.rate2 * g2 * g2);
    a.w_thrust = A.weight_thrust; a.w_tilt = A.weight_tilt; a.w_rate = A.weight_rate;
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r_flag(B.r, accumulate, [&](auto R, auto ACC) {
        hipLaunchKernelGGL((uavqp::attitude_penalty_kernel<decltype(R)::value, decltype(ACC)::value>), dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_attitude_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                             const double* d_times, const double* d_coeff, const int32_t* d_status,
                                             const uavqp_attitude_params* params, double* d_penalty, double* d_grad_coeff,
                                             double* d_grad_times, double* d_peak) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return attitude_params_valid(params); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_peak, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return attitude_penalty_enqueue(ctx, B, *params, d_penalty, d_grad_coeff, d_grad_times, d_peak);
}

extern "C" int uavqp_attitude_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                           const double* times, const double* coeff, const int32_t* status,
                                           const uavqp_attitude_params* params, double* penalty, double* grad_coeff, double* grad_times,
                                           double* peak) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return attitude_params_valid(params); },
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
    const int i_pk = peak ? st.out(peak, sizeof(double) * 4 * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = attitude_penalty_enqueue(ctx, in.device(st), *params, st.at<double>(i_p), st.at<double>(i_g), st.at<double>(i_gt), st.at<double>(i_pk));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_attitude_penalty_host");
}
