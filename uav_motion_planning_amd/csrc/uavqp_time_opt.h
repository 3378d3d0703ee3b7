// uavqp_time_opt.h -- host side of uavqp_cost_time_gradient_device / uavqp_time_optimize_device / _host (include/uavqp.h): included by
// uavqp.hip behind the entry points it sequences.  Kernels: qp_time_opt.h (translation unit k_timeopt.hip).
//
// The optimiser is host-side C++ sequencing like the corridor pipeline, but with NO data-dependent control flow on the host: the number of
// launches is fixed by max_iters, every accept / reject is taken per trajectory on the device, and nothing is read back inside the loop:
//     clamp -> solve(times) -> step<INIT> -> max_iters x { solve(trial) -> step<ITER> } -> solve(times)
// The inner solve is uavqp_solve_batch_device itself, so the coefficients handed back are those of a plain solve at the durations handed back.
// With limits (uavqp_time_optimize_limits_device, uavqp_limits.h) every step is preceded by the penalty of the point just solved and the
// backward pass of its coefficient gradient:
//     clamp -> solve(times) -> penalty, backward -> step<INIT> -> max_iters x { solve(trial) -> penalty, backward -> step<ITER> } -> solve(times)
#pragma once

// (uavqp_limits.h, included behind this file and uavqp_adjoint.h)
static int limit_penalty_enqueue(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                 const double* d_coeff, const int32_t* d_status, const uavqp_limit_params& L, double* d_penalty,
                                 double* d_grad_coeff, double* d_grad_times, double* d_peak);

extern "C" void uavqp_default_time_opt_params(uavqp_time_opt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_time_opt_params);
    p->max_iters = 24;        // measured: within 2 % of L-BFGS-B's decrease after 10 trials, within 1 % after 20
    p->time_weight = 50.0;
    p->t_min = 1e-2;
    p->t_max = 1e2;
    p->initial_step = 0.1;    // the first trial moves the most sensitive duration by 10 %
    p->armijo_c = 1e-4;
    p->shrink = 0.5;
    p->grow = 2.0;
}

static int topt_grid(const uavqp_ctx* ctx, int n_traj) {
    long long g = ((long long)n_traj * uavqp::TOPT_LPT + 63) / 64;
    if (g > (long long)ctx->num_cus * 32) g = (long long)ctx->num_cus * 32;
    return (int)g;
}

extern "C" int uavqp_cost_time_gradient_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                               const double* d_times, const double* d_coeff, double* d_cost, double* d_grad) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || (!d_cost && !d_grad)) return UAVQP_OK;
    if (!d_times || !d_coeff || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::CostGradArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff;
    a.cost = d_cost; a.grad = d_grad;
    const int grid = topt_grid(ctx, n_traj);
    if (r == 3)
        hipLaunchKernelGGL(uavqp::cost_grad_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::cost_grad_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

static bool topt_params_valid(const uavqp_time_opt_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_time_opt_params)) return false;
    if (p->max_iters < 0 || p->max_iters > 100000) return false;
    if (!(p->time_weight > 0.0 && p->time_weight < INFINITY)) return false;
    if (!(p->t_min > 0.0) || !(p->t_min <= p->t_max) || !(p->t_max < INFINITY)) return false;
    if (!(p->initial_step > 0.0 && p->initial_step < INFINITY)) return false;
    if (!(p->armijo_c > 0.0 && p->armijo_c < 1.0)) return false;
    if (!(p->shrink > 0.0 && p->shrink < 1.0)) return false;
    if (!(p->grow >= 1.0 && p->grow < INFINITY)) return false;
    return true;
}

// limits = null: uavqp_time_optimize_device.  Otherwise (validated by the caller) f and its gradient carry the limit penalty.
static int time_optimize_run(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                             const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                             const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                             int32_t* d_accepted_out, const uavqp_limit_params* limits, double* d_peak_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || total_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!topt_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out || !d_objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments > 0 && (long long)total_segments != (long long)uniform_segments * n_traj) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const uavqp_time_opt_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments;

    Carve c;
    const int i_tr = c.add(sizeof(double) * tot), i_gb = c.add(sizeof(double) * tot), i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n);
    const int i_nd = c.add(sizeof(double) * n), i_ac = c.add(sizeof(int32_t) * n), i_st = c.add(sizeof(int32_t) * n);
    const bool lim = limits != nullptr;
    const int i_lg = c.add(sizeof(double) * 3 * 2 * r * tot, lim), i_le = c.add(sizeof(double) * tot, lim), i_lt = c.add(sizeof(double) * tot, lim);
    const int i_lp = c.add(sizeof(double) * n, lim);
    int rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;
    int32_t* d_st_loop = c.at<int32_t>(i_st);
    int32_t* d_st_final = d_status_out ? d_status_out : d_st_loop;

    uavqp::TimeOptArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
    a.times = d_times; a.trial = c.at<double>(i_tr); a.gbest = c.at<double>(i_gb);
    a.coeff = d_coeff_out; a.status = P.max_iters > 0 ? d_st_loop : d_st_final;
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.active = c.at<int32_t>(i_ac);
    a.objective = d_objective_out; a.accepted = d_accepted_out;
    a.w = P.time_weight; a.t_min = P.t_min; a.t_max = P.t_max; a.initial_step = P.initial_step; a.armijo = P.armijo_c;
    a.shrink = P.shrink; a.grow = P.grow;
    a.propose = P.max_iters > 0 ? 1 : 0;
    a.phi = c.at<double>(i_lp); a.lim_explicit = c.at<double>(i_le); a.lim_through = c.at<double>(i_lt);
    // the penalty of the point `coeff` was solved at, its gradient in the coefficients, and that gradient taken through the minimiser
    auto penalty_and_backward = [&](const double* d_T, const int32_t* d_st) -> int {
        int e = limit_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_T, d_coeff_out, d_st, *limits, c.at<double>(i_lp),
                                      c.at<double>(i_lg), c.at<double>(i_le), nullptr);
        if (e != UAVQP_OK) return e;
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_T, d_bc,
                                           d_coeff_out, d_st, c.at<double>(i_lg), c.at<double>(i_lt), nullptr, nullptr);
    };
    const int grid = topt_grid(ctx, n_traj);
    hipStream_t s = ctx->stream;
#define UAVQP_TOPT_LAUNCH(KERNEL_)                                                                            \
    do {                                                                                                      \
        if (r == 3) hipLaunchKernelGGL((uavqp::KERNEL_(3)), dim3(grid), dim3(64), 0, s, a);                    \
        else hipLaunchKernelGGL((uavqp::KERNEL_(4)), dim3(grid), dim3(64), 0, s, a);                           \
        UAVQP_HIP(hipGetLastError());                                                                         \
    } while (0)
#define UAVQP_TOPT_CLAMP(R_) time_opt_clamp_kernel<R_>
#define UAVQP_TOPT_INIT(R_) time_opt_step_kernel<R_, true>
#define UAVQP_TOPT_ITER(R_) time_opt_step_kernel<R_, false>
#define UAVQP_TOPT_INIT_LIM(R_) time_opt_step_kernel<R_, true, true>
#define UAVQP_TOPT_ITER_LIM(R_) time_opt_step_kernel<R_, false, true>
    UAVQP_TOPT_LAUNCH(UAVQP_TOPT_CLAMP);
    rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                  const_cast<int32_t*>(a.status));
    if (rc != UAVQP_OK) return rc;
    if (lim) {
        rc = penalty_and_backward(d_times, a.status);
        if (rc != UAVQP_OK) return rc;
        UAVQP_TOPT_LAUNCH(UAVQP_TOPT_INIT_LIM);
    } else {
        UAVQP_TOPT_LAUNCH(UAVQP_TOPT_INIT);
    }
    for (int it = 0; it < P.max_iters; ++it) {
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, a.trial, d_bc, d_coeff_out,
                                      d_st_loop);
        if (rc != UAVQP_OK) return rc;
        a.propose = it + 1 < P.max_iters ? 1 : 0;
        if (lim) {
            rc = penalty_and_backward(a.trial, d_st_loop);
            if (rc != UAVQP_OK) return rc;
            UAVQP_TOPT_LAUNCH(UAVQP_TOPT_ITER_LIM);
        } else {
            UAVQP_TOPT_LAUNCH(UAVQP_TOPT_ITER);
        }
    }
    if (P.max_iters > 0) {
        // the coefficients on return are the solve AT the accepted durations (the last trial of a trajectory may have been rejected, and a
        // trajectory that never took part must carry what a plain solve leaves there)
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                      d_st_final);
        if (rc != UAVQP_OK) return rc;
    }
    if (lim && d_peak_out)   // the sampled peaks of what is handed back
        rc = limit_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st_final, *limits, nullptr, nullptr,
                                   nullptr, d_peak_out);
#undef UAVQP_TOPT_LAUNCH
#undef UAVQP_TOPT_CLAMP
#undef UAVQP_TOPT_INIT
#undef UAVQP_TOPT_ITER
#undef UAVQP_TOPT_INIT_LIM
#undef UAVQP_TOPT_ITER_LIM
    return rc;
}

extern "C" int uavqp_time_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                          const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                          const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                                          double* d_objective_out, int32_t* d_accepted_out) {
    return time_optimize_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, params,
                             d_coeff_out, d_status_out, d_objective_out, d_accepted_out, nullptr, nullptr);
}

static int time_optimize_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                  const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                                  double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out,
                                  const uavqp_limit_params* limits, double* peak_out, const char* who) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!topt_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out || !objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.in(waypoints, sizeof(double) * 3 * (tot + n));
    const int i_t = st.inout(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_obj = st.out(objective_out, sizeof(double) * 2 * n), i_acc = st.out(accepted_out, sizeof(int32_t) * n);
    const int i_pk = limits && peak_out ? st.out(peak_out, sizeof(double) * 2 * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = time_optimize_run(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                           st.at<double>(i_t), st.at<double>(i_bc), params, st.at<double>(i_out), st.at<int32_t>(i_st), st.at<double>(i_obj),
                           st.at<int32_t>(i_acc), limits, st.at<double>(i_pk));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, who);
}

extern "C" int uavqp_time_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                        const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                                        double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out) {
    return time_optimize_run_host(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, params, coeff_out, status_out,
                                  objective_out, accepted_out, nullptr, nullptr, "uavqp_time_optimize_host");
}
